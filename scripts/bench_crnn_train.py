"""Training the CRNN recogniser's recurrent half: `CRNNDecoder` + `CTCLoss`, forward and backward, at a batch of features
(N, 512, 1, 26) with targets, train backend "hip" (include/tpspp_crnn_train.h) against "torch" (nn.LSTM, nn.Linear,
log_softmax + nn.CTCLoss) on the same GPU.  Neither ratio is a pass bar; the default backend stays "torch".

Rows: decoder + loss forward + backward under each backend; the parts of the HIP step on their own -- the training
recurrence of the first layer (it stores gates and cell states) next to the inference recurrence, the backward through time
under the planner and under each group size, d w_hh both ways (tpspp_linear_bwd_weight on the direction-major copy of d_xg,
which the product uses, and tpspp_mm_f32 over shifted views of d_xg itself), the first layer's input projection with its
weight and data gradients and the per-call weight preparation, and the CTC loss forward and backward next to PyTorch's.
The "hip" step a second time with `set_train_compute_dtype("bf16x3")`, and per layer (lstm0: K = 512, tokens read from the
NCHW map; lstm1: K = 256, dense tokens) in fp32 and in bf16x3: the projection forward, the recurrence forward with stored
gates, the recurrence backward, d w_ih, d w_hh, dx and the per-call arrangement of the weights.

Every row: `reps` calls between two device events per region, the variants interleaved region by region, inputs rotated
over `--buffers` copies so that no call finds its own input in cache, medians over the regions with min and max
(scripts/bench_crnn.py's method).

    python scripts/bench_crnn_train.py [--batch 512] [--reps 10] [--regions 7] [--buffers 4] [--json out.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = ("hello", "tps", "crnn2016", "rectifier", "a", "mi355x", "gates", "wavefront")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from tps_pp_amd import build_decoder, build_convertor, ops
    from tps_pp_amd.losses import CTCLoss
    if not torch.cuda.is_available():
        raise SystemExit("bench_crnn_train: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    N, B, T, H = a.batch, a.buffers, 26, ops.CRNN_HIDDEN
    torch.manual_seed(0)
    conv = build_convertor(dict(type="CTCConvertor", dict_type="DICT36", with_unknown=False, lower=True))
    decs, losses = {}, {}
    decs["torch"] = build_decoder(dict(type="CRNNDecoder", in_channels=512, num_classes=conv.num_classes(),
                                       rnn_flag=True)).to(dev).train()
    decs["hip"] = copy.deepcopy(decs["torch"]).set_train_backend("hip")
    decs["hip bf16x3"] = copy.deepcopy(decs["hip"]).set_train_compute_dtype("bf16x3")
    for k in decs:
        losses[k] = CTCLoss().set_train_backend(k.split()[0])
    td = conv.str2tensor([WORDS[i % len(WORDS)] for i in range(N)])
    metas = [{} for _ in range(N)]
    feats = [torch.randn((N, 512, 1, T), device=dev).relu_() for _ in range(B)]
    it = {"i": 0}

    def rot(lst):
        it["i"] += 1
        return lst[it["i"] % B]

    def step(k):
        dec = decs[k]
        for p in dec.parameters():
            p.grad = None
        feat = rot(feats).detach().requires_grad_(True)
        loss = losses[k](dec(feat, None, None, None, train_mode=True), td, metas)["loss_ctc"]
        loss.backward()
        return loss

    # the parts, on saved operands
    l0 = decs["hip"].decoder[0]
    with torch.no_grad():
        w_ih, b, w_hh = l0._hip_weights()
        w_hh_t = w_hh.transpose(1, 2).contiguous()
        sn, sc, _, sw = feats[0].stride()
        xg = [ops.linear_fwd(f, (T, N, sw, sn, sc), w_ih, b).view(T, N, 2, 4 * H) for f in feats]
        saved = [ops.crnn_lstm_train_fwd(x, w_hh) for x in xg]
        d_out = [torch.randn((T, N, 2 * H), device=dev) for _ in range(B)]
        d_xg = [ops.crnn_lstm_bwd(d_out[i], saved[i][1], saved[i][2], w_hh_t, direction_major=True) for i in range(B)]
        logits = [torch.randn((N, T, conv.num_classes()), device=dev) * 2 for _ in range(B)]
        lens = td["target_lengths"].clamp(min=1, max=T)
        padded = torch.zeros((N, int(lens.max())), dtype=torch.int32)
        for n, t in enumerate(td["targets"]):
            padded[n, :len(t)] = t
        tg, tl, il = padded.to(dev), lens.to(dev, torch.int32), torch.full((N,), T, dtype=torch.int32, device=dev)
        ctc_saved = [ops.crnn_ctc_loss_fwd(x, tg, tl, il, 0, False, 1) for x in logits]
        one = torch.ones((1,), device=dev)
    flat, tl64, il64 = td["flatten_targets"].to(dev), lens.to(dev).long(), il.long()

    def bwd(group, direction_major=True):
        i = rot(range(B))
        return ops.crnn_lstm_bwd(d_out[i], saved[i][1], saved[i][2], w_hh_t, group, direction_major)

    def ctc_bwd():
        i = rot(range(B))
        return ops.crnn_ctc_loss_bwd(one, logits[i], tg, tl, il, ctc_saved[i][1], ctc_saved[i][3], 0, False, 1)

    def ctc_torch():
        x = rot(logits).detach().requires_grad_(True)
        F.ctc_loss(F.log_softmax(x, 2).permute(1, 0, 2), flat, il64, tl64).backward()

    def w_hh_grad():
        i = rot(range(B))
        return ops.crnn_lstm_bwd_w_hh(d_xg[i][1], saved[i][0])

    def w_hh_grad_mm():
        """The alternative without the direction-major copy: tpspp_mm_f32 over shifted views of d_xg (T, N, 2, 1024)."""
        i = rot(range(B))
        d, out = d_xg[i][0], saved[i][0]
        dw = torch.empty((2, 4 * H, H), device=dev)
        for k, (x, y) in enumerate(((d[1:, :, 0], out[:-1, :, :H]), (d[:-1, :, 1], out[1:, :, H:]))):
            ops.mm(x, (0, 1, 8 * H), y, (0, 1, 2 * H), dw[k], (0, H, 1), 1, 4 * H, H, (T - 1) * N)
        return dw

    desc0 = (T, N, sw, sn, sc)
    dx0 = torch.empty_like(feats[0])

    def w_ih_grad():
        i = rot(range(B))
        return ops.linear_bwd_weight(d_xg[i][0].view(T * N, 8 * H), feats[i], desc0, 8 * H, 512)

    def x_grad():
        return ops.linear_bwd_data(rot(d_xg)[0].view(T * N, 8 * H), w_ih, dx0, desc0)

    def weights():
        r = l0.rnn
        return (torch.cat([r.weight_ih_l0, r.weight_ih_l0_reverse]), torch.cat([r.bias_ih_l0 + r.bias_hh_l0,
                                                                               r.bias_ih_l0_reverse + r.bias_hh_l0_reverse]),
                torch.stack([ops.transpose2d(r.weight_hh_l0.detach()), ops.transpose2d(r.weight_hh_l0_reverse.detach())]))

    nograd = lambda f: (lambda: _no_grad(torch, f))  # noqa: E731

    # the five wide products of each layer, fp32 and bf16x3, on saved operands of that layer
    G = 4 * H
    layer_rows = {}
    for li, K in ((0, 512), (1, 256)):
        layer = decs["hip"].decoder[li]
        with torch.no_grad():
            lw_ih, lb, lw_hh = layer._hip_weights()
            lw_hh_t = lw_hh.transpose(1, 2).contiguous()
            xs = feats if li == 0 else [torch.randn((T, N, K), device=dev) for _ in range(B)]
            desc = desc0 if li == 0 else (T, N, N * K, K, 1)
            a_ih, a_hh = ops.arrange_mfma16(lw_ih, lb, x3=True), ops.arrange_mfma16(lw_hh, x3=True)
            a_hh_t, a_ih_t = ops.arrange_mfma16(lw_hh.transpose(1, 2), x3=True), ops.arrange_mfma16(lw_ih.t(), x3=True)
            lxg = [ops.linear_fwd(x, desc, lw_ih, lb).view(T, N, 2, G) for x in xs]
            lsv = [ops.crnn_lstm_train_fwd(x, lw_hh) for x in lxg]
            ldx = [ops.crnn_lstm_bwd(d_out[i], lsv[i][1], lsv[i][2], lw_hh_t, direction_major=True) for i in range(B)]
            dxo = torch.empty_like(xs[0])
        sdx = (dxo.stride(3), dxo.stride(0), dxo.stride(1)) if li == 0 else (N * K, K, 1)
        sd, sx = (N * 2 * G, 2 * G, 1), (N * 2 * H, 2 * H, 1)

        def parts(xs=xs, desc=desc, K=K, lw_ih=lw_ih, lb=lb, lw_hh=lw_hh, lw_hh_t=lw_hh_t, a_ih=a_ih, a_hh=a_hh, a_hh_t=a_hh_t,
                  a_ih_t=a_ih_t, lxg=lxg, lsv=lsv, ldx=ldx, dxo=dxo, sdx=sdx, layer=layer):
            def sv():
                i = rot(range(B))
                return d_out[i], lsv[i][1], lsv[i][2]

            def dwhh_bf16():
                i = rot(range(B))
                d, out = ldx[i][0], lsv[i][0]
                return (ops.linear_bwd_weight_bf16(d[1:, :, 0], sd, out[:-1, :, :H], sx, T - 1, N, G, H),
                        ops.linear_bwd_weight_bf16(d[:-1, :, 1], sd, out[1:, :, H:], sx, T - 1, N, G, H))

            def arrange():
                r = layer.rnn
                w_ih_ = torch.cat([r.weight_ih_l0, r.weight_ih_l0_reverse]).float().contiguous()
                b_ = torch.cat([r.bias_ih_l0 + r.bias_hh_l0, r.bias_ih_l0_reverse + r.bias_hh_l0_reverse]).float().contiguous()
                w_hh_ = torch.stack([r.weight_hh_l0, r.weight_hh_l0_reverse]).float().contiguous()
                return (ops.arrange_mfma16(w_ih_, b_, x3=True), ops.arrange_mfma16(w_hh_, x3=True),
                        ops.arrange_mfma16(w_hh_.transpose(1, 2), x3=True), ops.arrange_mfma16(w_ih_.t(), x3=True))

            def pair(f):
                """f(d_xg of a saved step, that step's layer input)."""
                i = rot(range(B))
                return f(ldx[i], xs[i], lsv[i][0])
            return {
                "projection forward, fp32": lambda: ops.linear_fwd(rot(xs), desc, lw_ih, lb),
                "projection forward, bf16x3": lambda: ops.linear_bf16_fwd(rot(xs), desc, a_ih),
                "recurrence forward with stored gates, fp32": lambda: ops.crnn_lstm_train_fwd(rot(lxg), lw_hh),
                "recurrence forward with stored gates, bf16x3": lambda: ops.crnn_lstm_bf16_train_fwd(rot(lxg), a_hh),
                "recurrence backward, fp32": lambda: ops.crnn_lstm_bwd(*sv(), lw_hh_t, 0, True),
                "recurrence backward, bf16x3": lambda: ops.crnn_lstm_bf16_bwd(*sv(), a_hh_t),
                "d w_ih, fp32 (with d bias)": lambda: pair(lambda d, x, o: ops.linear_bwd_weight(d[0].view(T * N, 2 * G), x, desc, 2 * G, K)),
                "d w_ih, bf16x3": lambda: pair(lambda d, x, o: ops.linear_bwd_weight_bf16(d[0], sd, x, desc[2:], T, N, 2 * G, K)),
                "d bias alone, fp32 (the bf16x3 step's)": lambda: pair(
                    lambda d, x, o: ops.linear_bwd_weight(d[0].view(T * N, 2 * G), x, desc, 2 * G, K, False, True)),
                "d w_hh, fp32": lambda: pair(lambda d, x, o: ops.crnn_lstm_bwd_w_hh(d[1], o)),
                "d w_hh, bf16x3 (shifted views)": dwhh_bf16,
                "dx, fp32": lambda: ops.linear_bwd_data(rot(ldx)[0].view(T * N, 2 * G), lw_ih, dxo, desc),
                "dx, bf16x3": lambda: ops.mm_bf16(rot(ldx)[0], sd, a_ih_t, dxo, sdx, T, N),
                "weights per call, bf16x3: four arrangements": arrange,
            }
        for name, f in parts().items():
            layer_rows[f"lstm{li} {name}"] = nograd(f)

    rows = {
        "decoder + loss, forward + backward, hip": lambda: step("hip"),
        "decoder + loss, forward + backward, hip bf16x3": lambda: step("hip bf16x3"),
        "decoder + loss, forward + backward, torch": lambda: step("torch"),
        "lstm0 recurrence forward (inference kernel)": nograd(lambda: ops.crnn_lstm(rot(xg), w_hh)),
        "lstm0 recurrence forward, saving gates and cell": nograd(lambda: ops.crnn_lstm_train_fwd(rot(xg), w_hh)),
        "lstm0 recurrence backward": nograd(lambda: bwd(0)),
        "lstm0 recurrence backward, 4 images per workgroup": nograd(lambda: bwd(4)),
        "lstm0 recurrence backward, 8 images per workgroup": nograd(lambda: bwd(8)),
        "lstm0 recurrence backward, 16 images per workgroup": nograd(lambda: bwd(16)),
        "lstm0 recurrence backward, no direction-major copy": nograd(lambda: bwd(0, False)),
        "lstm0 d w_hh (tpspp_linear_bwd_weight)": nograd(w_hh_grad),
        "lstm0 d w_hh (tpspp_mm_f32, shifted views)": nograd(w_hh_grad_mm),
        "lstm0 input projection 512 -> 2x1024 (tokens read from the NCHW map)": nograd(
            lambda: ops.linear_fwd(rot(feats), desc0, w_ih, b)),
        "lstm0 d w_ih and d bias (tpspp_linear_bwd_weight, x from the NCHW map)": nograd(w_ih_grad),
        "lstm0 dx into the NCHW map (tpspp_mm_f32)": nograd(x_grad),
        "lstm0 weights per call: cat, stack, two transposes": nograd(weights),
        "CTC loss forward, hip": nograd(lambda: ops.crnn_ctc_loss_fwd(rot(logits), tg, tl, il, 0, False, 1)),
        "CTC loss backward, hip": nograd(ctc_bwd),
        "CTC loss forward + backward, torch": ctc_torch,
    }
    rows.update(layer_rows)

    def region(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for f in rows.values():                                  # warm-up: code objects, the library's algorithm choices
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.regions):
        for k, f in rows.items():
            ms[k].append(region(f))
    table = []
    for k, v in ms.items():
        row = dict(stage=k, ms=statistics.median(v), ms_min=min(v), ms_max=max(v))
        table.append(row)
        print(f"{k:72s} {row['ms']:9.3f} ms / batch (min {row['ms_min']:.3f} max {row['ms_max']:.3f})", flush=True)
    med = {r["stage"]: r["ms"] for r in table}
    plan = ops.crnn_lstm_plan(N)
    result = dict(bench="crnn_train", batch=N, T=T, reps=a.reps, regions=a.regions, buffers=B, images_per_group=plan,
                  table=table,
                  step_hip_over_torch=med["decoder + loss, forward + backward, hip"] /
                  med["decoder + loss, forward + backward, torch"],
                  step_hip_bf16x3_over_torch=med["decoder + loss, forward + backward, hip bf16x3"] /
                  med["decoder + loss, forward + backward, torch"],
                  recurrence_bwd_over_fwd=med["lstm0 recurrence backward"] / med["lstm0 recurrence forward (inference kernel)"],
                  ctc_hip_over_torch=(med["CTC loss forward, hip"] + med["CTC loss backward, hip"]) /
                  med["CTC loss forward + backward, torch"])
    print(f"planner: {plan} images per workgroup; decoder + loss step hip / torch {result['step_hip_over_torch']:.2f}, "
          f"hip bf16x3 / torch {result['step_hip_bf16x3_over_torch']:.2f}; "
          f"recurrence backward / forward {result['recurrence_bwd_over_fwd']:.2f}; CTC loss hip / torch "
          f"{result['ctc_hip_over_torch']:.2f}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


def _no_grad(torch, f):
    with torch.no_grad():
        return f()


if __name__ == "__main__":
    main()
