"""The CRNN recogniser behind the classic rectifier, stage by stage, at a batch of 1 x 32 x 100 images (crnn_tps.py).

Rows: the rectifier; the VGG; each BiLSTM layer split into its input projection (tpspp_mm_f32) and its recurrence
(tpspp_crnn_lstm_fwd); the two embedding Linears; the CTC decode with its device->host copy; the whole `simple_test`.
Then, for each precision mode (fp32 = compute_dtype None, the control; "bf16x3"; torch.bfloat16): the VGG alone, each of its
seven convolutions (TFLOP/s) and four pools (GB/s) through the calls the VGG makes, and `simple_test` whole; and the
agreement of each reduced mode's decisions with the exact fp32 kernels on 256 images (printed, not a bar).
Then the decoder's own modes (`CRNNDecoder.set_compute_dtype`): the decoder whole in fp32 / bf16x3 / bf16, both input
projections (tpspp_mm_bf16) and both recurrences (tpspp_crnn_lstm_bf16_fwd) in the two reduced modes -- their fp32
counterparts are the rows above, in the same run --, and `simple_test` with VGG and decoder in the same mode.
Two comparison columns, neither of them a pass bar:
  * `torch.nn.LSTM` on the same GPU against projection + recurrence of the same layer (the library fuses the two, so the
    recurrence alone has no counterpart);
  * the mirror's PyTorch composition from the rectified image on (`_forward_torch` of the VGG and the decoder, the
    convertor's host path) against the HIP path over the same stages.

Every row: `reps` calls between two device events per region, the variants interleaved region by region, inputs rotated
over `--buffers` copies so that no call finds its own input in cache, medians over the regions with min and max.  The
decode and `simple_test` rows end in a host copy, so the host clock is what times them.

    python scripts/bench_crnn.py [--batch 512] [--reps 20] [--regions 7] [--buffers 4] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from tps_pp_amd import build_detector, ops, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_crnn: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    N, B = a.batch, a.buffers
    torch.manual_seed(0)
    m = build_detector(dict(
        type="CRNNNet", preprocessor=dict(type="TPSPreprocessor", num_fiducial=20, img_size=(32, 100),
                                          rectified_img_size=(32, 100), num_img_channel=1),
        backbone=dict(type="VeryDeepVgg", leaky_relu=False, input_channels=1), encoder=None,
        decoder=dict(type="CRNNDecoder", in_channels=512, rnn_flag=True), loss=dict(type="CTCLoss"),
        label_convertor=dict(type="CTCConvertor", dict_type="DICT36", with_unknown=False, lower=True))).eval().to(dev)
    conv, dec = m.label_convertor, m.decoder
    l0, l1 = dec.decoder[0], dec.decoder[1]
    H = ops.CRNN_HIDDEN
    imgs = [torch.from_numpy(synth.smooth_image((N, 1, 32, 100), f"bench.crnn{i}")).to(dev) for i in range(B)]
    metas = [dict(resize_shape=(32, 100, 1)) for _ in range(N)]
    with torch.no_grad():
        rects = [m.preprocessor(x) for x in imgs]
        feats = [m.backbone(x) for x in rects]
        T = feats[0].shape[3]
        w0, w1 = l0._hip_weights(), l1._hip_weights()
        sn, sc, _, sw = feats[0].stride()
        xg0 = [ops.linear_fwd(f, (T, N, sw, sn, sc), w0[0], w0[1]).view(T, N, 2, 4 * H) for f in feats]
        rec0 = [ops.crnn_lstm(x, w0[2]) for x in xg0]
        e0 = [ops.linear_fwd(r, ops._dense(T * N, 2 * H), l0.embedding.weight.detach(), l0.embedding.bias.detach()) for r in rec0]
        xg1 = [ops.linear_fwd(e, (T, N, N * H, H, 1), w1[0], w1[1]).view(T, N, 2, 4 * H) for e in e0]
        rec1 = [ops.crnn_lstm(x, w1[2]) for x in xg1]
        logits = [dec(f, None, None, None, train_mode=False) for f in feats]
        seq0 = [f[:, :, 0, :].permute(2, 0, 1).contiguous() for f in feats]          # (T, N, 512): nn.LSTM's input
        seq1 = [e.view(T, N, H) for e in e0]
    plan = ops.crnn_lstm_plan(N)
    it = {"i": 0}

    def rot(lst):
        it["i"] += 1
        return lst[it["i"] % B]

    def emb(layer, rec):
        return ops.linear_fwd(rec, ops._dense(T * N, 2 * H), layer.embedding.weight.detach(), layer.embedding.bias.detach())

    def torch_tail(rect):
        lg = dec._forward_torch(m.backbone._forward_torch(rect))
        return conv.tensor2idx(lg.cpu(), metas)

    def hip_tail(rect):
        return conv.tensor2str(dec(m.backbone(rect), None, None, None, train_mode=False), metas)

    # ---- the precision modes: the VGG alone, each of its layers and pools, simple_test whole ------------
    MODES = (("fp32", None), ("bf16x3", "bf16x3"), ("bf16", torch.bfloat16))
    POOLS = {0: (2, 2, 0), 1: (2, 2, 0), 3: ((2, 2), (2, 1), (0, 1)), 5: ((2, 2), (2, 1), (0, 1))}
    vgg = m.backbone
    work = {}                                               # row name -> (FLOP, bytes moved) per call

    def in_mode(mode, f, whole=False):
        """f() with the VGG (whole: the model, through its public switch) in `mode`; the default mode afterwards."""
        def call():
            if whole:
                m.set_compute_dtype(mode)
            else:
                vgg.compute_dtype = mode
            try:
                return f()
            finally:
                m.set_compute_dtype(None)
        return call

    def numel(t):
        return t.t.numel() if isinstance(t, ops.Blocked) else t.numel()

    def nbytes(t):
        return numel(t) * (t.t if isinstance(t, ops.Blocked) else t).element_size()

    def layer_ops(mode):
        """[(name, fn(x), is_conv)] of the VGG's eleven steps in `mode`, the calls `VeryDeepVgg.forward` makes."""
        steps = []
        if mode is None:
            cw = vgg._hip_weights()
            for i in range(7):
                steps.append((f"conv{i}", (lambda x, i=i: ops.conv2d([x], cw[i], (2, 1) if i == 6 else 1, True)), True))
                if i in POOLS:
                    steps.append((f"pool{len([s for s in steps if not s[2]])}", (lambda x, i=i: ops.crnn_maxpool(x, *POOLS[i])), False))
            return steps
        x3 = mode == "bf16x3"
        cw, dt = vgg._hip_weights_bf16(x3), torch.float32 if x3 else torch.bfloat16
        for i in range(6):
            steps.append((f"conv{i}", (lambda x, i=i: ops.conv2d_bf16([x], cw[i], 1, True, out_dtype=dt, out_blocked=True)), True))
            if i in POOLS:
                steps.append((f"pool{len([s for s in steps if not s[2]])}", (lambda x, i=i: ops.crnn_maxpool_blocked(x, *POOLS[i])), False))
        steps.append(("conv6", lambda x: ops.conv2d_bf16([x], cw[6], (2, 1), True, out_dtype=torch.float32), True))
        return steps

    mode_rows = {}
    with torch.no_grad():
        for label, mode in MODES:
            mode_rows[f"VGG, {label}"] = (in_mode(mode, lambda: vgg(rot(rects))), False)
            steps = layer_ops(mode)
            ins = [[r] for r in rects]                      # per buffer: the inputs of the eleven steps
            for name, fn, is_conv in steps:
                for b in range(B):
                    ins[b].append(fn(ins[b][-1]))
            for k, (name, fn, is_conv) in enumerate(steps):
                xin, out = ins[0][k], ins[0][k + 1]
                key = f"  {name}, {label}"
                if is_conv:
                    cin, (n_, cout, ho, wo) = xin.shape[1], out.shape
                    taps, wo = (4, wo - 1) if name == "conv6" else (9, wo)       # conv6 is the 2x2 valid convolution
                    work[key] = (2.0 * n_ * cout * ho * wo * cin * taps, 0)
                else:
                    work[key] = (0, nbytes(xin) + nbytes(out))
                mode_rows[key] = ((lambda fn=fn, k=k, ins=ins: fn(rot(ins)[k])), False)
            mode_rows[f"simple_test (whole model), {label}"] = (in_mode(mode, lambda: m.simple_test(rot(imgs), metas), True), True)
        # decisions of the reduced modes against the exact fp32 kernels on 256 images (random-init weights, synthetic images)
        agreement = {}
        k256 = min(256, N)
        x256, metas256 = imgs[0][:k256], metas[:k256]

        def decide():
            lg = dec(vgg(m.preprocessor(x256)), None, None, None, train_mode=False)
            return lg.argmax(2).cpu(), conv.tensor2str(lg, metas256)[0]
        am0, str0 = decide()
        for label, mode in MODES[1:]:
            am, strs = in_mode(mode, decide, True)()
            agreement[label] = dict(images=k256, greedy_string_agreement=sum(a == b for a, b in zip(strs, str0)) / k256,
                                    per_position_argmax_agreement=float((am == am0).float().mean()))

    rows = {
        "rectifier (TPSPreprocessor)": (lambda: m.preprocessor(rot(imgs)), False),
        "VGG (VeryDeepVgg)": (lambda: m.backbone(rot(rects)), False),
        "lstm0 input projection 512 -> 2x1024": (lambda: ops.linear_fwd(rot(feats), (T, N, sw, sn, sc), w0[0], w0[1]), False),
        "lstm0 recurrence": (lambda: ops.crnn_lstm(rot(xg0), w0[2]), False),
        "lstm0 recurrence, 4 images per workgroup": (lambda: ops.crnn_lstm(rot(xg0), w0[2], 4), False),
        "lstm0 recurrence, 8 images per workgroup": (lambda: ops.crnn_lstm(rot(xg0), w0[2], 8), False),
        "lstm0 recurrence, 16 images per workgroup": (lambda: ops.crnn_lstm(rot(xg0), w0[2], 16), False),
        "lstm0 torch.nn.LSTM (projection + recurrence)": (lambda: l0.rnn(rot(seq0)), False),
        "lstm0 embedding 512 -> 256": (lambda: emb(l0, rot(rec0)), False),
        "lstm1 input projection 256 -> 2x1024": (lambda: ops.linear_fwd(rot(e0), (T, N, N * H, H, 1), w1[0], w1[1]), False),
        "lstm1 recurrence": (lambda: ops.crnn_lstm(rot(xg1), w1[2]), False),
        "lstm1 torch.nn.LSTM (projection + recurrence)": (lambda: l1.rnn(rot(seq1)), False),
        "lstm1 embedding 512 -> 37": (lambda: emb(l1, rot(rec1)), False),
        "CTC decode + host copy (tensor2str)": (lambda: conv.tensor2str(rot(logits), metas), True),
        "VGG + decoder + decode, HIP": (lambda: hip_tail(rot(rects)), True),
        "VGG + decoder + decode, PyTorch composition": (lambda: torch_tail(rot(rects)), True),
        "simple_test (whole model)": (lambda: m.simple_test(rot(imgs), metas), True),
    }
    rows.update(mode_rows)

    # ---- the decoder's precision modes: both projections, both recurrences, the decoder whole, and
    # simple_test with VGG and decoder in the same mode; the fp32 rows above are their control in the same run --------------
    def with_decoder(mode, f, whole=False):
        """f() with the decoder (whole: VGG and decoder, through the model's public switch) in `mode`; defaults afterwards."""
        def call():
            if whole:
                m.set_compute_dtype(mode, decoder=mode)
            else:
                dec.set_compute_dtype(mode)
            try:
                return f()
            finally:
                m.set_compute_dtype(None, decoder=None)
        return call

    for label, mode in MODES:
        rows[f"decoder (whole), {label}"] = (with_decoder(mode, lambda: dec(rot(feats), None, None, None, train_mode=False)), False)
        if mode is None:
            continue
        b0, b1 = l0._hip_weights_bf16(mode == "bf16x3"), l1._hip_weights_bf16(mode == "bf16x3")
        rows[f"lstm0 input projection 512 -> 2x1024, {label}"] = (
            lambda b0=b0: ops.linear_bf16_fwd(rot(feats), (T, N, sw, sn, sc), b0[0]), False)
        rows[f"lstm0 recurrence, {label}"] = (lambda b0=b0: ops.crnn_lstm_bf16(rot(xg0), b0[1]), False)
        rows[f"lstm0 recurrence, {label}, 16 images per workgroup"] = (lambda b0=b0: ops.crnn_lstm_bf16(rot(xg0), b0[1], 16), False)
        rows[f"lstm1 input projection 256 -> 2x1024, {label}"] = (
            lambda b1=b1: ops.linear_bf16_fwd(rot(e0), (T, N, N * H, H, 1), b1[0]), False)
        rows[f"lstm1 recurrence, {label}"] = (lambda b1=b1: ops.crnn_lstm_bf16(rot(xg1), b1[1]), False)
        rows[f"simple_test (whole model), VGG and decoder {label}"] = (
            with_decoder(mode, lambda: m.simple_test(rot(imgs), metas), True), True)

    def region(f, host):
        e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0_.record()
        for _ in range(a.reps):
            f()
        e1_.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3 / a.reps if host else e0_.elapsed_time(e1_) / a.reps

    with torch.no_grad():
        for f, _ in rows.values():                          # warm-up: code objects, the library's algorithm choices
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in rows}
        for _ in range(a.regions):
            for k, (f, host) in rows.items():
                ms[k].append(region(f, host))
    table = []
    for k, v in ms.items():
        row = dict(stage=k, ms=statistics.median(v), ms_min=min(v), ms_max=max(v), clock="host" if rows[k][1] else "device")
        rate = ""
        if k in work:                                       # a layer of the VGG: its arithmetic or its traffic
            flop, moved = work[k]
            if flop:
                row["tflops"] = flop / (row["ms"] * 1e-3) / 1e12
                rate = f", {row['tflops']:.1f} TFLOP/s"
            else:
                row["gb_per_s"] = moved / (row["ms"] * 1e-3) / 1e9
                rate = f", {row['gb_per_s']:.0f} GB/s"
        table.append(row)
        print(f"{k:50s} {row['ms']:9.3f} ms / batch (min {row['ms_min']:.3f} max {row['ms_max']:.3f}, {row['clock']} clock{rate})",
              flush=True)
    med = {r["stage"]: r["ms"] for r in table}
    result = dict(bench="crnn", batch=N, T=int(T), reps=a.reps, regions=a.regions, buffers=B, images_per_group=plan,
                  workgroups=2 * -(-N // plan), table=table,
                  lstm0_hip_over_torch=(med["lstm0 input projection 512 -> 2x1024"] + med["lstm0 recurrence"]) /
                  med["lstm0 torch.nn.LSTM (projection + recurrence)"],
                  lstm1_hip_over_torch=(med["lstm1 input projection 256 -> 2x1024"] + med["lstm1 recurrence"]) /
                  med["lstm1 torch.nn.LSTM (projection + recurrence)"],
                  tail_hip_over_torch=med["VGG + decoder + decode, HIP"] / med["VGG + decoder + decode, PyTorch composition"],
                  images_per_s=N / med["simple_test (whole model)"] * 1e3,
                  images_per_s_by_mode={label: N / med[f"simple_test (whole model), {label}"] * 1e3 for label, _ in MODES},
                  decoder_ms_by_mode={label: med[f"decoder (whole), {label}"] for label, _ in MODES},
                  images_per_s_by_mode_with_decoder={
                      label: N / med[f"simple_test (whole model), VGG and decoder {label}"] * 1e3 for label, _ in MODES[1:]},
                  agreement_with_fp32_kernels=agreement)
    for label, ag in agreement.items():
        print(f"{label} against the exact fp32 kernels, {ag['images']} images (random-init weights): greedy strings equal "
              f"{ag['greedy_string_agreement']:.4f}, per-position arg-max equal {ag['per_position_argmax_agreement']:.4f}", flush=True)
    print(f"planner: {plan} images per workgroup, {result['workgroups']} workgroups; HIP / torch: lstm0 "
          f"{result['lstm0_hip_over_torch']:.2f}, lstm1 {result['lstm1_hip_over_torch']:.2f}, VGG + decoder + decode "
          f"{result['tail_hip_over_torch']:.2f}; simple_test {result['images_per_s']:.0f} images / s", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
