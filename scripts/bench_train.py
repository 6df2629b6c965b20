"""Training of TPS_PP's control-point regressor on the HIP kernels at batch 512, fp32; one JSON line.

(a) every ConvModule of the ResNet45v2 wiring: HIP backward (data gradient + weight / bias gradient) against
    torch.ops.aten.convolution_backward on the same tensors -- the library is handed the logical (concatenated,
    upsampled) input and the masked dZ ready-made, the HIP kernels build both on the fly -- in ms and TFLOP/s from the
    shapes (backward = 2 x the forward's 2*N*Ho*Wo*Cout*Cin*K*K);
(b) the regressor's other blocks -- DGAB, the score (feat_linear, p_linear, product, tanh), CBAM and the localization
    FCs -- forward and forward + backward on the HIP kernels of set_train_backend("hip_all") (tpspp_regressor_bwd.hip)
    against the PyTorch composition of the same module on the same tensors, in ms;
(c) a whole TPS_PP training step (forward + backward, no optimiser) with set_train_backend("torch"), "hip" and
    "hip_all": alternating timed regions, the median of each, in images/s.

    python scripts/bench_train.py [--batch 512] [--reps 20] [--regions 7] [--steps 3] [--skip-conv]
--skip-conv leaves (a) out (the line then carries the blocks and the step only: profiles/train_regressor_line.json).
Kernel times: `rocprofv3 --kernel-trace --stats -- python3 scripts/bench_train.py --reps 3 --regions 1` (own run).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tps_pp_amd import TPS_PP, ops  # noqa: E402

# (name, sources [(C, H, W, uh, uw)], Cout, K, stride) -- the 14 ConvModules of TPS_PP() (ResNet45v2 wiring)
LAYERS = [
    ("down0", [(32, 32, 128, 1, 1)], 64, 1, (1, 1)),
    ("down1", [(32, 32, 128, 1, 1)], 64, 1, (1, 1)),
    ("down2", [(64, 16, 64, 1, 1)], 64, 1, (1, 1)),
    ("down0_1", [(64, 32, 128, 1, 1)], 64, 3, (2, 2)),
    ("down1_1", [(64, 32, 128, 1, 1)], 64, 3, (2, 2)),
    ("down_feat", [(64, 32, 128, 1, 1), (64, 32, 128, 1, 1), (64, 16, 64, 2, 2)], 64, 1, (1, 1)),
    ("k_encoder.0", [(64, 16, 64, 1, 1)] * 3, 64, 3, (1, 1)),
    ("k_encoder.1", [(64, 16, 64, 1, 1)], 64, 3, (2, 2)),
    ("k_encoder.2", [(64, 8, 32, 1, 1)], 64, 3, (2, 2)),
    ("k_encoder.3", [(64, 4, 16, 1, 1)], 64, 3, (2, 1)),
    ("k_decoder.0", [(64, 2, 16, 2, 1)], 64, 3, (1, 1)),
    ("k_decoder.1", [(64, 4, 16, 2, 2)], 64, 3, (1, 1)),
    ("k_decoder.2", [(64, 8, 32, 2, 2)], 64, 3, (1, 1)),
    ("k_decoder.3", [(64, 16, 64, 1, 1)], 64, 3, (1, 1)),
]


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_row(dev, name, spec, cout, k, stride, N, reps):
    g = torch.Generator(device=dev).manual_seed(1)
    srcs = [torch.randn((N, C, H, W), generator=g, device=dev) for C, H, W, _, _ in spec]
    entries = [(s, uh, uw) for s, (_, _, _, uh, uw) in zip(srcs, spec)]
    cin = sum(s[0] for s in spec)
    w = torch.randn((cout, cin, k, k), generator=g, device=dev) * (1.0 / (cin * k * k) ** 0.5)
    b = 0.1 * torch.randn((cout,), generator=g, device=dev)
    cw = ops.prep_conv_weight_device(w, b, [s[0] for s in spec])
    y = ops.conv2d(entries, cw, stride, relu=True)
    dy = torch.randn(tuple(y.shape), generator=g, device=dev)
    Ho, Wo = y.shape[2], y.shape[3]
    flops = 2.0 * N * Ho * Wo * cout * cin * k * k                  # one direction (= the forward's)

    t_fwd = timed(lambda: ops.conv2d(entries, cw, stride, relu=True), reps)
    t_data = timed(lambda: ops.conv2d_bwd_data(dy, w, entries, stride, y=y, relu=True), reps)
    t_wgt = timed(lambda: ops.conv2d_bwd_weight(entries, dy, k, stride, y=y, relu=True), reps)
    # the library on the same problem: logical input and dZ handed over ready-made
    X = torch.cat([s.repeat_interleave(uh, 2).repeat_interleave(uw, 3) for s, (_, _, _, uh, uw) in zip(srcs, spec)], 1)
    dz = dy * (y > 0)
    pad = ((k - 1) // 2, (k - 1) // 2)

    def lib():
        return torch.ops.aten.convolution_backward(dz, X, w, [cout], list(stride), list(pad), [1, 1], False, [0, 0], 1,
                                                   [True, True, True])
    t_lib = timed(lib, reps)
    t_hip = t_data + t_wgt
    return dict(layer=name, ms_hip=round(t_hip, 4), ms_hip_data=round(t_data, 4), ms_hip_weight=round(t_wgt, 4),
                ms_miopen=round(t_lib, 4), ms_fwd_hip=round(t_fwd, 4),
                tflops_hip=round(2 * flops / t_hip / 1e9, 2), tflops_miopen=round(2 * flops / t_lib / 1e9, 2),
                tflops_hip_data=round(flops / t_data / 1e9, 2), tflops_hip_weight=round(flops / t_wgt / 1e9, 2),
                tflops_fwd_hip=round(flops / t_fwd / 1e9, 2), gflop_bwd=round(2 * flops / 1e9, 2))


def step_rates(dev, N, regions, steps):
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.rand((N, 64, 16, 64), generator=g, device=dev)
    outs = [torch.rand((N, 32, 32, 128), generator=g, device=dev) for _ in range(2)]
    m = TPS_PP().to(dev).train()
    params = list(m.parameters())

    def step():
        for p in params:
            p.grad = None
        res = m(x, outs)
        (res["output"].square().mean() + res["mp_img"].square().mean()).backward()

    modes = ("torch", "hip", "hip_all")
    times = {k: [] for k in modes}
    for mode in modes:                      # warm-up of each (kernel selection, caches)
        m.set_train_backend(mode)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    for _ in range(regions):
        for mode in modes:
            m.set_train_backend(mode)
            step()
            times[mode].append(timed(step, steps, warm=0))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {k: round(N / (v / 1e3), 1) for k, v in med.items()}, {k: round(v, 3) for k, v in med.items()}


def block_rows(dev, N, reps):
    """Each block of the regressor's TPE / CBAM at batch N: the HIP autograd function of "hip_all" against the PyTorch
    composition of the same module (library kernels), forward alone and forward + backward (every input and parameter
    gradient) for the same incoming gradient."""
    torch.manual_seed(3)
    m = TPS_PP().to(dev).train()
    T = m.TPE
    with torch.no_grad():
        T.localization_fc2.weight.normal_(0, 0.02)
    g = torch.Generator(device=dev).manual_seed(4)
    de = torch.randn((N, 64, 16, 64), generator=g, device=dev).requires_grad_(True)
    en = torch.randn((N, 64, 2, 16), generator=g, device=dev).abs().requires_grad_(True)
    n = N
    blocks = [
        ("dgab", [de, en], list(T.atten[0].parameters()),
         lambda: ops.dgab_autograd(de, en.reshape(n, 64, -1), T.atten[0]),
         lambda: T.atten[0](de, en.reshape(n, 64, -1).transpose(1, 2))),
        ("score", [de, en], list(T.feat_linear.parameters()) + list(T.p_linear.parameters()),
         lambda: ops.score_autograd(de, en, T),
         lambda: T.get_score(en.reshape(n, 64, -1).transpose(1, 2), de).transpose(1, 2)),
        ("cbam", [en], list(m.MSFA.conv.atten.parameters()),
         lambda: ops.cbam_autograd(en, m.MSFA.conv.atten), lambda: m.MSFA.conv.atten(en)),
        ("localization", [en], list(T.localization_fc1.parameters()) + list(T.localization_fc2.parameters()),
         lambda: ops.tpe_points_autograd(en, T),
         lambda: T.localization_fc2(T.localization_fc1(en.reshape(n, 64, -1).transpose(1, 2)).reshape(n, -1)).view(
             n, T.num_fiducial, 2)),
    ]
    rows = []
    for name, ins, params, hip, lib in blocks:
        r = dict(block=name)
        for tag, fn in (("hip", hip), ("torch", lib)):
            out = fn()
            gout = torch.randn(out.shape, generator=g, device=dev)
            wrt = ins + params

            def fwd_bwd(fn=fn, gout=gout, wrt=wrt):
                torch.autograd.grad(fn(), wrt, gout)

            def fwd(fn=fn):
                with torch.no_grad():
                    fn()
            r[f"ms_fwd_{tag}"] = round(timed(fwd, reps), 4)
            r[f"ms_fwd_bwd_{tag}"] = round(timed(fwd_bwd, reps), 4)
        r["speedup_fwd_bwd"] = round(r["ms_fwd_bwd_torch"] / r["ms_fwd_bwd_hip"], 3)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-conv", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    blocks = block_rows(dev, a.batch, a.reps)
    ips, ms = step_rates(dev, a.batch, a.regions, a.steps)
    step = dict(images_per_s=ips, ms=ms, regions=a.regions, steps_per_region=a.steps)
    if a.skip_conv:
        print(json.dumps(dict(metric="tpspp_regressor_train", batch=a.batch, dtype="fp32", blocks=blocks,
                              train_step=step)))
        return
    rows = [layer_row(dev, *L, a.batch, a.reps) for L in LAYERS]
    gflop = sum(r["gflop_bwd"] for r in rows)
    t_hip = sum(r["ms_hip"] for r in rows)
    t_lib = sum(r["ms_miopen"] for r in rows)
    enc0 = next(r for r in rows if r["layer"] == "k_encoder.0")
    out = dict(metric="tpspp_conv_backward", batch=a.batch, dtype="fp32",
               aggregate=dict(gflop=round(gflop, 1), ms_hip=round(t_hip, 3), ms_miopen=round(t_lib, 3),
                              tflops_hip=round(gflop / t_hip, 2), tflops_miopen=round(gflop / t_lib, 2)),
               k_encoder0_data_vs_fwd=round(enc0["tflops_hip_data"] / enc0["tflops_fwd_hip"], 3),
               train_step=step, layers=rows, blocks=blocks)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
