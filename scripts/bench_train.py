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

    python scripts/bench_train.py --backbone [--batch 512] [--reps 20] [--regions 7] [--steps 3]
measures the recogniser's backbone (ResNetABI_v2_large, NRTR TPS++ wiring: strides [2, 1, 2, 1, 2], 3x32x128) instead
(profiles/train_backbone_line.json):
(a) the BatchNorm + shortcut + ReLU work of each distinct block shape (and the stem) on tpspp_bn_train.hip, forward and
    forward + backward, against PyTorch's composition of the same ops (batch_norm, add, ReLU) on the same tensors, in ms
    and as a fraction of the 8 TB/s HBM peak from the passes the HIP kernels make;
(b) the backbone's 50 convolution backwards (relu = 0) against torch.ops.aten.convolution_backward, in TFLOP/s;
(c) a whole backbone training step (forward + backward, no optimiser, tpsnet=None) with set_train_backend("torch") and
    "hip": alternating timed regions, the median of each, in images/s.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tps_pp_amd import TPS_PP, ResNetABI_v2_large, ops  # noqa: E402

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


# ---- --backbone -------------------------------------------------------------------------------------------------------
HBM_TBPS = 8.0
BACKBONE = dict(arch_settings=[3, 4, 6, 6, 3], strides=[2, 1, 2, 1, 2])


def backbone_convs():
    """(Cin, H, W, Cout, K, stride) -> count over the backbone's 50 convolutions (shapes from one forward on the CPU)."""
    m = ResNetABI_v2_large(**BACKBONE)
    seen = {}

    def hook(mod, inp, out):
        x = inp[0]
        key = (x.shape[1], x.shape[2], x.shape[3], mod.out_channels, mod.kernel_size[0], mod.stride[0])
        seen[key] = seen.get(key, 0) + 1

    hs = [c.register_forward_hook(hook) for c in m.modules() if isinstance(c, torch.nn.Conv2d)]
    with torch.no_grad():
        m._forward_torch(torch.zeros((1, 3, 32, 128)))
    for h in hs:
        h.remove()
    return seen


def bb_conv_row(dev, key, count, N, reps):
    cin, H, W, cout, k, st = key
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn((N, cin, H, W), generator=g, device=dev)
    w = torch.randn((cout, cin, k, k), generator=g, device=dev) * (1.0 / (cin * k * k) ** 0.5)
    cw = ops.prep_conv_weight_device(w)
    z = ops.conv2d([x], cw, st, relu=False)
    dz = torch.randn(tuple(z.shape), generator=g, device=dev)
    flops = 2.0 * N * z.shape[2] * z.shape[3] * cout * cin * k * k
    t_data = timed(lambda: ops.conv2d_bwd_data(dz, w, [x], st, relu=False), reps)
    t_wgt = timed(lambda: ops.conv2d_bwd_weight([x], dz, k, st, relu=False, want_bias=False), reps)
    pad = [(k - 1) // 2] * 2
    t_lib = timed(lambda: torch.ops.aten.convolution_backward(dz, x, w, None, [st, st], pad, [1, 1], False, [0, 0], 1,
                                                              [True, True, False]), reps)
    t_hip = t_data + t_wgt
    return dict(conv=f"{cin}->{cout} k{k} s{st} @{H}x{W}", count=count, ms_hip=round(t_hip, 4), ms_miopen=round(t_lib, 4),
                tflops_hip=round(2 * flops / t_hip / 1e9, 2), tflops_miopen=round(2 * flops / t_lib / 1e9, 2),
                gflop_bwd=round(2 * flops / 1e9, 2))


def bn_block_row(dev, name, N, C, H, W, kind, reps, hw1=None):
    """The BatchNorm work of one block shape: kind "stem" (relu(bn z)), "plain" (relu(bn1 z1), relu(bn2 z2 + x)) or "down"
    (relu(bn1 z1), relu(bn2 z2 + bn_d z_d)); HIP kernels vs F.batch_norm + add + ReLU, forward and forward + backward.
    hw1: the size of z1 when it differs (the first block of a stage with stride 2 normalises conv1's output before the
    stride)."""
    g = torch.Generator(device=dev).manual_seed(6)
    shape = (N, C, H, W)
    shape1 = (N, C) + tuple(hw1) if hw1 else shape
    bns = [torch.nn.BatchNorm2d(C).to(dev).train() for _ in range(3)]
    zs = [torch.randn(s, generator=g, device=dev) for s in (shape1, shape, shape)]   # z1 (stem: z), z2, z_d or x
    gs = [torch.randn(s, generator=g, device=dev) for s in (shape1, shape)]          # gradients reaching h and y
    stem, down = kind == "stem", kind == "down"

    def st(b, z):
        return ops.bn_train_stats(z, b.eps, b.momentum, b.running_mean, b.running_var, b.num_batches_tracked)

    def hip(backward):
        b1, b2, bd = bns
        s1 = st(b1, zs[0])
        h = ops.bn_apply(zs[0], s1, b1.weight, b1.bias)
        if stem:
            if backward:
                sm = ops.bn_bwd_reduce(gs[0], h, zs[0], s1)
                ops.bn_bwd_data(gs[0], h, zs[0], s1, b1.weight, sm, True)
            return
        s2 = st(b2, zs[1])
        if down:
            sd = st(bd, zs[2])
            y = ops.bn_apply(zs[1], s2, b2.weight, b2.bias, zb=zs[2], stats_b=sd, gamma_b=bd.weight, beta_b=bd.bias)
        else:
            y = ops.bn_apply(zs[1], s2, b2.weight, b2.bias, residual=zs[2])
        if not backward:
            return
        sm2 = ops.bn_bwd_reduce(gs[1], y, zs[1], s2, zs[2] if down else None, sd if down else None)
        ops.bn_bwd_data(gs[1], y, zs[1], s2, b2.weight, sm2, True, zb=zs[2] if down else None, stats_b=sd if down else None,
                        gamma_b=bd.weight if down else None)
        sm1 = ops.bn_bwd_reduce(gs[0], h, zs[0], s1)
        ops.bn_bwd_data(gs[0], h, zs[0], s1, b1.weight, sm1, True)
        if not down:                                     # the shortcut's gradient added to the block input's
            ops.bn_bwd_data(gs[1], y, relu=True, dres=dx, dres_mode=2, want_a=False, want_b=False)

    zr = [z.clone().requires_grad_(True) for z in zs]
    dx = torch.zeros(shape, device=dev)

    def lib(backward):
        F = torch.nn.functional
        b1, b2, bd = bns
        h = F.relu(b1(zr[0]))
        outs, grads, wrt = [h], [gs[0]], [zr[0]] + list(b1.parameters())
        if not stem:
            r = bd(zr[2]) if down else zr[2]
            outs.append(F.relu(b2(zr[1]) + r))
            grads.append(gs[1])
            wrt += [zr[1], zr[2]] + list(b2.parameters()) + (list(bd.parameters()) if down else [])
        if backward:
            torch.autograd.grad(outs, wrt, grads)

    e1, e = zs[0].numel(), zs[1].numel()
    # HBM passes of the HIP kernels over (N, C, H, W) tensors.  Forward: stats (1) + apply (2) of bn1; stats (1) + apply
    # (3: z2, the shortcut, y) of bn2, and bn_d's stats (1).  Backward: reduce (3) + data (4) of bn1; the same of bn2, with
    # z_d read twice and dz_d written (+3) or the identity shortcut's add into the input's gradient (4)
    bytes_f = 4 * (3 * e1 + (0 if stem else (5 if down else 4) * e))
    bytes_fb = bytes_f + 4 * (7 * e1 + (0 if stem else (10 if down else 11) * e))
    r = dict(block=name, shape=[N, C, H, W], kind=kind, shape_z1=list(shape1))
    for tag, fn in (("hip", hip), ("torch", lib)):
        r[f"ms_fwd_{tag}"] = round(timed(lambda: fn(False), reps), 4)
        r[f"ms_fwd_bwd_{tag}"] = round(timed(lambda: fn(True), reps), 4)
    r["gb_fwd_bwd_hip"] = round(bytes_fb / 1e9, 3)
    r["hbm_frac_fwd_hip"] = round(bytes_f / (r["ms_fwd_hip"] * 1e-3) / (HBM_TBPS * 1e12), 3)
    r["hbm_frac_fwd_bwd_hip"] = round(bytes_fb / (r["ms_fwd_bwd_hip"] * 1e-3) / (HBM_TBPS * 1e12), 3)
    r["speedup_fwd"] = round(r["ms_fwd_torch"] / r["ms_fwd_hip"], 3)
    r["speedup_fwd_bwd"] = round(r["ms_fwd_bwd_torch"] / r["ms_fwd_bwd_hip"], 3)
    return r


# (name, C, H, W, kind, size of z1 if it differs): the distinct block shapes of the NRTR TPS++ wiring at 3x32x128
BN_SHAPES = [("stem", 32, 32, 128, "stem", None), ("layer1.0", 32, 16, 64, "down", (32, 128)),
             ("layer1.1", 32, 16, 64, "plain", None), ("layer2.0", 64, 16, 64, "down", None),
             ("layer2.1", 64, 16, 64, "plain", None), ("layer3.0", 128, 8, 32, "down", (16, 64)),
             ("layer3.1", 128, 8, 32, "plain", None), ("layer4.0", 256, 8, 32, "down", None),
             ("layer4.1", 256, 8, 32, "plain", None), ("layer5.0", 512, 4, 16, "down", (8, 32)),
             ("layer5.1", 512, 4, 16, "plain", None)]


def backbone_step_rates(dev, N, regions, steps):
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn((N, 3, 32, 128), generator=g, device=dev)
    torch.manual_seed(8)
    m = ResNetABI_v2_large(**BACKBONE).to(dev).train()
    params = list(m.parameters())

    def step():
        for p in params:
            p.grad = None
        m(x)["output"].square().mean().backward()

    modes = ("torch", "hip")
    times = {k: [] for k in modes}
    for mode in modes:
        m.set_train_backend(mode)
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    for _ in range(regions):
        for mode in modes:
            m.set_train_backend(mode)
            step()
            times[mode].append(timed(step, steps, warm=0))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {k: round(N / (v / 1e3), 1) for k, v in med.items()}, {k: round(v, 3) for k, v in med.items()}


def main_backbone(a, dev):
    bn = [bn_block_row(dev, name, a.batch, C, H, W, kind, a.reps, hw1) for name, C, H, W, kind, hw1 in BN_SHAPES]
    convs = [bb_conv_row(dev, key, n, a.batch, a.reps) for key, n in backbone_convs().items()]
    gflop = sum(r["gflop_bwd"] * r["count"] for r in convs)
    t_hip = sum(r["ms_hip"] * r["count"] for r in convs)
    t_lib = sum(r["ms_miopen"] * r["count"] for r in convs)
    ips, ms = backbone_step_rates(dev, a.batch, a.regions, a.steps)
    print(json.dumps(dict(metric="backbone_train", batch=a.batch, dtype="fp32", input=[3, 32, 128],
                          bn_blocks=bn,
                          conv_backward=dict(count=sum(r["count"] for r in convs), gflop=round(gflop, 1),
                                             ms_hip=round(t_hip, 3), ms_miopen=round(t_lib, 3),
                                             tflops_hip=round(gflop / t_hip, 2), tflops_miopen=round(gflop / t_lib, 2),
                                             layers=convs),
                          train_step=dict(images_per_s=ips, ms=ms, regions=a.regions, steps_per_region=a.steps))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-conv", action="store_true")
    ap.add_argument("--backbone", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    if a.backbone:
        main_backbone(a, dev)
        return
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
