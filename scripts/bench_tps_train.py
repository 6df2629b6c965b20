"""Training the classic rectifier: `TPSPreprocessor` forward + backward at a batch of 1x32x100 and 3x32x100 images with the
localisation network on the "hip" train backend (tpspp_bn_pool_train.hip and the convolution / BatchNorm / GEMM training
kernels) against "torch" (PyTorch's layers) on the same GPU; the warp is on the HIP kernels under both.  No ratio here is a
pass bar; the default backend stays "torch".

Rows: the module step under each backend and each channel count; per pooled layer (z = 64x32x100, 128x16x50, 256x8x25 per
image) the fused forward (`bn_pool2x2_fwd`) next to `bn_apply` + `maxpool2x2`, and the fused backward
(`bn_pool2x2_bwd_reduce` + `_bwd_data`) next to PyTorch's max-pool backward + `bn_bwd_reduce` + `bn_bwd_data`.  GB/s from
bytes counted from the shapes, Z = the bytes of z:
    fused forward    1.25 Z  (read z, write p)
    unfused forward  3.25 Z  (bn_apply: read z, write y; maxpool2x2: read y, write p)
    fused backward   3.5 Z   (reduce: read z, dp; data: read z, dp, write dz)
    unfused backward 8.75 Z  (pool backward: read dp and int64 indices, write dy; reduce: read dy, y, z; data: read dy, y, z,
                              write dz)
and `torch.cuda.max_memory_allocated` of one module step under each backend.

Every row: `reps` calls between two device events per region, the variants interleaved region by region, inputs rotated
over `--buffers` copies so that no call finds its own input in cache, medians over the regions with min and max
(scripts/bench_crnn_train.py's method).

    python scripts/bench_tps_train.py [--batch 512] [--reps 5] [--regions 7] [--buffers 2] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS = ((64, 32, 100), (128, 16, 50), (256, 8, 25))
BYTES_IN_Z = {"fused forward": 1.25, "unfused forward": 3.25, "fused backward": 3.5, "unfused backward": 8.75}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from tps_pp_amd import TPSPreprocessor, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_tps_train: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    N, B = a.batch, a.buffers
    torch.manual_seed(0)
    it = {"i": 0}

    def rot(lst):
        it["i"] += 1
        return lst[it["i"] % B]

    rows, gbytes = {}, {}
    # ---- the module under each backend ----------------------------------------------------------------------------------
    mods, imgs = {}, {}
    for ch in (1, 3):
        imgs[ch] = [torch.rand((N, ch, 32, 100), device=dev) for _ in range(B)]
        for mode in ("hip", "torch"):
            m = TPSPreprocessor(20, (32, 100), (32, 100), ch).to(dev).train().set_train_backend(mode)
            with torch.no_grad():          # the constructor's zero fc2 weight would make every gradient below it zero
                m.LocalizationNetwork.localization_fc2.weight.normal_(0, 0.01)
            mods[ch, mode] = m

    def step(ch, mode):
        m = mods[ch, mode]
        for p in m.parameters():
            p.grad = None
        m(rot(imgs[ch])).square().mean().backward()

    for ch in (1, 3):
        for mode in ("hip", "torch"):
            rows[f"TPSPreprocessor forward + backward, {ch}x32x100, {mode}"] = (lambda ch=ch, mode=mode: step(ch, mode))

    # ---- the pooled layers on saved operands ------------------------------------------------------------------------------
    def add_layer(C, H, W):
        tag = f"{C}x{H}x{W}"
        zs = [torch.randn((N, C, H, W), device=dev) for _ in range(B)]
        dps = [torch.randn((N, C, H // 2, W // 2), device=dev) for _ in range(B)]
        gamma = 1 + 0.3 * torch.randn(C, device=dev)
        beta = 0.2 * torch.randn(C, device=dev)
        with torch.no_grad():
            stats = [ops.bn_train_stats(z) for z in zs]
            ys = [ops.bn_apply(z, st, gamma, beta, relu=True) for z, st in zip(zs, stats)]
            idx = [torch.nn.functional.max_pool2d(y, 2, 2, return_indices=True)[1] for y in ys]
        zb = zs[0].numel() * 4 / 1e9

        def fused_fwd():
            i = rot(range(B))
            return ops.bn_pool2x2_fwd(zs[i], stats[i], gamma, beta)

        def unfused_fwd():
            i = rot(range(B))
            return ops.maxpool2x2(ops.bn_apply(zs[i], stats[i], gamma, beta, relu=True))

        def fused_bwd():
            i = rot(range(B))
            sums = ops.bn_pool2x2_bwd_reduce(dps[i], zs[i], stats[i], gamma, beta)
            return ops.bn_pool2x2_bwd_data(dps[i], zs[i], stats[i], gamma, beta, sums, True)

        def unfused_bwd():
            i = rot(range(B))
            dy = torch.ops.aten.max_pool2d_with_indices_backward(dps[i], ys[i], [2, 2], [2, 2], [0, 0], [1, 1], False, idx[i])
            sums = ops.bn_bwd_reduce(dy, ys[i], zs[i], stats[i], relu=True)
            return ops.bn_bwd_data(dy, ys[i], zs[i], stats[i], gamma, sums, True, relu=True)[0]

        for kind, f in (("fused forward", fused_fwd), ("unfused forward", unfused_fwd), ("fused backward", fused_bwd),
                        ("unfused backward", unfused_bwd)):
            rows[f"{tag} {kind}"] = (lambda f=f: _no_grad(torch, f))
            gbytes[f"{tag} {kind}"] = BYTES_IN_Z[kind] * zb

    for layer in LAYERS:
        add_layer(*layer)

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
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.regions):
        for k, f in rows.items():
            ms[k].append(region(f))
    table = []
    for k, v in ms.items():
        row = dict(stage=k, ms=statistics.median(v), ms_min=min(v), ms_max=max(v))
        if k in gbytes:
            row.update(gbytes=gbytes[k], gb_per_s=gbytes[k] / (row["ms"] * 1e-3))
        table.append(row)
        extra = f"  {row['gbytes']:.3f} GB  {row['gb_per_s']:7.0f} GB/s" if k in gbytes else ""
        print(f"{k:60s} {row['ms']:9.3f} ms / batch (min {row['ms_min']:.3f} max {row['ms_max']:.3f}){extra}", flush=True)
    med = {r["stage"]: r["ms"] for r in table}

    # ---- peak memory of one module step ----------------------------------------------------------------------------------
    peak = {}
    for (ch, mode), m in mods.items():
        for p in m.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step(ch, mode)
        torch.cuda.synchronize()
        peak[f"{ch}x32x100 {mode}"] = (torch.cuda.max_memory_allocated(dev) - base) / 2**20
        for p in m.parameters():
            p.grad = None
    for k, v in peak.items():
        print(f"peak memory of one step above the resident set, {k}: {v:.0f} MiB", flush=True)

    result = dict(bench="tps_train", batch=N, reps=a.reps, regions=a.regions, buffers=B, table=table, peak_mib=peak,
                  step_hip_over_torch={f"{ch}x32x100": med[f"TPSPreprocessor forward + backward, {ch}x32x100, hip"] /
                                       med[f"TPSPreprocessor forward + backward, {ch}x32x100, torch"] for ch in (1, 3)},
                  fused_over_unfused={f"{C}x{H}x{W} {d}": med[f"{C}x{H}x{W} fused {d}"] / med[f"{C}x{H}x{W} unfused {d}"]
                                      for C, H, W in LAYERS for d in ("forward", "backward")})
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
