"""Training the CRNN's VGG: `VeryDeepVgg` forward + backward at a batch of 1x32x100 images on the "hip" backend
(`set_vgg_train_backend("hip")`: the fp32 convolution forward / backward kernels, tpspp_crnn_maxpool_bwd, the BatchNorm
training kernels) against "torch" (PyTorch's layers) on the same GPU.  No ratio here is a pass bar; the default backend
stays "torch".

Rows:
  * the module step under each backend (the image carries a gradient, as behind a rectifier);
  * per pool (y = 64x32x100 and 128x16x50 at 2x2 / 2, 256x8x25 and 512x4x26 at (2,2) / (2,1) / (0,1) per image) the backward
    with the ReLU mask folded in (`crnn_maxpool_bwd`) next to PyTorch's `max_pool2d_with_indices_backward` +
    `threshold_backward` on stored int64 indices.  GB/s from bytes counted from the shapes, Y = the bytes of y, q = the
    pool's output elements over its input elements:
        crnn_maxpool_bwd   (2 + q) Y     (read y and dp, write dy)
        PyTorch            (4 + 3 q) Y   (pool backward: read dp and int64 indices, write dy; threshold: read dy and y, write)
  * conv0's two backward launches (`conv2d_bwd_weight`, `conv2d_bwd_data`) with relu = 1, which re-reads y for the mask in
    both, next to relu = 0, which is what they run with once the pool's backward has applied the mask;
and `torch.cuda.max_memory_allocated` of one module step under each backend.

Every row: `reps` calls between two device events per region, the variants interleaved region by region, inputs rotated
over `--buffers` copies so that no call finds its own input in cache, medians over the regions with min and max
(scripts/bench_tps_train.py's method).

    python scripts/bench_crnn_vgg_train.py [--batch 512] [--reps 5] [--regions 7] [--buffers 2] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P22 = ((2, 2), (2, 2), (0, 0))
RECT = ((2, 2), (2, 1), (0, 1))
POOLS = ((64, 32, 100, P22), (128, 16, 50, P22), (256, 8, 25, RECT), (512, 4, 26, RECT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from tps_pp_amd import ops
    from tps_pp_amd.crnn import VeryDeepVgg
    if not torch.cuda.is_available():
        raise SystemExit("bench_crnn_vgg_train: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    N, B = a.batch, a.buffers
    torch.manual_seed(0)
    it = {"i": 0}

    def rot(lst):
        it["i"] += 1
        return lst[it["i"] % B]

    rows, gbytes = {}, {}
    # ---- the module under each backend ----------------------------------------------------------------------------------
    imgs = [torch.rand((N, 1, 32, 100), device=dev) for _ in range(B)]
    mods = {mode: VeryDeepVgg(leaky_relu=False, input_channels=1).to(dev).train().set_vgg_train_backend(mode)
            for mode in ("hip", "torch")}
    mods["torch"].load_state_dict(mods["hip"].state_dict())

    def step(mode):
        m = mods[mode]
        for p in m.parameters():
            p.grad = None
        m(rot(imgs).detach().requires_grad_(True)).square().mean().backward()

    for mode in ("hip", "torch"):
        rows[f"VeryDeepVgg forward + backward, 1x32x100, {mode}"] = (lambda mode=mode: step(mode))

    # ---- the pool backwards on saved operands ---------------------------------------------------------------------------
    def add_pool(C, H, W, pool):
        k, s, p = pool
        tag = f"{C}x{H}x{W} k{k[0]}{k[1]} s{s[0]}{s[1]} p{p[0]}{p[1]}"
        ys = [torch.randn((N, C, H, W), device=dev).clamp_(min=0) for _ in range(B)]
        with torch.no_grad():
            pooled = [torch.nn.functional.max_pool2d(y, k, s, p, return_indices=True) for y in ys]
        idx = [i for _, i in pooled]
        dps = [torch.randn_like(o) for o, _ in pooled]
        yb = ys[0].numel() * 4 / 1e9
        q = dps[0].numel() / ys[0].numel()
        del pooled

        def ours():
            i = rot(range(B))
            return ops.crnn_maxpool_bwd(dps[i], ys[i], k, s, p, relu_mask=True)

        def theirs():
            i = rot(range(B))
            dy = torch.ops.aten.max_pool2d_with_indices_backward(dps[i], ys[i], list(k), list(s), list(p), [1, 1], False, idx[i])
            return torch.ops.aten.threshold_backward(dy, ys[i], 0)

        for kind, f, nbytes in (("crnn_maxpool_bwd (mask folded)", ours, (2 + q) * yb),
                                ("PyTorch pool backward + threshold_backward", theirs, (4 + 3 * q) * yb)):
            rows[f"{tag} {kind}"] = (lambda f=f: _no_grad(torch, f))
            gbytes[f"{tag} {kind}"] = nbytes

    for layer in POOLS:
        add_pool(*layer)

    # ---- conv0's two backward launches with and without the mask ---------------------------------------------------------
    w0 = torch.randn((64, 1, 3, 3), device=dev) / 3
    y0 = [torch.randn((N, 64, 32, 100), device=dev).clamp_(min=0) for _ in range(B)]
    d0 = [torch.randn((N, 64, 32, 100), device=dev) for _ in range(B)]

    def conv0_bwd(relu):
        i = rot(range(B))
        kw = dict(y=y0[i], relu=True) if relu else dict(relu=False)
        dw, db = ops.conv2d_bwd_weight([imgs[i]], d0[i], 3, (1, 1), **kw)
        return dw, db, ops.conv2d_bwd_data(d0[i], w0, [imgs[i]], (1, 1), **kw)[0]

    for relu in (1, 0):
        rows[f"conv0 bwd_weight + bwd_data, relu = {relu}"] = (lambda relu=relu: _no_grad(torch, lambda: conv0_bwd(relu)))

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
        print(f"{k:72s} {row['ms']:9.3f} ms / batch (min {row['ms_min']:.3f} max {row['ms_max']:.3f}){extra}", flush=True)
    med = {r["stage"]: r["ms"] for r in table}

    # ---- peak memory of one module step ----------------------------------------------------------------------------------
    peak = {}
    for mode, m in mods.items():
        for p in m.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step(mode)
        torch.cuda.synchronize()
        peak[mode] = (torch.cuda.max_memory_allocated(dev) - base) / 2**20
        for p in m.parameters():
            p.grad = None
    for k, v in peak.items():
        print(f"peak memory of one step above the resident set, {k}: {v:.0f} MiB", flush=True)

    pools = [k[:-len(" crnn_maxpool_bwd (mask folded)")] for k in med if k.endswith("crnn_maxpool_bwd (mask folded)")]
    result = dict(bench="crnn_vgg_train", batch=N, reps=a.reps, regions=a.regions, buffers=B, table=table, peak_mib=peak,
                  step_hip_over_torch=med["VeryDeepVgg forward + backward, 1x32x100, hip"] /
                  med["VeryDeepVgg forward + backward, 1x32x100, torch"],
                  pool_bwd_over_torch={t: med[f"{t} crnn_maxpool_bwd (mask folded)"] /
                                       med[f"{t} PyTorch pool backward + threshold_backward"] for t in pools},
                  conv0_bwd_relu0_over_relu1=med["conv0 bwd_weight + bwd_data, relu = 0"] /
                  med["conv0 bwd_weight + bwd_data, relu = 1"])
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
