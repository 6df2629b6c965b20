"""Training step of the NRTR encoder on both train backends, in one process (needs an MI355X; fails without a GPU).

    python scripts/bench_encoder_train.py [--batch 512] [--hw 1 64] [--layers 6] [--reps 7] [--iters 5] [--out FILE]

Shape: the recogniser's own (6 layers, d_model 512, d_inner 256, 8 heads) on the 32 x 128 geometry with backbone strides
[2, 1, 2, 1, 2]: T = 64 tokens per image.  For dropout 0.1 and 0.0 it reports
  * ms per forward + backward of the whole encoder for "torch" and "hip": after a warm-up of each, `reps` timed regions of
    `iters` steps per backend, the two backends alternating region by region, device events around each region, median
    and min / max of the per-step times;
  * the attention kernels' own times at the same shape: device events around `iters` isolated calls of
    ops.attn_train_fwd (one kernel) and ops.attn_train_bwd (two kernels), median over `reps` regions, and what the six
    layers of a step spend in them.
One JSON line per dropout rate."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tps_pp_amd import NRTREncoder, ops  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def summary(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--hw", type=int, nargs=2, default=(1, 64))
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_encoder_train: no GPU (there is no CPU form of this measurement)")
    dev = torch.device("cuda:0")
    N, (H, W), C, heads = a.batch, a.hw, 512, 8
    T = H * W
    lines = []
    for p in (0.1, 0.0):
        torch.manual_seed(0)
        enc = NRTREncoder(n_layers=a.layers, d_model=C, d_inner=256, n_head=heads, dropout=p).to(dev).train()
        feat = torch.randn((N, C, H, W), device=dev, requires_grad=True)
        gout = torch.randn((N, T, C), device=dev)
        metas = [dict(valid_ratio=1.0 if i % 2 else 0.8) for i in range(N)]

        def step(mode):
            def run():
                enc.set_train_backend(mode)
                for q in enc.parameters():
                    q.grad = None
                feat.grad = None
                enc(feat, metas).backward(gout)
            return run

        steps = {m: step(m) for m in ("torch", "hip")}
        for m in steps:                      # warm-up: code objects, allocator, library algorithm choices
            timed(steps[m], 3)
        times = {m: [] for m in steps}
        for _ in range(a.reps):              # alternate the backends region by region
            for m in steps:
                times[m].append(timed(steps[m], a.iters))

        # the attention kernels by themselves, on one layer's fused projection
        qkv = torch.randn((N * T, 3 * C), device=dev)
        dqkv = torch.empty_like(qkv)
        dout = torch.randn((N * T, C), device=dev)
        vl = torch.tensor([T if i % 2 else int(0.8 * T) for i in range(N)], dtype=torch.int32, device=dev)
        out, lse = ops.attn_train_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, N, C, heads, T, T, vl, p, 1, 0)

        def fwd():
            ops.attn_train_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, N, C, heads, T, T, vl, p, 1, 0)

        def bwd():
            ops.attn_train_bwd(dout, qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, out, lse, N, C, heads, T, T, vl, p, 1, 0, dqkv,
                               dqkv[:, C:], dqkv[:, 2 * C:], 3 * C)

        timed(fwd, 3), timed(bwd, 3)
        kf = [timed(fwd, 4 * a.iters) for _ in range(a.reps)]
        kb = [timed(bwd, 4 * a.iters) for _ in range(a.reps)]
        rec = dict(what="nrtr_encoder_train_step", batch=N, tokens=T, layers=a.layers, d_model=C, d_inner=256, dropout=p,
                   reps=a.reps, iters=a.iters, torch=summary(times["torch"]), hip=summary(times["hip"]),
                   attn_train_fwd_call=summary(kf), attn_train_bwd_call=summary(kb),
                   attention_ms_per_step=round(a.layers * (statistics.median(kf) + statistics.median(kb)), 4),
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del enc, feat, gout, qkv, dqkv, dout
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
