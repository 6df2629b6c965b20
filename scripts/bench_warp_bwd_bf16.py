"""The warp backward with bf16 images and gradients (TPSPP_IO_BF16 of tpspp_warp_bwd) against the fp32 kernels, in ONE process,
at batch 512: the TPS++ geometry (feat_grid 64x32x128 + x 64x16x64 -> 16x64, F = 32, with the score) and the classic
rectifier's 3x32x100 (F = 20, the one-launch form).

Three variants, interleaved region by region so that clocks, neighbours on the machine and the allocator's state are shared:
  fp32   tpspp_warp_bwd on fp32 tensors (the kernels a graph ran before the bit existed);
  bf16   the same call with the bit on the same values held in bf16;
  cast   what a caller with bf16 tensors did before: images and output gradients cast to fp32, the fp32 backward, the
         input gradients cast back to bf16.
Every variant is the default accumulator (fp64 LDS atomics), as a training step runs it.  A region = `steps` calls of the C
entry point on pre-marshalled arguments and preallocated buffers (no allocation, no Python wrapper in the timed loop)
between device events, after `--warmup` untimed ones, on one stream; the classic geometry rotates buffer sets larger than
twice the 256 MB Infinity Cache (one set of the TPS++ geometry is 0.9 - 1.9 GB already).  The figure of a variant is the
MEDIAN region, with min and max.  Bytes: each variant's own algorithmic bytes per call, computed from the shapes (images,
output gradients and input gradients at its element size; grid, score, dL/d score and dL/d control points fp32; the cast
route also pays its six conversion passes).  Before timing, the bf16 result with the fixed-point accumulator is compared bit
for bit with the fp32 result rounded once.

    python scripts/bench_warp_bwd_bf16.py [--steps 300] [--warmup 20] [--regions 7] [--batch 512]

Prints one JSON line (stored as profiles/warp_bwd_bf16_bench_line.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tps_pp_amd import _lib, constants, ops                            # noqa: E402

HBM_PEAK_GBS = 8000.0
CACHE_BYTES = 256 << 20
BF, F32 = torch.bfloat16, torch.float32


class Geometry:
    def __init__(self, name, C0, in0_hw, C1, in1_hw, out_hw, point, classic, steps_scale):
        self.name, self.C0, self.in0_hw, self.C1, self.in1_hw, self.out_hw = name, C0, in0_hw, C1, in1_hw, out_hw
        self.point, self.classic, self.steps_scale = point, classic, steps_scale


GEOMETRIES = (
    Geometry("tpspp_64x32x128+64x16x64->16x64", 64, (32, 128), 64, (16, 64), (16, 64), (2, 16), False, 1),
    Geometry("classic_3x32x100", 3, (32, 100), 0, None, (32, 100), None, True, 10),
)


def measure(dev, geo, batch, steps, warmup, regions):
    lib = _lib.lib()
    Ho, Wo = geo.out_hw
    n = Ho * Wo
    if geo.classic:
        F = 20
        K = constants.classic(F, geo.out_hw)
        inv, P, xy = torch.from_numpy(K["inv_delta_C"]).to(dev), torch.from_numpy(K["P_hat"]).to(dev), None
        Pt = ops.transpose_p_hat(P)
        ident = torch.from_numpy(constants.classic_identity_ctrl(F)).to(dev)
    else:
        F = geo.point[0] * geo.point[1]
        K = constants.tpspp(geo.out_hw, geo.point)
        inv, P, xy = (torch.from_numpy(K[k]).to(dev) for k in ("hat_C", "P_hat", "P_xy"))
        Pt = ops.transpose_p_hat(P)
        ident = torch.from_numpy(constants.tpspp_initial_ctrl(geo.point)).to(dev)
    shapes = {"in0": (batch, geo.C0) + geo.in0_hw, "g0": (batch, geo.C0) + geo.out_hw}
    if geo.C1:
        shapes.update(in1=(batch, geo.C1) + geo.in1_hw, g1=(batch, geo.C1) + geo.out_hw)
    numel = {k: torch.Size(s).numel() for k, s in shapes.items()}
    set_elems = sum(numel.values()) + sum(v for k, v in numel.items() if k.startswith("in"))     # + the input gradients
    n_sets = {dt: max(1, -(-2 * CACHE_BYTES // (set_elems * sz))) for dt, sz in ((F32, 4), (BF, 2))}
    ws_floats = int(lib.tpspp_warp_bwd_workspace_floats(batch, Ho, Wo))

    def make_set(dt, j):
        gj = torch.Generator(device=dev).manual_seed(100 + j)
        t = {k: (torch.rand(s, generator=gj, device=dev) * 2 - 1).to(BF).to(dt) for k, s in shapes.items()}   # bf16-exact values
        t["ctrl"] = ident[None] + 0.05 * (torch.rand((batch, F, 2), generator=gj, device=dev) * 2 - 1)
        t["score"] = None if geo.classic else torch.tanh(torch.randn((batch, n, F), generator=gj, device=dev))
        t["grid"] = ops.warp(t["in0"].float(), t["ctrl"], inv, P, geo.out_hw, P_xy=xy, score=t["score"],
                             in1=t["in1"].float() if geo.C1 else None, want_grid=True)[2]
        t["T"] = ops.solve_T(inv, t["ctrl"]) if t["score"] is not None else None
        t["g_in0"] = torch.empty_like(t["in0"])
        t["g_in1"] = torch.empty_like(t["in1"]) if geo.C1 else None
        t["g_ctrl"] = torch.empty((batch, F, 2), device=dev)
        t["g_score"] = torch.empty_like(t["score"]) if t["score"] is not None else None
        t["ws"] = torch.empty((ws_floats,), device=dev)
        return t

    def args_of(t, flags):
        p = ops._ptr
        H1, W1 = geo.in1_hw if geo.C1 else (0, 0)
        return (p(t["g0"]), p(t["in0"]), geo.C0, geo.in0_hw[0], geo.in0_hw[1], p(t.get("g1")), p(t.get("in1")), geo.C1, H1, W1,
                p(t["grid"]), p(t["T"]), p(inv), p(P), P.shape[1], p(xy), p(t["score"]), p(Pt), flags, batch, F, Ho, Wo,
                p(t["g_in0"]), p(t["g_in1"]), p(t["g_ctrl"]), p(t["g_score"]), p(t["ws"]), ws_floats)

    sets_f = [make_set(F32, j) for j in range(n_sets[F32])]
    sets_b = [make_set(BF, j) for j in range(n_sets[BF])]
    torch.cuda.synchronize(dev)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    args_f = [args_of(t, 0) + (sp,) for t in sets_f]
    args_b = [args_of(t, ops.IO_BF16) + (sp,) for t in sets_b]
    bwd = lib.tpspp_warp_bwd

    # parity of what is timed (set 0 holds the same values in both dtypes): fixed point, bit for bit
    _lib.check(bwd(*(args_of(sets_f[0], ops.BWD_FIXED_POINT) + (sp,))), "tpspp_warp_bwd")
    _lib.check(bwd(*(args_of(sets_b[0], ops.BWD_FIXED_POINT | ops.IO_BF16) + (sp,))), "tpspp_warp_bwd")
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(sets_b[0]["g_in0"], sets_f[0]["g_in0"].bfloat16()) and
                torch.equal(sets_b[0]["g_ctrl"], sets_f[0]["g_ctrl"]))

    img_keys = [k for k in ("in0", "in1", "g0", "g1") if k in shapes]
    gin_keys = ["g_in0"] + (["g_in1"] if geo.C1 else [])

    def step_f(i):
        rc = bwd(*args_f[i % len(args_f)])
        assert rc == 0

    def step_b(i):
        rc = bwd(*args_b[i % len(args_b)])
        assert rc == 0

    def step_cast(i):                                                 # bf16 tensors through the fp32 kernel
        f, b = sets_f[i % len(sets_f)], sets_b[i % len(sets_b)]
        for k in img_keys:
            f[k].copy_(b[k])
        rc = bwd(*args_f[i % len(args_f)])
        assert rc == 0
        for k in gin_keys:
            b[k].copy_(f[k])

    nsteps = steps * geo.steps_scale

    def timed(step):
        for i in range(warmup):
            step(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record(stream)
        for i in range(nsteps):
            step(i)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / nsteps

    variants = (("fp32", step_f), ("bf16", step_b), ("cast", step_cast))
    samples = {name: [] for name, _ in variants}
    for _ in range(regions):                                          # interleaved: one region of every variant per round
        for name, step in variants:
            samples[name].append(timed(step))

    img = sum(numel.values())
    gin = sum(v for k, v in numel.items() if k.startswith("in"))
    fixed = batch * n * 2 * 4 + batch * F * 2 * 4 + (0 if geo.classic else 2 * batch * n * F * 4)     # grid, g_ctrl, score + g_score
    own = {"fp32": (img + gin) * 4 + fixed, "bf16": (img + gin) * 2 + fixed,
           "cast": (img + gin) * 4 + fixed + (img + gin) * (2 + 4)}   # + each conversion pass reads one size and writes the other
    rec = {"geometry": geo.name, "batch": batch, "steps_per_region": nsteps, "same_bits_as_fp32_rounded_once_fixed_point": same,
           "rotating_buffer_sets": {"fp32": len(sets_f), "bf16": len(sets_b)}}
    for name, _ in variants:
        s = samples[name]
        med = statistics.median(s)
        rec[name] = {"call_us_median": round(med, 2), "call_us_min": round(min(s), 2), "call_us_max": round(max(s), 2),
                     "own_bytes_per_call": own[name],
                     "frac_of_hbm_peak_on_own_bytes": round(own[name] / (med * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    f, b, c = (statistics.median(samples[k]) for k in ("fp32", "bf16", "cast"))
    rec["bf16_over_fp32_median"] = round(b / f, 4)
    rec["bf16_over_cast_route_median"] = round(b / c, 4)
    rec["fp32_spread_us"] = round(max(samples["fp32"]) - min(samples["fp32"]), 2)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300, help="calls per region at the TPS++ geometry (x10 at the classic one)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    if a.regions < 5:
        ap.error("--regions: at least 5 (the figure is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp_bwd_bf16: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rec = {"metric": "warp_backward_bf16_vs_fp32_vs_cast_route", "device": torch.cuda.get_device_name(dev),
           "steps": a.steps, "warmup": a.warmup, "regions": a.regions, "accumulator": "default (fp64 LDS atomics)",
           "estimator": "median region of `steps_per_region` calls / steps_per_region, per variant; variants interleaved",
           "results": [measure(dev, geo, a.batch, a.steps, a.warmup, a.regions) for geo in GEOMETRIES]}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
