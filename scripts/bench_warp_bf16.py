"""The classic rectifier with bf16 images in and out (TPSPP_IO_BF16 with the prepared table) against the fp32 kernels, in ONE
process: batch 512 of 3x32x100 (the headline geometry of bench.py) and of 3x64x256 (the largest staged image).

Three variants, interleaved region by region so that clocks, neighbours on the machine and the allocator's state are shared:
  fp32   the fp32 plan bench.py times (image-pair kernel at 32x100, span staging at 64x256);
  bf16   the bf16 plan on the same images rounded to bf16 (tps_warp_geo_bf16_kernel);
  cast   what a caller with bf16 tensors did before: cast to fp32, fp32 warp, cast the result to bf16 (three passes).
Both launch protocols of bench.py: every launch behind the previous one on one stream, and round-robin on two streams.
A region = `--steps` pre-marshalled launches (ops.WarpPlan) between device events after `--warmup` untimed ones, on rotating
buffer sets larger than twice the 256 MB Infinity Cache; the figure of a variant is the MEDIAN region, with min and max.
Fraction of the 8 TB/s peak: each dtype's own algorithmic bytes (image in + image out + control points) over its period.
Before timing, the bf16 result is compared bit for bit with the fp32 result rounded once.

    python scripts/bench_warp_bf16.py [--steps 1000] [--warmup 50] [--regions 7] [--batch 512]

Prints one JSON line (stored as profiles/warp_bf16_bench_line.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tps_pp_amd import constants, ops                                  # noqa: E402
from tps_pp_amd.tps_preprocessor import TPSPreprocessor                # noqa: E402

F, C = 20, 3
HBM_PEAK_GBS = 8000.0
CACHE_BYTES = 256 << 20
GEOMETRIES = ((32, 100), (64, 256))


def measure(dev, hw, batch, steps, warmup, regions):
    H, W = hw
    mod = TPSPreprocessor(num_fiducial=F, img_size=hw, rectified_img_size=hw, num_img_channel=C).eval().to(dev)
    gg = mod.GridGenerator
    p_hat_t, flags = gg.prepared_table()
    assert flags & ops.TABLE_PACKED and flags & ops.TABLE_MIRROR4
    elems = batch * C * H * W
    nbuf = {torch.float32: max(2, -(-2 * CACHE_BYTES // (2 * elems * 4))), torch.bfloat16: max(2, -(-2 * CACHE_BYTES // (2 * elems * 2)))}
    g = torch.Generator(device=dev).manual_seed(99)
    ident = torch.from_numpy(constants.classic_identity_ctrl(F)).to(dev)
    n_sets = max(nbuf.values())
    img_b = [(torch.rand((batch, C, H, W), generator=g, device=dev) * 2 - 1).to(torch.bfloat16) for _ in range(n_sets)]
    ctrls = [ident[None] + 0.05 * (torch.rand((batch, F, 2), generator=g, device=dev) * 2 - 1) for _ in range(n_sets)]
    img_f = [img_b[j].float() for j in range(nbuf[torch.float32])]      # the same values
    out_f = [torch.empty((batch, C, H, W), device=dev) for _ in range(nbuf[torch.float32])]
    out_b = [torch.empty((batch, C, H, W), device=dev, dtype=torch.bfloat16) for _ in range(n_sets)]
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(dev)]

    def plans_of(imgs, outs, n):
        return [ops.WarpPlan(imgs[j], ctrls[j], gg.inv_delta_C, gg.P_hat, hw, outs[j], P_hat_t=p_hat_t, table_flags=flags)
                for j in range(n)]
    plan_f = plans_of(img_f, out_f, nbuf[torch.float32])
    plan_b = plans_of(img_b, out_b, nbuf[torch.bfloat16])

    # parity of what is timed: same bits as the fp32 kernel rounded once
    plan_f[0].run()
    plan_b[0].run()
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(out_b[0], out_f[0].bfloat16()))

    def step_f(i, st):
        plan_f[i % len(plan_f)].run(st)

    def step_b(i, st):
        plan_b[i % len(plan_b)].run(st)

    def step_cast(i, st):                                             # bf16 tensors through the fp32 kernel: three passes
        j = i % len(plan_f)
        with torch.cuda.stream(st):
            img_f[j].copy_(img_b[j])
            plan_f[j].run(st)
            out_b[j].copy_(out_f[j])

    def timed(step, ns):
        for i in range(warmup):
            step(i, streams[i % ns])
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = [torch.cuda.Event(enable_timing=True) for _ in range(ns)]
        e0.record(streams[0])                                         # (created at their first record: in front of the region)
        for k in range(ns):
            e1[k].record(streams[k])
        torch.cuda.synchronize(dev)
        e0.record(streams[0])
        for st in streams[1:ns]:
            st.wait_event(e0)
        for i in range(steps):
            step(i, streams[i % ns])
        for k in range(ns):
            e1[k].record(streams[k])
        torch.cuda.synchronize(dev)
        return max(e0.elapsed_time(e) for e in e1) * 1e3 / steps

    variants = (("fp32", step_f), ("bf16", step_b), ("cast", step_cast))
    samples = {(name, ns): [] for name, _ in variants for ns in (1, 2)}
    for _ in range(regions):                                          # interleaved: one region of every variant per round
        for name, step in variants:
            for ns in (1, 2):
                samples[(name, ns)].append(timed(step, ns))

    item = {"fp32": 4, "bf16": 2, "cast": 2}
    rec = {"geometry": f"{C}x{H}x{W}", "batch": batch, "same_bits_as_fp32_rounded_once": same,
           "rotating_buffer_sets": {"fp32": len(plan_f), "bf16": len(plan_b)}}
    for name, _ in variants:
        bytes_launch = batch * (2 * C * H * W * item[name] + F * 2 * 4)
        for ns in (1, 2):
            s = samples[(name, ns)]
            med = statistics.median(s)
            rec[f"{name}_{ns}_stream{'s' if ns > 1 else ''}"] = {
                "launch_us_median": round(med, 3), "launch_us_min": round(min(s), 3), "launch_us_max": round(max(s), 3),
                "images_per_s": round(batch / (med * 1e-6)), "own_bytes_per_launch": bytes_launch,
                "frac_of_hbm_peak_on_own_bytes": round(bytes_launch / (med * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    # the condition of the comparison: the bf16 median period is no longer than the fp32 median of the same run, with the
    # fp32 kernel's own spread across its regions (max - min) as the margin; per launch protocol
    for ns in (1, 2):
        f, b = samples[("fp32", ns)], samples[("bf16", ns)]
        key = f"{ns}_stream{'s' if ns > 1 else ''}"
        rec[f"bf16_vs_fp32_{key}"] = {
            "bf16_over_fp32_median": round(statistics.median(b) / statistics.median(f), 4),
            "fp32_spread_us": round(max(f) - min(f), 3),
            "bf16_no_slower_within_fp32_spread": bool(statistics.median(b) <= statistics.median(f) + (max(f) - min(f))),
            "bf16_over_cast_route_median": round(statistics.median(b) / statistics.median(samples[("cast", ns)]), 4)}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    if a.regions < 5:
        ap.error("--regions: at least 5 (the figure is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp_bf16: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rec = {"metric": "classic_warp_bf16_vs_fp32", "device": torch.cuda.get_device_name(dev), "steps": a.steps,
           "warmup": a.warmup, "regions": a.regions,
           "estimator": "median region of `steps` launches / steps, per variant and launch protocol; variants interleaved",
           "results": [measure(dev, hw, a.batch, a.steps, a.warmup, a.regions) for hw in GEOMETRIES]}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
