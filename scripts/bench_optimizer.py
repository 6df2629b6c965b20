"""The optimiser step on the full recogniser's parameter set (nrtr_tps++: 390 tensors, 35.6 M parameters), with gradients
from one real backward:

  * the HIP multi-tensor Adam `step()` alone and with gradient clipping (tps_pp_amd/optim.py),
  * the same step of torch.optim.Adam three ways: foreach=False, foreach=True, fused=True,

interleaved region by region, medians over the regions.  Per variant: GPU milliseconds per step (device events around a
run of steps, the host running ahead), host milliseconds per step (the host clock around the same run, ended by a
synchronise), kernel launches per step (torch.profiler, one step, a pass of its own) and the achieved bytes/s over the
28 B per parameter that one pass needs (p, g, m, v read, p, m, v written) as a fraction of the 8 TB/s HBM peak.
Then a sweep of the update kernel alone over chunk and workgroup sizes (direct launches, no host work in between).

    python scripts/bench_optimizer.py [--batch 8] [--reps 20] [--regions 7] [--no-sweep] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tps_pp_amd as P  # noqa: E402
from tps_pp_amd import _lib, optim  # noqa: E402

HBM_PEAK = 8.0e12
BYTES_PER_PARAM = 28


def gradients(dev, batch):
    """The full recogniser in train mode and the gradients of one forward_train + backward on synthetic images."""
    torch.manual_seed(0)
    m = P.build_detector(bench.NRTR_TPSPP_MODEL).to(dev).train()
    img = torch.randn((batch, 3, 32, 128), device=dev)
    metas = [dict(resize_shape=(32, 128, 3), text="tps" + "ab"[i % 2] * (1 + i % 5)) for i in range(batch)]
    out = m.train_step(dict(img=img, img_metas=metas), None)
    out["loss"].backward()
    named = [(n, p) for n, p in m.named_parameters() if p.grad is not None]
    return named, out["log_vars"]["loss"]


def clones(named):
    ps = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    for q, (_, p) in zip(ps, named):
        q.grad = p.grad.detach().clone()
    return ps


def region(step, reps):
    """(GPU ms per step, host ms per step) of `reps` consecutive steps."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3 / reps


def launches(step):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.name
                   and "Memset" not in e.name)
    except Exception as e:                                   # the profiler is optional: the count is then not measured
        print("launch count not measured:", repr(e))
        return None


def sweep(dev, ps, reps):
    """The update kernel alone: `reps` direct launches between two events, per (chunk, threads)."""
    rows = []
    n = sum(p.numel() for p in ps)
    for chunk in (1024, 2048, 4096, 8192, 16384, 32768):
        for threads in (128, 256, 512, 1024):
            if chunk < 4 * threads:
                continue
            opt = optim.Adam(ps, lr=1e-4, chunk=chunk, threads=threads)
            opt.step()
            L, stream = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream

            def kernel():
                _lib.check(L.tpspp_mt_adam(opt._table.data_ptr(), opt._scalars.data_ptr(), opt._n_tensors, opt._map.data_ptr(),
                                           opt._n_chunks, chunk, threads, 0.9, 0.999, 1e-8, 0, 0, stream), "tpspp_mt_adam")
            kernel()
            ms = statistics.median(region(kernel, reps)[0] for _ in range(5))
            rows.append(dict(chunk=chunk, threads=threads, workgroups=opt._n_chunks, kernel_ms=ms,
                             tb_per_s=n * BYTES_PER_PARAM / (ms * 1e-3) / 1e12))
            print(f"sweep chunk {chunk:6d} threads {threads:5d} workgroups {opt._n_chunks:6d}  {ms * 1e3:8.1f} us  "
                  f"{rows[-1]['tb_per_s']:.2f} TB/s", flush=True)
            del opt
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    named, loss = gradients(dev, a.batch)
    n = sum(p.numel() for _, p in named)
    small = sum(1 for _, p in named if p.numel() <= 1024)
    odd = sum(1 for _, p in named if p.numel() % 4)
    print(f"{len(named)} tensors, {n / 1e6:.2f} M parameters, {small} of at most 1024 elements, {odd} with a length that is "
          f"no multiple of 4; loss {loss:.4f}; {n * BYTES_PER_PARAM / 1e9:.3f} GB per step, floor "
          f"{n * BYTES_PER_PARAM / HBM_PEAK * 1e6:.0f} us at {HBM_PEAK / 1e12:.0f} TB/s", flush=True)
    variants = {
        "hip Adam": lambda ps: optim.Adam(ps, lr=1e-4),
        "hip Adam + clip": lambda ps: optim.Adam(ps, lr=1e-4, grad_clip=dict(max_norm=1.0)),
        "torch foreach=False": lambda ps: torch.optim.Adam(ps, lr=1e-4, foreach=False),
        "torch foreach=True": lambda ps: torch.optim.Adam(ps, lr=1e-4, foreach=True),
        "torch fused=True": lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True),
    }
    opts = {k: make(clones(named)) for k, make in variants.items()}
    for o in opts.values():                                   # warm-up: state, tables, code objects
        for _ in range(3):
            o.step()
    gpu, host = {k: [] for k in opts}, {k: [] for k in opts}
    for _ in range(a.regions):
        for k, o in opts.items():
            g, h = region(o.step, a.reps)
            gpu[k].append(g)
            host[k].append(h)
    table = []
    for k, o in opts.items():
        g, h = statistics.median(gpu[k]), statistics.median(host[k])
        row = dict(variant=k, gpu_ms=g, gpu_ms_min=min(gpu[k]), gpu_ms_max=max(gpu[k]), host_ms=h, launches=launches(o.step),
                   tb_per_s=n * BYTES_PER_PARAM / (g * 1e-3) / 1e12)
        row["of_hbm_peak"] = row["tb_per_s"] * 1e12 / HBM_PEAK
        table.append(row)
        print(f"{k:22s} gpu {g:8.3f} ms (min {row['gpu_ms_min']:.3f} max {row['gpu_ms_max']:.3f})  host {h:8.3f} ms  "
              f"launches {row['launches']}  {row['tb_per_s']:.2f} TB/s = {100 * row['of_hbm_peak']:.1f} % of peak", flush=True)
    result = dict(tensors=len(named), parameters=n, regions=a.regions, reps=a.reps, table=table)
    if not a.no_sweep:
        del opts
        torch.cuda.empty_cache()
        result["sweep"] = sweep(dev, clones(named), a.reps)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(bench="optimizer", table=table)))


if __name__ == "__main__":
    main()
