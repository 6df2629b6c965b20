#!/usr/bin/env python
"""bench.py -- rectified images/sec of the TPS hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): one step = one launch of the fused TPS grid-gen + bilinear
grid_sample HIP kernel on a batch of 512 synthetic 3x32x100 fp32 images, 20 fiducials, control
points = fiducial lattice + 0.05 * noise.  Inputs are resident in HBM before the timed region; the
steps rotate over enough distinct input/output buffers (> 256 MB) that the Infinity Cache cannot
hold the working set.  Weak scaling: every rank rectifies its own 512-image batches, there is no
data-path collective (images are independent).

A plain run does only what the headline needs: set-up, W warm-up steps, ONE timed region of exactly K steps round-robin
on `--streams` HIP streams (default 2 for K <= 200, else 3), then the JSON line (`value`, `ms_per_step` and the roofline
fraction of that region).  `--dump-outputs DIR` writes what the last timed step computed, the rectified batch a caller
of the path receives, as DIR/rectified.npy (float32, 19.7 MB); the inputs are the same from run to run.

`--full` adds everything else, as described below: both launch protocols over `--repeats` regions each, the parity
spot-check against the CPU oracle, the plain-copy ceiling, device clocks, `extra` and `cpu_baseline`.
With `--full`, two launch protocols are timed over exactly K steps each: all steps on ONE
stream (every launch waits for the previous one: kernel duration + launch gap, what a kernel trace shows), and the steps
round-robin on `--streams` HIP streams (default 2 for K <= 200, else 3 -- consecutive batches are independent, so a serving
loop has no reason to serialise their launches).  Each protocol's region is repeated (`--repeats`, default 5 for K <= 200: a
20-step region is 0.2 ms and at the mercy of the queues' wake-up after the synchronize) with barrier + synchronize before
each.  `value`, `ms_per_step` and `roofline.frac` come from the MEDIAN region of the protocol whose median is lower
(`config.streams` says which); the kernel-alone figure (`roofline.one_stream_frac`), the overlapped one
(`roofline.multi_stream_frac_median`), the fastest regions (`*_best`) and a plain device copy of the same bytes
(`roofline.plain_copy_frac`) are flat scalars of `roofline`.  Times are HIP events -- every stream records one before its first
and one after its last launch, a region is latest end - earliest start -- max over ranks; the host wall clock around the
region is reported as `wall_ms_per_step`.

`--gpus N` without a launcher (WORLD_SIZE unset) starts the N ranks itself (torch.distributed.run as a
child process; the parent never touches a GPU) and passes rank 0's JSON line through.  At N > 1 with `--full` the line
also carries `extra.recognizer_sharded`: the whole recogniser on 256 images per rank with the one collective
of the inference path, the RCCL all-gather of the decoder scores, inside the timed region
(tools/test.py:202-207).

Prints ONE JSON line on rank 0 with two extra objects (the second under `--full` only):
  roofline     -- algorithmic HBM bytes per launch / average launch duration (HIP events on the
                  launch stream over the timed region) against the 8 TB/s HBM peak;
  cpu_baseline -- the CPU oracle (a port of the reference's algorithm, OpenMP over images) timed on
                  this box's host cores on a bounded sample of the same workload (N = 1 only).
"""
import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from tps_pp_amd import TPSPreprocessor, constants, ops, synth  # noqa: E402

BATCH, C, H, W, F = 512, 3, 32, 100, 20
# SURVEY.md section 8d / DESIGN.md section 5: image in + control points + image out, per image
BYTES_PER_IMG = C * H * W * 4 + F * 2 * 4 + C * H * W * 4          # 76,960
HBM_PEAK_GBS = 8000.0                                               # MI355X_MICROARCH.md
CACHE_BYTES = 256 << 20


TRAFFIC_FILE = "profiles/pmc_traffic.json"


def load_traffic():
    """HBM bytes per launch from the PMC passes, if a summary was committed (profiles/): (bytes, kernel it was
    measured on).  Not measured in this run: PMC collection needs its own rocprofv3 passes."""
    try:
        d = json.load(open(os.path.join(ROOT, TRAFFIC_FILE)))
        return d.get("hbm_bytes_per_launch"), d.get("kernel")
    except Exception:
        return None, None


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(img, ctrl, inv, p_hat, budget_s=10.0):
    """The CPU oracle on the host cores, same workload, bounded sample: all threads and one thread
    (SURVEY.md section 8d), plus the reference's own composition on PyTorch's CPU kernels."""
    from oracle import tps_oracle as O
    O.build()
    threads = O.max_threads()

    out_buf = np.empty((img.shape[0], C, H, W), dtype=np.float32)   # reused: no first-touch page faults inside the timing

    def sample(nthreads, budget):
        O.set_threads(nthreads)
        O.warp(img, ctrl, inv, p_hat, (H, W), out0=out_buf)         # warm-up (page faults, OpenMP)
        t0 = time.perf_counter()
        reps = 0
        while True:
            O.warp(img, ctrl, inv, p_hat, (H, W), out0=out_buf)
            reps += 1
            if time.perf_counter() - t0 >= budget or reps >= 20000:
                break
        return reps, time.perf_counter() - t0

    reps1, dt1 = sample(1, 4.0)
    # thread sweep (1.5 s each): a 512-image batch is 27 ms of work on one core, so beyond a few dozen threads a call is
    # dominated by the OpenMP fork / join and the Python call; the baseline is quoted at the best count
    sweep = {}
    for t in sorted({min(threads, x) for x in (8, 16, 32, 64, threads)}):
        r_, d_ = sample(t, 1.5)
        sweep[t] = r_ * BATCH / d_
    best_t = max(sweep, key=sweep.get)
    reps, dt = sample(best_t, budget_s - 2.0)
    all_threads_rate = sweep[threads]
    threads_used = best_t
    O.set_threads(threads)
    # the same arithmetic as the reference composes it, on PyTorch's CPU kernels (torch.bmm x2 +
    # F.grid_sample; tps_preprocessor.py:71-83,270-282), all host threads, ~6 s sample
    import torch.nn.functional as Fn
    with torch.no_grad():
        ti, tc = torch.from_numpy(img), torch.from_numpy(ctrl)
        tinv = torch.from_numpy(inv).unsqueeze(0).repeat(BATCH, 1, 1)
        tph = torch.from_numpy(p_hat).unsqueeze(0).repeat(BATCH, 1, 1)

        def ref_step():
            cz = torch.cat((tc, torch.zeros(BATCH, 3, 2)), dim=1)
            grid = torch.bmm(tph, torch.bmm(tinv, cz)).reshape(BATCH, H, W, 2)
            return Fn.grid_sample(ti, grid, padding_mode="border", align_corners=True)
        ref_step()
        t1 = time.perf_counter()
        treps = 0
        while time.perf_counter() - t1 < 6.0 and treps < 2000:
            ref_step()
            treps += 1
        tdt = time.perf_counter() - t1
    return {"value": reps * BATCH / dt, "unit": "images/s", "cores": threads_used, "kind": "port",
            "cpu_model": cpu_model(), "host_threads_available": threads,
            "sample": f"{reps} batches of {BATCH} images (3x32x100, F=20) in {dt:.1f} s, "
                      f"oracle/tps_oracle.c with {threads_used} OpenMP threads (the best of the sweep below), output "
                      "buffer reused between calls",
            # flat scalars (nested objects are dropped by the driver's parser)
            "thread_sweep_images_per_s": " ".join(f"{k}:{v:.0f}" for k, v in sweep.items()),
            "all_host_threads_images_per_s": all_threads_rate,
            "all_host_threads_note": "one 512-image batch per call is ~27 ms of single-core work: with every host thread a "
                                     "call is mostly OpenMP fork / join + the ctypes call",
            "one_thread_images_per_s": reps1 * BATCH / dt1,
            # the reference's own composition (torch.bmm x2 + F.grid_sample, tps_preprocessor.py:79-83,270-282) on PyTorch's
            # CPU kernels: what north_star calls "the reference's CPU path"
            "reference_composition_images_per_s": treps * BATCH / tdt,
            "reference_composition_threads": torch.get_num_threads(),
            "reference_composition_sample": f"{treps} batches of {BATCH} in {tdt:.1f} s: torch.bmm x2 + F.grid_sample as the "
                                            "reference composes them, PyTorch CPU kernels"}


def extra_measurements(dev):
    """Not the headline metric: the other two figures BASELINE.md section 5 asks for, measured with the
    same protocol (inputs resident, HIP events, warm caches) on rank 0 at N = 1.
      * warp stage at the TPS_PP geometry (batch 512, fp32): HBM roofline fraction;
      * whole TPS++ module forward (regressor + warp, batch 512, fp32): images/s against the
        north-star's >= 50k."""
    from tps_pp_amd import TPS_PP, ops

    def timeit(fn, iters, warm):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / iters

    n = 512
    m = TPS_PP().eval().to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand((n, 64, 16, 64), generator=g, device=dev)
    o0 = torch.rand((n, 32, 32, 128), generator=g, device=dev)
    o1 = torch.rand((n, 32, 32, 128), generator=g, device=dev)
    with torch.no_grad():
        t_full = timeit(lambda: m(x, [o0, o1]), 10, 4)
        cp, sc, fg = m.regress(x, [o0, o1])
        t_warp = timeit(lambda: m.rectify(fg, x, cp, sc), 20, 3)
        # row F2: backward of the same warp stage (input, control-point and score gradients)
        at = m.atten_tps
        P_xy, P_hat_t = at.device_constants(dev)
        fgc = fg.contiguous()
        _, _, grid, _ = ops.warp(fgc, cp, at.hat_C, at.P_hat, (16, 64), P_xy=P_xy, score=sc, in1=x, want_grid=True,
                                 P_hat_t=P_hat_t)
        g0 = torch.rand((n, 64, 16, 64), generator=g, device=dev)
        g1 = torch.rand((n, 64, 16, 64), generator=g, device=dev)
        t_bwd = timeit(lambda: ops.warp_backward(g0, fgc, grid, cp, at.hat_C, at.P_hat, (16, 64), P_xy=P_xy, score=sc,
                                                 in1=x, g_out1=g1, P_hat_t=P_hat_t), 10, 3)
        del g0, g1, grid, fgc
        # the classic rectifier's backward (configs[1] geometry: 3 x 32 x 100, 20 fiducials), one launch per batch
        from tps_pp_amd import TPSPreprocessor, constants
        gc = TPSPreprocessor(20, (32, 100), (32, 100), 3).eval().to(dev).GridGenerator
        tab_t, tab_flags = gc.prepared_table()
        cimg = torch.rand((n, 3, 32, 100), generator=g, device=dev)
        cctrl = torch.from_numpy(constants.classic_initial_ctrl(20)).to(dev)[None].repeat(n, 1, 1).contiguous()
        cctrl = cctrl + 0.05 * (torch.rand(cctrl.shape, generator=g, device=dev) - 0.5)
        cgo = torch.rand((n, 3, 32, 100), generator=g, device=dev)
        _, _, cgrid, _ = ops.warp(cimg, cctrl, gc.inv_delta_C, gc.P_hat, (32, 100), want_grid=True, P_hat_t=tab_t,
                                  table_flags=tab_flags)
        t_cbwd = timeit(lambda: ops.warp_backward(cgo, cimg, cgrid, cctrl, gc.inv_delta_C, gc.P_hat, (32, 100),
                                                  P_hat_t=tab_t), 30, 5)
        del cimg, cgo, cgrid, gc
        # the same fp32 tensors with the three-term bf16 split in the convolutions ("bf16x3": within the 1e-4 bar,
        # tests/test_gpu_modules.py::test_tpspp_module_bf16x3_meets_the_fp32_bar)
        m.compute_dtype = "bf16x3"
        t_x3 = timeit(lambda: m(x, [o0, o1]), 10, 4)
        m.compute_dtype = None
        # BASELINE.json configs[2]: the same module at batch 1024 on bf16 activations (bf16 MFMA convolutions;
        # control points, TPS solve, grid and sampling stay fp32)
        n2 = 1024
        xb = torch.rand((n2, 64, 16, 64), generator=g, device=dev).to(torch.bfloat16)
        o0b = torch.rand((n2, 32, 32, 128), generator=g, device=dev).to(torch.bfloat16)
        o1b = torch.rand((n2, 32, 32, 128), generator=g, device=dev).to(torch.bfloat16)
        t_bf16 = timeit(lambda: m(xb, [o0b, o1b]), 10, 4)
        del xb, o0b, o1b
    bytes_img = 1966336                                  # SURVEY.md section 8d, G-PP warp stage fp32
    bw = bytes_img * n / (t_warp * 1e-3) / 1e9
    # backward: read g_out0, g_out1, both inputs, grid, score; write g_in0, g_in1, g_score (fp32)
    bwd_bytes_img = 4 * (2 * 64 * 1024 + 2 * (64 * 32 * 128 + 64 * 16 * 64) + 2 * 1024 + 2 * 32 * 1024)
    del m, x, o0, o1
    rec = recognizer_measurement(dev, timeit)
    return {"nrtr_tpspp_inference_batch512_fp32": rec,
            "tpspp_warp_backward_batch512_fp32": {"us_per_batch": t_bwd * 1e3,
                                                  "achieved_GBps": bwd_bytes_img * n / (t_bwd * 1e-3) / 1e9,
                                                  "algorithmic_bytes_per_image": bwd_bytes_img,
                                                  "kernels": "warp_bwd_sample_lds2_kernel (fp64 LDS atomics) + warp_bwd_params_kernel<36,...> (table columns per wavefront; the last workgroup of an image applies inv_delta_C^T)"},
            # read g_out, the image and the grid; write dL/d image, dL/d grid, dL/d control points (fp32)
            "classic_warp_backward_batch512_fp32": {"us_per_batch": t_cbwd * 1e3,
                                                    "achieved_GBps": 4 * (3 * 3 * 3200 + 2 * 2 * 3200 + 40) * n / (t_cbwd * 1e-3) / 1e9,
                                                    "algorithmic_bytes_per_image": 4 * (3 * 3 * 3200 + 2 * 2 * 3200 + 40),
                                                    "kernel": "warp_bwd_classic_kernel<3>: one launch (image staged in LDS, fp64 LDS accumulators, dL/dT and inv_delta_C^T in the workgroup); host-inclusive time of ops.warp_backward (allocations + one launch)"},
            "tpspp_module_batch512_fp32": {"images_per_s": n / (t_full * 1e-3), "ms_per_batch": t_full,
                                           "gflop_per_image": 0.82},
            "tpspp_module_batch512_bf16x3": {"images_per_s": n / (t_x3 * 1e-3), "ms_per_batch": t_x3,
                                             "note": "fp32 tensors, convolution products as hi*hi + hi*lo + lo*hi of bf16 "
                                                     "halves: within 1e-4 of the reference"},
            "tpspp_module_batch1024_bf16": {"images_per_s": n2 / (t_bf16 * 1e-3), "ms_per_batch": t_bf16,
                                            "gflop_per_image": 0.82,
                                            "note": "BASELINE.json configs[2]: bf16 tensors at the module boundary"},
            "tpspp_warp_stage_batch512_fp32": {"us_per_batch": t_warp * 1e3, "achieved_GBps": bw,
                                               "frac_of_hbm_peak": bw / HBM_PEAK_GBS,
                                               "algorithmic_bytes_per_image": bytes_img,
                                               "kernel": "tps_warp_stream_kernel<32,true,true,2>"}}


def classic_warp_extra(dev, hw, nstreams, kernel_choice=0):
    """The classic warp at another geometry (configs/textrecog/nrtr/nrtr_tps++.py:28-33: img_size 32x128, 3 channels,
    20 fiducials), batch 512, same protocol as the headline: rotating buffer sets > 2x the Infinity Cache, one
    pre-marshalled call per step, HIP events; on one stream and on `nstreams`."""
    Hh, Ww = hw
    if kernel_choice:
        ops.set_warp_tuning(0, 0, kernel_choice, 0)
        try:
            return classic_warp_extra(dev, hw, nstreams)
        finally:
            ops.set_warp_tuning(0, 0, 0, 0)
    mod = TPSPreprocessor(num_fiducial=F, img_size=hw, rectified_img_size=hw, num_img_channel=C).eval().to(dev)
    gg = mod.GridGenerator
    p_hat_t, flags = gg.prepared_table()
    per_set = 2 * BATCH * C * Hh * Ww * 4
    nbuf = max(2, (2 * CACHE_BYTES + per_set - 1) // per_set)
    g = torch.Generator(device=dev).manual_seed(99)
    ident = torch.from_numpy(constants.classic_identity_ctrl(F)).to(dev)
    imgs = [torch.rand((BATCH, C, Hh, Ww), generator=g, device=dev) * 2 - 1 for _ in range(nbuf)]
    ctrls = [ident[None] + 0.05 * (torch.rand((BATCH, F, 2), generator=g, device=dev) * 2 - 1) for _ in range(nbuf)]
    outs = [torch.empty((BATCH, C, Hh, Ww), device=dev) for _ in range(nbuf)]
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(nstreams - 1)]
    plans = []
    for j in range(nbuf):
        row = []
        for st in streams:
            with torch.cuda.stream(st):
                row.append(ops.WarpPlan(imgs[j], ctrls[j], gg.inv_delta_C, gg.P_hat, hw, outs[j], P_hat_t=p_hat_t,
                                        table_flags=flags))
        plans.append(row)

    def timed(nsteps, ns):
        for i in range(50):
            plans[i % nbuf][i % ns].run()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = [torch.cuda.Event(enable_timing=True) for _ in range(ns)]
        e0.record(streams[0])                                  # (created at their first record: in front of the region)
        for k in range(ns):
            e1[k].record(streams[k])
        torch.cuda.synchronize(dev)
        e0.record(streams[0])
        for st in streams[1:ns]:
            st.wait_event(e0)
        for i in range(nsteps):
            plans[i % nbuf][i % ns].run()
        for k in range(ns):
            e1[k].record(streams[k])
        torch.cuda.synchronize(dev)
        return max(e0.elapsed_time(e) for e in e1) * 1e3 / nsteps

    us1, usn = timed(1000, 1), timed(1000, nstreams)
    # parity of what was timed: four images against the CPU oracle
    from oracle import tps_oracle as O
    O.build()
    plans[0][0].run()
    torch.cuda.synchronize(dev)
    sel = [0, 1, 255, 511]
    ref = O.warp(imgs[0][sel].cpu().numpy(), ctrls[0][sel].cpu().numpy(), gg.inv_delta_C.cpu().numpy(),
                 gg.P_hat.cpu().numpy(), hw)
    err = float(np.abs(outs[0][sel].cpu().numpy() - ref["out0"]).max())
    bytes_launch = BATCH * (2 * C * Hh * Ww * 4 + F * 2 * 4)
    return {"launch_us": usn, "streams": nstreams, "frac_of_hbm_peak": bytes_launch / (usn * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "one_stream": {"launch_us": us1, "frac_of_hbm_peak": bytes_launch / (us1 * 1e-6) / 1e9 / HBM_PEAK_GBS},
            "algorithmic_bytes_per_launch": bytes_launch, "max_abs_err_vs_oracle": err,
            "kernel": "automatic choice of tpspp_warp_fwd: tps_warp_img_kernel (instantiated in-place staging) for 32x100, "
                      "32x128, 48x160, 32x64, 32x160; else tps_warp_geo_kernel (one workgroup per image, run-time geometry) or, "
                      "for larger images, tps_warp_span_kernel (row bands, span staging)"
            if bool(flags & ops.TABLE_PACKED) else "LDS-staged kernel", "rotating_buffer_sets": int(nbuf)}


def device_clocks():
    """Best effort: the device's current clock levels as the amdgpu driver's sysfs files report them, read right behind the
    timed regions (no child process: rocm-smi is a `#!/usr/bin/env python3` script, and a process that has initialised the GPU
    must not exec one on this pool).  The cards are not mapped to HIP devices here: the levels of every card that shows an
    active shader clock are listed.  None when nothing is readable."""
    import glob
    out = {}
    for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_*clk")):
        try:
            cur = [ln.strip() for ln in open(f).read().splitlines() if ln.strip().endswith("*")]
        except OSError:
            continue
        if cur:
            card = f.split("/")[4]
            out.setdefault(card, {})[os.path.basename(f)[len("pp_dpm_"):]] = cur[0].rstrip(" *")

    def mhz(v):
        try:
            return int(v.split(":")[1].strip().lower().replace("mhz", ""))
        except (IndexError, ValueError):
            return 0
    # only the cards whose shader clock is up (this process's GPU -- and whatever other GPUs of the node are busy for other
    # tenants at that moment: the host's cores are shared with them)
    busy = {c: {k: v for k, v in d.items() if k in ("sclk", "mclk", "fclk", "socclk")} for c, d in out.items() if mhz(d.get("sclk", "")) >= 1000}
    return {"cards_with_shader_clock_up": busy, "cards_in_sysfs": len(out)} if out else None


def recognizer_measurement(dev, timeit):
    """BASELINE.json configs[3]/[4] shape at one GPU: the whole NRTR + TPS++ recogniser (backbone, TPS++,
    6+6-layer transformer, greedy 40-step decoding, label conversion) on 3x32x128 images, batch 512,
    random-init weights; plus a string-parity check of a small batch against the CPU oracle."""
    import tps_pp_amd as P
    from oracle import tpspp_oracle as TO
    torch.manual_seed(11)
    m = P.build_detector(NRTR_TPSPP_MODEL).eval()
    with torch.no_grad():      # spread the classifier so that the random-init arg-max is far from ties
        m.decoder.classifier.weight.mul_(8.0)
    sds = [{k: v.clone() for k, v in mod.state_dict().items()} for mod in (m.backbone, m.tpsnet, m.encoder, m.decoder)]
    m = m.to(dev)
    n = 512
    g = torch.Generator(device=dev).manual_seed(12)
    img = torch.rand((n, 3, 32, 128), generator=g, device=dev) * 2 - 1
    metas = [dict(resize_shape=(32, 128, 3)) for _ in range(n)]
    def stages():
        """The three device stages of simple_test enqueued back to back, nothing copied to the host: what is left of
        ms_per_batch beyond this is the label conversion's kernel + its one device->host copy + the host's string work."""
        feat_ = m.extract_feat(img, test=True)["output"]
        return m.decoder(feat_, m.encoder(feat_, metas), None, metas, train_mode=False)

    def whole_and_stages():
        """ms of the whole simple_test and of its three device stages back to back: two alternating rounds of three calls each,
        the faster round counts (round 6: timed once, one after the other, the difference -- ms_outside_stages, ~1 ms of a
        20 - 50 ms batch -- carried whatever one-off cost the first of the two met: 0.8 / 2.0 ms in two runs of one tree)."""
        full = lambda: m(img, metas, return_loss=False)           # noqa: E731
        a1 = timeit(full, 3, 1); b1 = timeit(stages, 3, 1); a2 = timeit(full, 3, 1); b2 = timeit(stages, 3, 1)
        return min(a1, a2), min(b1, b2)

    with torch.no_grad():
        t_all, t_b2b = whole_and_stages()
        t_feat = timeit(lambda: m.extract_feat(img, test=True), 3, 1)
        feat = m.extract_feat(img, test=True)["output"]
        t_enc = timeit(lambda: m.encoder(feat, None), 3, 1)
        out_enc = m.encoder(feat, None)
        t_dec = timeit(lambda: m.decoder(feat, out_enc, None, None, train_mode=False), 3, 1)
        k = 4
        got = [r["text"] for r in m(img[:k], metas[:k], return_loss=False)]
        # fp32 tensors, three-term bf16 split in every wide matrix product (within 1e-4: strings must not change)
        m.backbone.compute_dtype = m.tpsnet.compute_dtype = m.encoder.compute_dtype = m.decoder.compute_dtype = "bf16x3"
        t_allx3, t_b2bx3 = whole_and_stages()
        t_featx3 = timeit(lambda: m.extract_feat(img, test=True), 3, 1)
        t_encx3 = timeit(lambda: m.encoder(feat, None), 3, 1)
        out_encx3 = m.encoder(feat, None)
        t_decx3 = timeit(lambda: m.decoder(feat, out_encx3, None, None, train_mode=False), 3, 1)
        gotx3 = [r["text"] for r in m(img[:k], metas[:k], return_loss=False)]
        m.tpsnet.compute_dtype = m.encoder.compute_dtype = m.decoder.compute_dtype = None
        # BASELINE.json configs[4]: backbone + TPS++ convolutions on the bf16 matrix cores (head stays fp32)
        m.backbone.compute_dtype = torch.bfloat16
        t_all16 = timeit(lambda: m(img, metas, return_loss=False), 3, 1)
        t_feat16 = timeit(lambda: m.extract_feat(img, test=True), 3, 1)
        got16 = [r["text"] for r in m(img[:k], metas[:k], return_loss=False)]
        # ... and the head's wide projections + encoder keys / values in bf16 (TPSPP_HEAD_BF16)
        m.encoder.compute_dtype = m.decoder.compute_dtype = torch.bfloat16
        t_all16h, t_b2b16h = whole_and_stages()
        t_enc16 = timeit(lambda: m.encoder(feat, None), 3, 1)
        out_enc16 = m.encoder(feat, None)
        t_dec16 = timeit(lambda: m.decoder(feat, out_enc16, None, None, train_mode=False), 3, 1)
        got16h = [r["text"] for r in m(img[:k], metas[:k], return_loss=False)]
        m.encoder.compute_dtype = m.decoder.compute_dtype = None
        m.backbone.compute_dtype = None
    want = TO.recognizer_simple_test(sds[0], sds[1], sds[2], sds[3], img[:k].cpu().numpy(), [128] * k)["text"]
    # configs[4]: decisions of the reduced-precision configurations against the exact-fp32 kernels, 256 images
    from tps_pp_amd import metrics
    agree16 = metrics.precision_agreement(m, img[:256], metas[:256], torch.bfloat16)
    agreex3 = metrics.precision_agreement(m, img[:256], metas[:256], "bf16x3")
    # where the bf16 configuration's flipped decisions come from: one stage in bf16 at a time (the decoder's per-step
    # projections and the classifier are on the three-term split in EVERY reduced mode, include/tpspp.h)
    bf = torch.bfloat16
    stages = {}
    for name, md in (("bf16_backbone__fp32_head", dict(backbone=bf)),
                     ("fp32_backbone__bf16_head", dict(encoder=bf, decoder=bf)),
                     ("fp32_backbone__bf16_encoder_only", dict(encoder=bf)),
                     ("fp32_backbone__bf16_decoder_keys_values_only", dict(decoder=bf)),
                     ("bf16_backbone__bf16x3_head", dict(backbone=bf, encoder="bf16x3", decoder="bf16x3"))):
        r = metrics.precision_agreement(m, img[:256], metas[:256], md)
        stages[name] = {k: r[k] for k in ("teacher_forced_argmax_agreement", "greedy_word_agreement", "greedy_char_agreement",
                                          "teacher_forced_agreement_margin_ge_0.05", "greedy_agreement_up_to_first_margin_lt_0.05")}
    outside = "ms_per_batch - ms_three_stages_back_to_back, same process: tpspp_attn_tensor2idx_fwd + one device->host copy + strings"
    return {"images_per_s": n / (t_all * 1e-3), "ms_per_batch": t_all,
            "ms_three_stages_back_to_back": t_b2b, "ms_outside_stages": t_all - t_b2b, "ms_outside_stages_is": outside,
            "ms_backbone_tpspp": t_feat, "ms_encoder": t_enc, "ms_greedy_decoder_40_steps": t_dec,
            "strings_equal_to_cpu_oracle": f"{sum(a == b for a, b in zip(got, want))}/{k}",
            "parity_configuration_of_configs4": "bf16x3 (fp32 tensors, three-term bf16 split: scores within 1e-4, strings "
                                                "identical); plain bf16 below is the THROUGHPUT configuration, not a parity claim "
                                                "-- see its agreement figures, incl. the ones restricted to fp32 top-2 margin >= 0.05",
            "bf16x3": {"images_per_s": n / (t_allx3 * 1e-3), "ms_per_batch": t_allx3,
                       "ms_three_stages_back_to_back": t_b2bx3, "ms_outside_stages": t_allx3 - t_b2bx3, "ms_backbone_tpspp": t_featx3,
                       "ms_encoder": t_encx3, "ms_greedy_decoder_40_steps": t_decx3,
                       "strings_equal_to_fp32_cpu_oracle": f"{sum(a == b for a, b in zip(gotx3, want))}/{k}",
                       "agreement_with_fp32_kernels_256_images": agreex3},
            "bf16_backbone": {"images_per_s": n / (t_all16 * 1e-3), "ms_per_batch": t_all16,
                              "ms_backbone_tpspp": t_feat16,
                              "strings_equal_to_fp32_cpu_oracle": f"{sum(a == b for a, b in zip(got16, want))}/{k}"},
            "bf16_backbone_and_head": {"images_per_s": n / (t_all16h * 1e-3), "ms_per_batch": t_all16h,
                                       "ms_three_stages_back_to_back": t_b2b16h, "ms_outside_stages": t_all16h - t_b2b16h,
                                       "ms_encoder": t_enc16, "ms_greedy_decoder_40_steps": t_dec16,
                                       "strings_equal_to_fp32_cpu_oracle":
                                           f"{sum(a == b for a, b in zip(got16h, want))}/{k}",
                                       "agreement_with_fp32_kernels_256_images": agree16,
                                       "agreement_by_stage_256_images": stages},
            "data": "synthetic images, random-init weights"}


def _free_port():
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def self_launch(a):
    """`python bench.py --gpus N` typed without a launcher: start the N ranks as children (torch.distributed.run)
    and pass their output through.  This process never initialises a GPU and never exec()s."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.run(cmd, env=env).returncode


def dry_run(a, world, rank):
    """CPU stand-in for the launch path (tests/test_bench_launch.py): the same process-group set-up, barrier,
    all-gather of per-rank rows and max-over-ranks reduction, on gloo, without a GPU and without the kernels."""
    from tps_pp_amd import dist as tdist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    rows = torch.full((3, 40, 93), float(rank))
    t0 = time.perf_counter()
    got = tdist.all_gather_rows(rows, 3 * world) if world > 1 else rows
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    ok = all(float(got[3 * r, 0, 0]) == r for r in range(world))
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                          "gathered_rows": int(got.shape[0]), "gather_ok": bool(ok)}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0 if ok else 1


def recognizer_sharded(dev, world, rank, per_rank=256):
    """N > 1: the whole recogniser (NRTR + TPS++, the model dict of configs/textrecog/nrtr/nrtr_tps++.py:26-42) on
    `per_rank` 3x32x128 images per rank; the decoder scores (per_rank, 40, 92) fp32 of every rank are all-gathered
    over RCCL inside the timed region and every rank converts the full tensor to strings (tools/test.py:202-207)."""
    import tps_pp_amd as P
    from tps_pp_amd import dist as tdist
    torch.manual_seed(11)                                            # identical replicated weights on every rank
    m = P.build_detector(NRTR_TPSPP_MODEL).eval().to(dev)
    n_total = per_rank * world
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    img = torch.rand((per_rank, 3, 32, 128), generator=g, device=dev) * 2 - 1
    metas = [dict(resize_shape=(32, 128, 3)) for _ in range(per_rank)]

    def decode_local(lo, hi):
        feat = m.extract_feat(img, test=True)["output"]
        return m.decoder(feat, m.encoder(feat, metas), None, metas, train_mode=False)

    def once():
        torch.cuda.synchronize(dev)
        dist.barrier()
        t0 = time.perf_counter()
        res = tdist.recognize_sharded(decode_local, n_total, m.label_convertor)
        torch.cuda.synchronize(dev)
        dist.barrier()
        return time.perf_counter() - t0, res

    with torch.no_grad():
        once()
        times = []
        for _ in range(3):
            dt, res = once()
            times.append(dt)
    tt = torch.tensor([min(times), -min(times)], device=dev, dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    payload = per_rank * 40 * 92 * 4
    # the collective alone (HIP events on the stream the process group enqueues behind): separates compute from the
    # all-gather in a scaling curve
    scores = torch.zeros((per_rank, 40, 92), device=dev)
    for _ in range(3):
        tdist.all_gather_rows(scores, n_total)
    torch.cuda.synchronize(dev)
    dist.barrier()
    g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g0.record()
    for _ in range(20):
        tdist.all_gather_rows(scores, n_total)
    g1.record()
    torch.cuda.synchronize(dev)
    ag = torch.tensor([g0.elapsed_time(g1) * 1e3 / 20], device=dev, dtype=torch.float64)
    dist.all_reduce(ag, op=dist.ReduceOp.MAX)
    return {"images_per_s": n_total / float(tt[0]), "ms_per_batch": float(tt[0]) * 1e3,
            "ms_per_batch_fastest_rank": -float(tt[1]) * 1e3, "images_per_rank": per_rank,
            "timing": "host clock around barrier -> decode + all-gather + strings -> synchronize -> barrier, min of 3, "
                      "max over ranks (a 30 ms step: the ~0.1 ms of the two barriers is inside it)",
            "all_gather_us": float(ag[0]),
            "all_gather_timing": "HIP events around 20 back-to-back all-gathers of the same payload, max over ranks",
            "strings_returned": len(res), "collective": "all_gather_into_tensor of (images_per_rank, 40, 92) fp32 scores",
            "all_gather_bytes_per_rank": payload, "backend": dist.get_backend(), "rccl_world_size": dist.get_world_size(),
            "env": {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "HSA_ENABLE_IPC_MODE_LEGACY", "NCCL_DEBUG",
                                                   "MASTER_ADDR", "LOCAL_WORLD_SIZE")},
            "data": "synthetic images, random-init weights (replicated)"}


# the model dict of configs/textrecog/nrtr/nrtr_tps++.py:26-42 (values typed here; dictionary file replaced by DICT90)
NRTR_TPSPP_MODEL = dict(
    type="NRTR",
    backbone=dict(type="ResNetABI_v2_large", arch_settings=[3, 4, 6, 6, 3], strides=[2, 1, 2, 1, 2]),
    tpsnet=dict(type="TPS_PP"),
    encoder=dict(type="NRTREncoder"),
    decoder=dict(type="NRTRDecoder"),
    loss=dict(type="TFLoss"),
    label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
    max_seq_len=40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: both launch protocols over `--repeats` regions each, parity against the CPU "
                         "oracle, plain-copy ceiling, device clocks, `extra` and `cpu_baseline`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the rectified batch of the last timed step to DIR/rectified.npy (float32)")
    ap.add_argument("--repeats", type=int, default=0,
                    help="--full: timed regions of `steps` steps per launch protocol (0 = 5 when steps <= 200, else 1)")
    ap.add_argument("--streams", type=int, default=0,
                    help="HIP streams the steps are launched on, round-robin (1 = every launch waits for the previous one; "
                         "0 = 2 when steps <= 200, else 3)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without `cpu_baseline`")
    ap.add_argument("--no-extras", action="store_true", help="--full without `extra`")
    ap.add_argument("--precondition-ms", type=float, default=300.0,
                    help="device copies over the bench buffers before the warm-up steps: the chip leaves its idle "
                         "clocks only after some hundred ms of activity (not steps of the workload; 0 disables)")
    ap.add_argument("--dry-run", action="store_true", help="CPU / gloo check of the launch path, no GPU work")
    ap.add_argument("--sharded-extra", action="store_true",
                    help="--full: run extra.recognizer_sharded at N = 1 as well (a 1-rank RCCL group): exercises the N > 1 "
                         "code path on a single-GPU machine")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but the launcher started {world} ranks (WORLD_SIZE={world})")
    if a.dry_run:
        raise SystemExit(dry_run(a, world, rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    # ---- the module boundary a recognizer would hold (constants, prepared table) ----
    mod = TPSPreprocessor(num_fiducial=F, img_size=(H, W), rectified_img_size=(H, W),
                          num_img_channel=C).eval().to(dev)
    gg = mod.GridGenerator
    p_hat_t, flags = gg.prepared_table()
    pair_kernel = bool(flags & ops.TABLE_PACKED) and bool(flags & ops.TABLE_MIRROR4)

    # ---- synthetic inputs, resident in HBM; buffer 0 is the exactly reproducible one ----
    per_set = 2 * BATCH * C * H * W * 4
    nbuf = max(2, (2 * CACHE_BYTES + per_set - 1) // per_set)       # >= 2x the Infinity Cache
    ident = constants.classic_identity_ctrl(F)
    img0 = synth.dyadic((BATCH, C, H, W), f"bench.img.r{rank}")
    ctrl0 = (ident[None] + 0.05 * synth.dyadic((BATCH, F, 2), f"bench.ctrl.r{rank}")).astype(np.float32)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    imgs = [torch.from_numpy(img0).to(dev)]
    ctrls = [torch.from_numpy(ctrl0).to(dev)]
    ident_d = torch.from_numpy(ident).to(dev)
    for _ in range(1, nbuf):
        imgs.append(torch.rand((BATCH, C, H, W), generator=g, device=dev) * 2 - 1)
        ctrls.append(ident_d[None] + 0.05 * (torch.rand((BATCH, F, 2), generator=g, device=dev) * 2 - 1))
    outs = [torch.empty((BATCH, C, H, W), device=dev) for _ in range(nbuf)]

    # one validated, pre-marshalled tpspp_warp_fwd call per (buffer set, stream) (ops.WarpPlan: the launch goes to the
    # stream that is current when the plan is built): a step is exactly one foreign call = one kernel launch; per-call
    # tensor checks in Python would cost about a launch period
    # 0 = auto: short regions (the driver's 20 steps) pay for every extra queue's wake-up after the synchronize -- two streams
    # measured best there (8.5-8.9 us against 8.9-9.0 with three and 9.6-9.9 with one); long runs gain a little from a third
    S = int(a.streams) if int(a.streams) > 0 else (2 if a.steps <= 200 else 3)
    S = max(1, min(S, 8))
    main_stream = torch.cuda.current_stream(dev)
    streams = [main_stream] + [torch.cuda.Stream(dev) for _ in range(S - 1)]
    plans = []
    for j in range(nbuf):
        row = []
        for st in streams:
            with torch.cuda.stream(st):
                row.append(ops.WarpPlan(imgs[j], ctrls[j], gg.inv_delta_C, gg.P_hat, (H, W), outs[j], P_hat_t=p_hat_t,
                                        table_flags=flags))
        plans.append(row)

    def step(i, nstreams=S):
        plans[i % nbuf][i % nstreams].run()

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()

    # ---- not steps: keep the device busy with plain copies until its clocks have left the idle state ----
    if a.precondition_ms > 0:
        t_end = time.perf_counter() + a.precondition_ms * 1e-3
        j = 0
        while time.perf_counter() < t_end:
            for _ in range(64):
                outs[j % nbuf].copy_(imgs[j % nbuf])
                j += 1
            torch.cuda.synchronize(dev)

    def timed(nsteps, nstreams, first):
        """Exactly `nsteps` steps, step i on stream i % nstreams.  Every stream records an event before its first and after
        its last launch; the region's time is latest end - earliest start (the maximum over all (start, end) pairs)."""
        e0 = [torch.cuda.Event(enable_timing=True) for _ in range(nstreams)]
        e1 = [torch.cuda.Event(enable_timing=True) for _ in range(nstreams)]
        # torch creates the HIP event at its first record(): that would be a hipEventCreate between the start event and the
        # first launch (and another one in front of the second stream's first launch).  Record every event once here and
        # synchronize again -- still in front of the region; record() re-uses the handle
        for k in range(nstreams):
            e0[k].record(streams[k])
            e1[k].record(streams[k])
        torch.cuda.synchronize(dev)
        gc_was = gc.isenabled()
        gc.disable()                                           # (a collection inside a 160-us region is a host hiccup the device sees)
        t0 = time.perf_counter()
        # (round 6: a stream's start event is recorded right in front of ITS first launch instead of all start events first --
        # the device sat idle behind the earliest start event while the host recorded the others, ~2.5 us of every region)
        pending = set(range(nstreams))
        for i in range(nsteps):
            k = (first + i) % nstreams
            if k in pending:
                pending.discard(k)
                e0[k].record(streams[k])
            step(first + i, nstreams)
        for k in sorted(pending):                              # (fewer steps than streams)
            e0[k].record(streams[k])
        for k in range(nstreams):
            e1[k].record(streams[k])
        torch.cuda.synchronize(dev)
        if gc_was:
            gc.enable()
        return max(b.elapsed_time(e) for e in e1 for b in e0), time.perf_counter() - t0

    for i in range(a.warmup):
        step(i)
    alg_bytes = BYTES_PER_IMG * BATCH
    kernel = "tps_warp_pair_kernel<20,3,32,100,32,100,false,false>" if pair_kernel else \
        "tps_warp_lds_mirror_kernel<20,3,32,100,false>"
    if not a.full:
        # ---- plain run: one region of exactly `steps` steps on S streams, nothing else on the device ----
        barrier()
        tt = torch.tensor(timed(a.steps, S, a.warmup), device=dev, dtype=torch.float64)    # (ms, wall s)
        if world > 1:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        ev_ms, dt = float(tt[0]), float(tt[1])
        rec = None
        if rank == 0:
            if a.dump_outputs:
                dump_outputs(a.dump_outputs, outs[(a.warmup + a.steps - 1) % nbuf])
            launch_us = ev_ms * 1e3 / a.steps
            achieved = alg_bytes / (launch_us * 1e-6) / 1e9
            rec = {
                **headline(world, a.steps, a.warmup, ev_ms, dt),
                "config": {"workload": "BASELINE.json configs[1]: fused TPS grid-gen + bilinear "
                                       "grid_sample HIP kernel, batch 512 per GPU, 3x32x100 fp32, "
                                       "20 fiducials, inputs resident in HBM",
                           "batch_per_gpu": BATCH, "rotating_buffer_sets": int(nbuf),
                           "working_set_MB": round(nbuf * per_set / 1e6, 1),
                           "streams": S, "repeats": 1,
                           "timing": f"one region of exactly `steps` launches (barrier + synchronize before it), step i on HIP "
                                     f"stream i % {S}; HIP events per stream, region = latest end - earliest start, max over "
                                     "ranks; --full for both launch protocols over repeated regions",
                           "preconditioning": f"{a.precondition_ms:.0f} ms of plain device copies over the bench buffers "
                                              "before the warm-up steps (clock ramp; not steps)"},
                "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK_GBS, "kernel": kernel, "algorithmic_bytes_per_launch": alg_bytes,
                             "launch_us": launch_us,
                             "launch_us_is": f"region of `steps` launches on {S} stream(s) / steps"
                                             + ("; launches overlap: a period, not one kernel's duration" if S > 1 else "")},
            }
        if world > 1:
            dist.destroy_process_group()
        if rank == 0:
            print_line(rec)
        return

    # `repeats` timed regions of exactly `steps` steps per protocol (barrier + synchronize before each).  A 20-step region is
    # 0.2 ms: one region alone is at the mercy of the queues' wake-up after the synchronize.
    R = a.repeats if a.repeats > 0 else (5 if a.steps <= 200 else 1)
    # Round 6: the two protocols' regions are INTERLEAVED (S-stream region r, then one-stream region r, r = 0 .. R - 1) instead of
    # all S-stream regions first: on some boxes of the pool the first regions after the warm-up steps are measurably slower than
    # the later ones (r06: 9.88, 9.48, 9.24, 9.03, 9.08 us over five consecutive one-stream regions), and the protocol that ran
    # first carried all of that.  Same regions, same estimator (median per protocol), neither protocol favoured.
    reg_m, reg_1 = [], []
    for r in range(R):
        barrier()
        reg_m.append(timed(a.steps, S, a.warmup + 2 * r * a.steps))
        last = a.warmup + (2 * r + 1) * a.steps - 1
        if S > 1:
            barrier()
            reg_1.append(timed(a.steps, 1, a.warmup + (2 * r + 1) * a.steps))
            last = a.warmup + (2 * r + 2) * a.steps - 1
    if S == 1:
        reg_1 = reg_m
    # a region's time is the MAX over ranks (every rank times the same R regions behind the same barriers); the
    # estimator is then the fastest region, with the median and every region's time reported beside it
    tt = torch.tensor([[list(x) for x in reg_m], [list(x) for x in reg_1]], device=dev, dtype=torch.float64)   # (2, R, 2)
    tt_min = tt.clone()
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dist.all_reduce(tt_min, op=dist.ReduceOp.MIN)
    tt, tt_min = tt.cpu(), tt_min.cpu()
    clocks = device_clocks() if rank == 0 else None          # (right behind the last region: what the device ran at)
    if rank == 0 and a.dump_outputs:                         # (before the parity step below rewrites buffer set 0)
        dump_outputs(a.dump_outputs, outs[last % nbuf])
    regions_m = [float(x) for x in tt[0, :, 0]]              # ms per region, `steps` launches each
    regions_1 = [float(x) for x in tt[1, :, 0]]

    def median_region(regs):
        """Index of the median region (the lower middle one for an even count: a region that was actually timed)."""
        order = np.argsort(regs)
        return int(order[(len(regs) - 1) // 2])

    km, k1 = median_region(regions_m), median_region(regions_1)
    # `value` / `ms_per_step` / `roofline.frac` come from the MEDIAN region of the protocol whose median is lower (both
    # protocols and the fastest region are reported beside it as flat scalars: roofline.one_stream_frac,
    # roofline.multi_stream_frac_median, roofline.frac_best)
    ms_multi, ms_one = regions_m[km], regions_1[k1]
    used_streams = S if ms_multi <= ms_one else 1
    if used_streams == 1:
        regions_used, ku = regions_1, k1
        ev_ms, dt, ev_ms_min = ms_one, float(tt[1, k1, 1]), float(tt_min[1, k1, 0])
    else:
        regions_used, ku = regions_m, km
        ev_ms, dt, ev_ms_min = ms_multi, float(tt[0, km, 1]), float(tt_min[0, km, 0])
    best_ms = min(regions_used)
    to_us = lambda ms: ms * 1e3 / a.steps                    # noqa: E731  (ms per region -> us per launch)

    # ---- parity spot-check of what was just measured (not timed) ----
    max_err = None
    if rank == 0:
        from oracle import tps_oracle as O
        O.build()
        step(0)
        torch.cuda.synchronize(dev)
        sel = [0, 1, 255, 511]
        ref = O.warp(img0[sel], ctrl0[sel], gg.inv_delta_C.cpu().numpy(), gg.P_hat.cpu().numpy(), (H, W))
        max_err = float(np.abs(outs[0][sel].cpu().numpy() - ref["out0"]).max())

    # ---- the practical ceiling under the same protocol: a plain device copy of the same image bytes
    # (one launch per step over the same rotating buffers; not part of `value`) ----
    copy_us = None
    if rank == 0:
        for i in range(20):
            outs[i % nbuf].copy_(imgs[i % nbuf])
        torch.cuda.synchronize(dev)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for i in range(500):
            outs[i % nbuf].copy_(imgs[i % nbuf])
        c1.record()
        torch.cuda.synchronize(dev)
        copy_us = c0.elapsed_time(c1) * 1e3 / 500

    sharded = None
    if world > 1 and not a.no_extras:
        sharded = recognizer_sharded(dev, world, rank)
    elif a.sharded_extra:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        sharded = recognizer_sharded(dev, 1, 0)
        dist.destroy_process_group()

    rec = None
    if rank == 0:
        def frac_of(us):
            return alg_bytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS

        launch_us = to_us(ev_ms)
        launch1_us = to_us(ms_one)                           # median region, every launch behind the previous one
        launchm_us = to_us(ms_multi)                         # median region, S streams
        achieved = alg_bytes / (launch_us * 1e-6) / 1e9
        traffic, traffic_kernel = load_traffic()
        rec = {
            **headline(world, a.steps, a.warmup, ev_ms, dt),
            "config": {"workload": "BASELINE.json configs[1]: fused TPS grid-gen + bilinear "
                                   "grid_sample HIP kernel, batch 512 per GPU, 3x32x100 fp32, "
                                   "20 fiducials, inputs resident in HBM",
                       "batch_per_gpu": BATCH, "rotating_buffer_sets": int(nbuf),
                       "working_set_MB": round(nbuf * per_set / 1e6, 1),
                       "streams": used_streams, "streams_tried": f"1 and {S}", "repeats": R,
                       "estimator": f"MEDIAN of {R} regions of `steps` launches; of the 2 launch protocols ({S} streams / 1 "
                                    "stream) the one with the lower median; fastest region in roofline.frac_best",
                       "timing": f"two launch protocols, each over `repeats` regions of exactly `steps` launches (barrier + "
                                 f"synchronize before each region): step i on HIP stream i % {S}, and all steps on one "
                                 "stream.  HIP events per stream, region = latest end - earliest start, max over ranks",
                       "timing_detail": "`value` / `ms_per_step` / `roofline.frac` = the median region of the protocol named by "
                                        "`streams`; roofline.one_stream_* = every launch behind the previous one (what a kernel "
                                        "trace shows as the kernel's duration + launch gap); roofline.multi_stream_* = overlapped "
                                        "launches (period between launches); `wall_ms_per_step` = host clock incl. the synchronize",
                       "ms_per_step_min_over_ranks": ev_ms_min / a.steps,
                       "region_order": "interleaved" if S > 1 else "one protocol",
                       "device_clocks_after_regions": clocks,
                       "preconditioning": f"{a.precondition_ms:.0f} ms of plain device copies over the bench buffers "
                                          "before the warm-up steps (clock ramp; not steps)"},
            "max_abs_err_vs_oracle": max_err,
            # every figure the review asks for is a FLAT scalar of `roofline` (nested objects are dropped by the driver's parser)
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_source": f"{TRAFFIC_FILE} (rocprofv3 --pmc passes of this command, measured on "
                                           f"{traffic_kernel}; not re-measured in this run)" if traffic else None,
                         "kernel": kernel,
                         "algorithmic_bytes_per_launch": alg_bytes,
                         "launch_us": launch_us,
                         "launch_us_is": f"median region of `steps` launches on {used_streams} stream(s) / steps"
                                         + ("; launches overlap: a period, not one kernel's duration" if used_streams > 1 else ""),
                         "launch_us_best": to_us(best_ms), "frac_best": frac_of(to_us(best_ms)),
                         "one_stream_launch_us": launch1_us, "one_stream_frac": frac_of(launch1_us),
                         "one_stream_launch_us_best": to_us(min(regions_1)), "one_stream_frac_best": frac_of(to_us(min(regions_1))),
                         "multi_stream_streams": S,
                         "multi_stream_launch_us_median": launchm_us, "multi_stream_frac_median": frac_of(launchm_us),
                         "multi_stream_launch_us_best": to_us(min(regions_m)), "multi_stream_frac_best": frac_of(to_us(min(regions_m))),
                         "plain_copy_launch_us": copy_us, "plain_copy_frac": 2 * BATCH * C * H * W * 4 / (copy_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                         "plain_copy_is": "torch device copy of the same 19.7 MB in + 19.7 MB out per step, same rotating buffers, "
                                          "one stream: the practical ceiling for one launch per 512 images",
                         "regions_us_one_stream": " ".join(f"{to_us(x):.3f}" for x in regions_1),
                         "regions_us_multi_stream": " ".join(f"{to_us(x):.3f}" for x in regions_m)},
        }
        if world == 1 and not a.no_extras:
            del plans, imgs, outs, ctrls
            torch.cuda.empty_cache()
            rec["extra"] = extra_measurements(dev)
            rec["extra"]["classic_warp_32x128_batch512_fp32"] = classic_warp_extra(dev, (32, 128), S)
            # the reference's recog-config test shape (tests/test_models/test_recog_config.py:103-157), and a geometry
            # that only the run-time-geometry in-place kernel takes (tpspp_warp_geo.h)
            rec["extra"]["classic_warp_32x160_batch512_fp32"] = classic_warp_extra(dev, (32, 160), S)
            rec["extra"]["classic_warp_64x200_batch512_fp32"] = classic_warp_extra(dev, (64, 200), S)
            # round 5: an image that fits no LDS as a whole (196 KB; round 4: gather kernel, 0.25), and 48x160 with the
            # run-time-geometry kernels REQUIRED (kernel_choice 7) instead of its instantiated kernel
            rec["extra"]["classic_warp_64x256_batch512_fp32"] = classic_warp_extra(dev, (64, 256), S)
            rec["extra"]["classic_warp_48x160_runtime_geometry_batch512_fp32"] = classic_warp_extra(dev, (48, 160), S, kernel_choice=7)
        if sharded is not None:
            rec.setdefault("extra", {})["recognizer_sharded"] = sharded
        if world == 1 and not a.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(img0, ctrl0, gg.inv_delta_C.cpu().numpy(),
                                               gg.P_hat.cpu().numpy())
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        print_line(rec)


def headline(world, steps, warmup, ev_ms, wall_s):
    """The result line's leading fields: `ev_ms` is the timed region of `steps` launches (HIP events), `wall_s` the host
    clock around it."""
    return {"metric": "rectified images/sec (3x32x100)", "value": world * BATCH * steps / (ev_ms * 1e-3),
            "unit": "images/s", "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": ev_ms / steps,
            "wall_ms_per_step": wall_s * 1e3 / steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic"}


def print_line(rec):
    # RCCL prints its version banner through C stdio, which a pipe buffers until exit: flush it first so that the
    # JSON line is the last line of stdout
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(rec), flush=True)


def dump_outputs(dirname, out):
    """--dump-outputs: the rectified batch (BATCH, C, H, W) of the last timed step, what a caller of the path receives."""
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "rectified.npy"), out.float().cpu().numpy())


if __name__ == "__main__":
    main()
