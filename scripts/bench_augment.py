"""The train pipeline's GPU stage against the test pipeline's: 512 crops of 48 x 160 x 3, resized to 32 x 128.

  (a) tpspp_resize_normalize_fwd, what OCRBatchPreprocessor launches: the yardstick (with --parent-lib, also the same entry
      point of another build of the library, e.g. the commit before the augmentation kernel, alternating with this one);
  (b) tpspp_augment_normalize_fwd with every op list empty;
  (c) with the op lists the reference's train pipeline draws (geometry p = 0.5, ColorJitter p = 0.25);
  (d) with one geometric op and the four colour ops on every image;
  and the host time OCRTrainBatchPreprocessor.plan takes to draw a batch's op lists.

Kernel variants are interleaved region by region: `reps` direct calls of the entry point between two device events (no Python
wrapper, outputs allocated once; where a kernel is shorter than the host's call the figure is the host's rate, which the
end of each row shows by the host clock's time per call), medians over the regions with min and max.  Inputs stay on the
device; the upload of the crops is no part of any figure.

    python scripts/bench_augment.py [--batch 512] [--reps 1000] [--regions 9] [--backend pillow] [--parent-lib other.so]
    python scripts/bench_augment.py --pillow-cpu [--images 2000]     the same pipeline in Pillow on one CPU core (no GPU)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SKIP = ("PyramidRescale", "Albu")


def pipeline(p_geo=None, p_color=None, backend=None):
    import augment_ref
    cfg = augment_ref.train_pipeline(p_geo, p_color)
    next(t for t in cfg if t["type"] == "ResizeOCR")["backend"] = backend
    return cfg


def preprocessor(device, p_geo=None, p_color=None, backend=None, seed=0):
    from tps_pp_amd import OCRTrainBatchPreprocessor
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return OCRTrainBatchPreprocessor(pipeline(p_geo, p_color, backend), device, seed=seed, skip=SKIP)


def crops(n, seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (48, 160, 3), dtype=np.uint8) for _ in range(n)]


def pillow_cpu(n_images):
    """images/s of ResizeOCR + the config's augmentations + ToTensor + Normalize, per image, in Pillow and numpy on this core."""
    import torch
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_augment_golden as MG
    torch.set_num_threads(1)
    pre = preprocessor("cpu")
    imgs = crops(64)
    codes, params = pre.plan(n_images, 32, 128)
    mean = np.asarray(MEAN, dtype=np.float32).reshape(3, 1, 1)
    std = np.asarray(STD, dtype=np.float32).reshape(3, 1, 1)
    t0 = time.perf_counter()
    for i in range(n_images):
        im = np.asarray(Image.fromarray(imgs[i % 64]).resize((128, 32), Image.BILINEAR))
        ops_ = [(1 if c == 3 else c, p) for c, p in zip(codes[i], params[i]) if c != 0]   # (cv2's rotation: see the note)
        if ops_:
            im = MG.pillow_apply(im[:, :, ::-1], ops_)[:, :, ::-1]          # TorchVisionWrapper's BGR -> RGB -> BGR
        t = (im.transpose(2, 0, 1).astype(np.float32) / 255 - mean) / std
    dt = time.perf_counter() - t0
    assert t.shape == (3, 32, 128)
    cv2 = int((codes == 3).sum())
    print(json.dumps(dict(bench="augment_pillow_cpu", images=n_images, seconds=dt, images_per_s=n_images / dt,
                          note=f"{cv2} cv2 rotations ran as Pillow affines (OpenCV is not installed)")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--backend", default=None, choices=[None, "cv2", "pillow"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pillow-cpu", action="store_true")
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.pillow_cpu:
        return pillow_cpu(a.images)
    import torch
    from tps_pp_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    N, H, W, C = a.batch, 32, 128, 3
    pre = {"b": preprocessor(dev, 0.0, 0.0, a.backend), "c": preprocessor(dev, None, None, a.backend),
           "d": preprocessor(dev, 1.0, 1.0, a.backend)}
    imgs = crops(N)
    _, _, _, interpolation, packed, offs, meta = pre["b"]._prepare(imgs, 0)
    lut = pre["b"]._lut
    plans = {}
    for k, p in pre.items():
        codes, params = p.plan(N, H, W)
        plans[k] = (torch.from_numpy(codes).to(dev), torch.from_numpy(params).to(dev), float((codes != 0).sum()) / N)
    assert plans["b"][2] == 0 and plans["d"][2] == 5

    def resize_with(lib):
        out = torch.empty((N, C, H, W), device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def run():
            rc = lib.tpspp_resize_normalize_fwd(packed.data_ptr(), offs.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
                                                meta[2].data_ptr(), lut.data_ptr(), 0, N, C, H, W, out.data_ptr(),
                                                interpolation, stream)
            assert rc == 0, rc
        return run, out

    def augment(k):
        """The entry point itself, like (a): no wrapper, the output allocated once."""
        out = torch.empty((N, C, H, W), device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev).cuda_stream
        L = _lib.lib()
        codes, params = plans[k][0], plans[k][1]

        def run():
            rc = L.tpspp_augment_normalize_fwd(packed.data_ptr(), offs.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
                                               meta[2].data_ptr(), lut.data_ptr(), 0, N, C, H, W, out.data_ptr(),
                                               interpolation, codes.data_ptr(), params.data_ptr(), codes.shape[1], 1, stream)
            assert rc == 0, rc
        return run, out
    run_a, out_a = resize_with(_lib.lib())
    variants = {"(a) resize_normalize": run_a}
    if a.parent_lib:
        other = ctypes.CDLL(os.path.abspath(a.parent_lib))
        other.tpspp_resize_normalize_fwd.argtypes = _lib._SIGNATURES["tpspp.h"]["tpspp_resize_normalize_fwd"][0]
        other.tpspp_resize_normalize_fwd.restype = ctypes.c_int
        run_p, out_p = resize_with(other)
        variants[f"(a) resize_normalize, {os.path.basename(os.path.dirname(os.path.abspath(a.parent_lib)))}"] = run_p
    run_b, out_b = augment("b")
    variants.update({"(b) augment, empty lists": run_b, "(c) augment, config probabilities": augment("c")[0],
                     "(d) augment, 1 geometric + 4 colour ops": augment("d")[0]})
    for f in variants.values():                                # warm-up: code objects, the allocator's blocks
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    if a.parent_lib:
        assert torch.equal(out_a, out_p), "the two builds of tpspp_resize_normalize_fwd disagree"
    assert torch.equal(out_b, out_a), "empty op lists do not give resize_normalize's bits"

    def region(f):
        """(GPU ms per call between two events, host ms per call spent enqueueing)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.reps):
            f()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps, (t1 - t0) * 1e3 / a.reps
    ms, enq = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(a.regions):
        for k, f in variants.items():
            g, h = region(f)
            ms[k].append(g)
            enq[k].append(h)
    table = []
    for k, v in ms.items():
        row = dict(variant=k, ms=statistics.median(v), ms_min=min(v), ms_max=max(v), images_per_s=N / statistics.median(v) * 1e3,
                   host_enqueue_ms=statistics.median(enq[k]))
        table.append(row)
        print(f"{k:46s} {row['ms'] * 1e3:8.1f} us / batch (min {row['ms_min'] * 1e3:.1f} max {row['ms_max'] * 1e3:.1f})  "
              f"{row['images_per_s'] / 1e6:.2f} M img/s; host enqueue {row['host_enqueue_ms'] * 1e3:.1f} us", flush=True)
    host = []
    for _ in range(a.regions):
        t0 = time.perf_counter()
        pre["c"].plan(N, H, W)
        host.append((time.perf_counter() - t0) * 1e3)
    by = {r["variant"][:3]: r for r in reversed(table)}       # (a): this build's row, the first of the table
    result = dict(bench="augment", batch=N, backend=a.backend or "cv2", reps=a.reps, regions=a.regions, table=table,
                  ops_per_image={k: plans[k][2] for k in plans}, plan_host_ms=statistics.median(host),
                  b_over_a=by["(b)"]["ms"] / by["(a)"]["ms"],
                  a_spread=(by["(a)"]["ms_max"] - by["(a)"]["ms_min"]) / by["(a)"]["ms"])
    print(f"host: a batch's plan {result['plan_host_ms']:.3f} ms; (b) / (a) = {result['b_over_a']:.3f}, spread of (a) "
          f"{100 * result['a_spread']:.1f} %; ops per image in (c): {plans['c'][2]:.2f}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
