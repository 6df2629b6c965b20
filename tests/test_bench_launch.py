"""`python bench.py --gpus N` as typed (no launcher): the parent starts the ranks itself, never touches a GPU, passes
rank 0's single JSON line through and returns the children's exit status.  Checked here on CPU with `--dry-run`
(gloo process group, barrier, all-gather of per-rank rows, max-over-ranks reduction; no kernels)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


def test_self_launch_two_ranks_prints_one_json_line():
    r = run_bench("--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["dry_run"] is True and rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["gathered_rows"] == 6 and rec["gather_ok"] is True


def test_single_rank_needs_no_launcher_and_a_failing_child_fails_the_parent():
    r = run_bench("--dry-run")
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["n_gpus"] == 1
    # a rank that dies makes the parent exit non-zero: without a GPU the real (non dry-run) ranks refuse to start
    r = run_bench("--gpus", "2", "--steps", "1", "--warmup", "0", "--no-extras", "--no-cpu-baseline")
    assert r.returncode != 0


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_and_dumps_the_last_output(cuda, oracle, tmp_path):
    """A plain run (no --full): one JSON line with the headline keys for exactly `--steps` timed steps, nothing of the
    --full measurements, and DIR/rectified.npy = the output batch of the last timed step.  --warmup 1 and --steps = the
    number of rotating buffer sets put that step on buffer set 0, whose inputs are the reproducible synthetic ones: the
    dump is checked bit for bit against the CPU oracle on them."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from tps_pp_amd import TPSPreprocessor, constants, synth
    per_set = 2 * bench.BATCH * bench.C * bench.H * bench.W * 4
    nbuf = max(2, (2 * bench.CACHE_BYTES + per_set - 1) // per_set)
    out_dir = tmp_path / "dump"
    r = run_bench("--gpus", "1", "--steps", str(nbuf), "--warmup", "1", "--dump-outputs", str(out_dir))
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["config"]["rotating_buffer_sets"] == nbuf
    assert rec["steps"] == nbuf and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["metric"] == "rectified images/sec (3x32x100)" and rec["unit"] == "images/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] * 1e-3 - bench.BATCH) < 1e-6 * bench.BATCH
    assert "extra" not in rec and "cpu_baseline" not in rec
    got = np.load(out_dir / "rectified.npy")
    assert got.dtype == np.float32 and got.shape == (bench.BATCH, bench.C, bench.H, bench.W)
    gg = TPSPreprocessor(bench.F, (bench.H, bench.W), (bench.H, bench.W), bench.C).GridGenerator
    img0 = synth.dyadic(got.shape, "bench.img.r0")
    ctrl0 = (constants.classic_identity_ctrl(bench.F)[None]
             + 0.05 * synth.dyadic((bench.BATCH, bench.F, 2), "bench.ctrl.r0")).astype(np.float32)
    want = oracle.warp(img0, ctrl0, gg.inv_delta_C.numpy(), gg.P_hat.numpy(), (bench.H, bench.W))["out0"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
