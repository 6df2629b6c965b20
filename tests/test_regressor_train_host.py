"""CPU tests of the "hip_all" train backend (every layer of the TPS_PP control-point regressor on HIP kernels in the
training graph): the switch on TPS_PP and the recogniser, and the workspace queries of tpspp_regressor_bwd.hip.  No GPU."""
import pytest
import torch

from tps_pp_amd import TPS_PP, _lib, build, ops
from test_conv_bwd_host import small_recognizer


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def test_tps_pp_accepts_hip_all():
    m = TPS_PP()
    assert m.set_train_backend("hip_all") is m and m.train_backend == "hip_all"
    assert m.set_train_backend("hip").train_backend == "hip"
    assert m.set_train_backend("torch").train_backend == "torch"


@pytest.mark.parametrize("mode", ["bogus", None, "HIP_ALL", "hip-all", "all"])
def test_unknown_modes_still_raise(mode):
    m = TPS_PP().set_train_backend("hip_all")
    with pytest.raises(ValueError):
        m.set_train_backend(mode)
    assert m.train_backend == "hip_all"


@pytest.mark.parametrize("variant", ["ResNet45v2", "ResNet45"])
def test_state_dict_unchanged_by_switching(variant):
    torch.manual_seed(0)
    m = TPS_PP(variant=variant)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = [id(p) for p in m.parameters()]
    for mode in ("hip_all", "hip", "hip_all", "torch"):
        m.set_train_backend(mode)
        after = m.state_dict()
        assert list(before) == list(after)
        assert all(torch.equal(before[k], after[k]) for k in before)
        assert [id(p) for p in m.parameters()] == params


def test_recognizer_forwards_hip_all():
    r = small_recognizer()
    before = {k: v.clone() for k, v in r.state_dict().items()}
    assert r.set_train_backend("hip_all") is r and r.tpsnet.train_backend == "hip_all"
    with pytest.raises(ValueError):
        r.set_train_backend("hip_some")
    assert r.tpsnet.train_backend == "hip_all"
    assert all(torch.equal(before[k], v) for k, v in r.state_dict().items())


def test_hip_all_refuses_cpu_tensors():
    m = TPS_PP()
    x = torch.randn(1, 64, 2, 16)
    with pytest.raises(_lib.TpsppError):
        ops.cbam_autograd(x, m.MSFA.conv.atten)
    with pytest.raises(_lib.TpsppError):
        ops.tpe_points_autograd(x, m.TPE)
    with pytest.raises(_lib.TpsppError):
        ops.score_autograd(torch.randn(1, 64, 16, 64), x, m.TPE)
    with pytest.raises(_lib.TpsppError):
        ops.dgab_autograd(torch.randn(1, 64, 16, 64), x.reshape(1, 64, 32), m.TPE.atten[0])


def _slices(M, min_rows):
    L = max(min_rows, -(-M // 512))
    L = -(-L // 16) * 16
    return -(-M // L)


def test_linear_bwd_weight_workspace_sizes(lib):
    """S * O * (K + 1), S = ceil(M / L), L = max(256, ceil(M / 512)) rounded up to 16 (include/tpspp.h)."""
    q = lib.tpspp_linear_bwd_weight_workspace_floats
    # DGAB's fc1 at batch 512: 512 * 64 * 16 rows -> 512 slices of 1024
    assert q(512 * 64 * 16, 256, 64) == 512 * 256 * 65
    assert _slices(512 * 64 * 16, 256) == 512
    # localization fc2: one row per image, a single slice up to 256 images
    assert q(4, 64, 64) == 1 * 64 * 65
    assert q(257, 64, 64) == 2 * 64 * 65
    # the score's p_linear at batch 3
    assert q(3 * 32, 32, 64) == 32 * 65
    for M, O, K in ((1, 2, 256), (1000, 17, 48), (10 ** 6, 65, 96), (4096 * 1024, 128, 32)):
        assert q(M, O, K) == _slices(M, 256) * O * (K + 1), (M, O, K)
    assert q(0, 64, 64) == 0 and q(10, 0, 64) == 0 and q(10, 64, 0) == 0 and q(-1, 64, 64) == 0
    assert ops.linear_bwd_weight_workspace_floats(512 * 1024, 128, 32) == q(512 * 1024, 128, 32)


def test_plane_ln_and_cbam_workspace_sizes(lib):
    q = lib.tpspp_plane_ln_bwd_workspace_floats
    assert q(512 * 64, 1024) == 512 * 2 * 1024            # 32768 planes: 512 slices of 64
    assert q(3 * 64, 1024) == 12 * 2 * 1024               # 192 planes: 12 slices of 16
    assert q(1, 1024) == 2 * 1024
    for rows in (1, 15, 16, 17, 8191, 10 ** 6):
        assert q(rows, 1024) == _slices(rows, 16) * 2 * 1024, rows
    assert q(0, 1024) == 0 and q(5, 0) == 0
    c = lib.tpspp_cbam_bwd_workspace_floats
    assert c(512, 64, 4) == 512 * (2 * 64 * 4 + 19)
    assert c(1, 64, 4) == 2 * 64 * 4 + 19
    assert c(0, 64, 4) == 0 and c(3, 0, 4) == 0
    assert ops.cbam_bwd_workspace_floats(3, 64, 4) == 3 * 531
    assert ops.plane_ln_bwd_workspace_floats(3 * 64, 1024) == q(3 * 64, 1024)


def test_argument_errors_come_back_as_codes(lib):
    """No launch happens here: every call fails its argument checks first (or has nothing to do)."""
    import ctypes
    a = (ctypes.c_longlong * 3)(0, 1, 1)
    vp = ctypes.cast(a, ctypes.c_void_p)
    assert lib.tpspp_mm_f32(1, 4, 4, 4, None, vp, None, vp, None, vp, None, None, 0, 1.0, 0, None) == -22
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tpspp_mm_f32(1, 4, 4, 4, p, vp, p, vp, p, vp, None, None, 7, 1.0, 0, None) == -22
    assert b"epilogue" in lib.tpspp_last_error()
    assert lib.tpspp_mm_f32(0, 4, 4, 4, p, vp, p, vp, p, vp, None, None, 0, 1.0, 0, None) == 0      # empty batch
    assert lib.tpspp_linear_bwd_weight(p, p, vp, 0, 1000, 64, 64, p, p, p, 10, None) == -22
    assert b"ws too small" in lib.tpspp_last_error()
    assert lib.tpspp_linear_bwd_weight(p, p, vp, 1, 1000, 64, 64, p, p, p, 10 ** 6, None) == -22
    assert b"x_act" in lib.tpspp_last_error()
    assert lib.tpspp_act_bwd(5, 4, p, p, 1.0, p, None) == -22
    assert lib.tpspp_dgab_gate_fwd(p, p, p, 1, 64, 128, 64, p, None) == -22                          # H * W > 4096
    assert lib.tpspp_cbam_train_fwd(p, p, p, p, p, 1, 64, 4, 16, 64, p, p, p, None) == -22          # C * H * W > 4096
    assert lib.tpspp_cbam_bwd(p, p, p, p, p, p, 2, 64, 4, 2, 16, p, p, p, p, p, p, 100, None) == -22
    assert b"ws too small" in lib.tpspp_last_error()
    assert lib.tpspp_plane_ln_bwd(p, p, p, p, p, 64, 1024, p, 2, None, None, None, 0, None) == -22
