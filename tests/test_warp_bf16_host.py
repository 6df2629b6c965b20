"""Host-side checks (no GPU) of the bf16 classic rectifier: the module switch, the ABI number, the empty batch and the
argument checks of a bf16 `ops.WarpPlan`, which raise before any library call."""
import pytest
import torch

from tps_pp_amd import _lib, ops
from tps_pp_amd.tps_preprocessor import TPSPreprocessor


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_set_compute_dtype_accepts_three_modes_and_sets_the_localisation_network():
    m = TPSPreprocessor(num_fiducial=20, img_size=(32, 100), rectified_img_size=(32, 100), num_img_channel=3).eval()
    assert getattr(m, "io_dtype", None) is None                       # unset: forward is what it was
    assert m.set_compute_dtype(torch.bfloat16) is m
    assert m.io_dtype == torch.bfloat16 and m.LocalizationNetwork.compute_dtype == torch.bfloat16
    m.set_compute_dtype("bf16x3")                                     # the localisation network only
    assert m.io_dtype is None and m.LocalizationNetwork.compute_dtype == "bf16x3"
    m.set_compute_dtype(None)
    assert m.io_dtype is None and m.LocalizationNetwork.compute_dtype is None
    for bad in ("fp16", torch.float16, "bf16", 16):
        with pytest.raises(ValueError):
            m.set_compute_dtype(bad)
    assert m.io_dtype is None and m.LocalizationNetwork.compute_dtype is None      # a refused mode changes nothing


def test_abi_version_is_12(lib):
    assert _lib.ABI_VERSION == lib.tpspp_abi_version() == 12


def test_empty_bf16_classic_batch_returns_ok(lib):
    flags = ops.IO_BF16 | ops.TABLE_MIRROR4 | ops.TABLE_PACKED
    # (pointers are only compared with NULL for N = 0)
    rc = lib.tpspp_warp_fwd(16, 3, 32, 100, None, 0, 0, 0, 16, None, 16, 16, 23, None, 16, flags, 0, 20, 32, 100,
                            16, None, None, None, None)
    assert rc == 0, lib.tpspp_last_error()


def test_warp_plan_mixed_dtypes_raise_before_any_library_call(monkeypatch):
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} reached")
    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    f32 = lambda *s: torch.zeros(s)                                             # noqa: E731
    b16 = lambda *s: torch.zeros(s, dtype=torch.bfloat16)                       # noqa: E731
    ctrl, inv, P_hat = f32(2, 20, 2), f32(23, 23), f32(3200, 23)
    img = (2, 3, 32, 100)
    for in0, out0 in ((b16(*img), f32(*img)), (f32(*img), b16(*img))):
        with pytest.raises(TypeError, match="share their dtype"):
            ops.WarpPlan(in0, ctrl, inv, P_hat, (32, 100), out0)
    with pytest.raises(TypeError, match="share their dtype"):                      # in0 / in1 differ
        ops.WarpPlan(b16(*img), ctrl, inv, P_hat, (32, 100), b16(*img), in1=f32(*img), out1=b16(*img))
    with pytest.raises(TypeError, match="share their dtype"):                      # out1 differs
        ops.WarpPlan(b16(*img), ctrl, inv, P_hat, (32, 100), b16(*img), in1=b16(*img), out1=f32(*img))
    # all bf16 (or all fp32) passes the dtype gate: on CPU tensors the device check is what raises
    for mk in (b16, f32):
        with pytest.raises(_lib.TpsppError, match="GPU tensor"):
            ops.WarpPlan(mk(*img), ctrl, inv, P_hat, (32, 100), mk(*img))
