"""Host-side checks (no GPU) of the bf16 warp backward (TPSPP_IO_BF16 of tpspp_warp_bwd): the module switches, the dtype gate
of `ops.warp_backward`, which raises before any library call, and the argument checks of the entry point, which come before
any device work (the served / refused geometries included: they are decided before the N == 0 return)."""
import pytest
import torch

from tps_pp_amd import TPS_PP, _lib, ops
from tps_pp_amd.nrtr_head import EncodeDecodeRecognizer
from tps_pp_amd.tps_preprocessor import TPSPreprocessor


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.mark.parametrize("make", [lambda: TPS_PP(), lambda: TPSPreprocessor(20, (32, 100), (32, 100), 3)],
                         ids=["TPS_PP", "TPSPreprocessor"])
def test_setter_exists_returns_self_and_defaults_to_none(make):
    m = make()
    assert m.train_io_dtype is None
    assert m.set_train_io_dtype(torch.bfloat16) is m and m.train_io_dtype == torch.bfloat16
    for bad in (torch.float16, torch.float32, "bf16", 16):
        with pytest.raises(ValueError):
            m.set_train_io_dtype(bad)
    assert m.train_io_dtype == torch.bfloat16                          # a refused value changes nothing
    assert m.set_train_io_dtype(None) is m and m.train_io_dtype is None


class _Part(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.train_io_dtype = None

    def set_train_io_dtype(self, dtype):
        self.train_io_dtype = dtype
        return self


def test_recognizer_forwards_the_setting_to_the_rectifier_it_owns():
    for owned in ("tpsnet", "preprocessor"):
        r = EncodeDecodeRecognizer.__new__(EncodeDecodeRecognizer)
        torch.nn.Module.__init__(r)
        r.tpsnet = r.preprocessor = None
        part = _Part()
        setattr(r, owned, part)
        assert r.set_train_io_dtype(torch.bfloat16) is r and part.train_io_dtype == torch.bfloat16
        assert r.set_train_io_dtype(None) is r and part.train_io_dtype is None
    r = EncodeDecodeRecognizer.__new__(EncodeDecodeRecognizer)
    torch.nn.Module.__init__(r)
    r.tpsnet = r.preprocessor = None
    with pytest.raises(ValueError):
        r.set_train_io_dtype(torch.bfloat16)
    r.tpsnet = TPS_PP()                                                # the real module
    assert r.set_train_io_dtype(torch.bfloat16).tpsnet.train_io_dtype == torch.bfloat16


def test_warp_backward_mixed_dtypes_raise_before_any_library_call(monkeypatch):
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} reached")
    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    f32 = lambda *s: torch.zeros(s)                                             # noqa: E731
    b16 = lambda *s: torch.zeros(s, dtype=torch.bfloat16)                       # noqa: E731
    grid, ctrl, inv, P_hat = f32(2, 3200, 2), f32(2, 20, 2), f32(23, 23), f32(3200, 23)
    img = (2, 3, 32, 100)
    for g0, in0 in ((b16(*img), f32(*img)), (f32(*img), b16(*img))):
        with pytest.raises(TypeError, match="share their dtype"):
            ops.warp_backward(g0, in0, grid, ctrl, inv, P_hat, (32, 100))
    with pytest.raises(TypeError, match="share their dtype"):                      # in1 differs
        ops.warp_backward(b16(*img), b16(*img), grid, ctrl, inv, P_hat, (32, 100), in1=f32(*img), g_out1=b16(*img))
    with pytest.raises(TypeError, match="share their dtype"):                      # g_out1 differs
        ops.warp_backward(b16(*img), b16(*img), grid, ctrl, inv, P_hat, (32, 100), in1=b16(*img), g_out1=f32(*img))
    # all bf16 (or all fp32) passes the dtype gate: on CPU tensors the device check is what raises
    for mk in (b16, f32):
        with pytest.raises(_lib.TpsppError, match="GPU tensor"):
            ops.warp_backward(mk(*img), mk(*img), grid, ctrl, inv, P_hat, (32, 100))


def _bwd(lib, flags, N=0, H0=32, W0=100, Ho=32, Wo=100, in0=16, g_out0=16, g_in0=16, ws=16, ws_floats=0, C0=3):
    """tpspp_warp_bwd on stand-in pointers (for N = 0 they are only compared with NULL and looked at for their alignment)."""
    return lib.tpspp_warp_bwd(g_out0, in0, C0, H0, W0, None, None, 0, 0, 0, 16, None, 16, 16, 23, None, None, None, flags,
                              N, 20, Ho, Wo, g_in0, None, 16, None, ws, ws_floats, None)


def test_empty_bf16_batch_returns_ok(lib):
    for flags in (ops.IO_BF16, ops.IO_BF16 | ops.BWD_FIXED_POINT, ops.IO_BF16 | ops.BWD_TWO_KERNELS):
        assert _bwd(lib, flags) == 0, lib.tpspp_last_error()
    assert _bwd(lib, ops.IO_BF16, H0=16, W0=64, Ho=16, Wo=64, C0=64) == 0, lib.tpspp_last_error()


def test_argument_errors_with_the_bit_come_back_without_a_device(lib):
    assert _bwd(lib, ops.IO_BF16, in0=None) == -22 and "null pointer" in lib.tpspp_last_error().decode()
    assert _bwd(lib, ops.IO_BF16, ws=None) == -22
    assert _bwd(lib, ops.IO_BF16, N=2, ws_floats=8) == -22 and "g_grid_ws too small" in lib.tpspp_last_error().decode()
    assert _bwd(lib, ops.IO_BF16, C0=0) == -22
    # the geometries the bf16 backward does not serve, each named (decided before the N == 0 return)
    for kw, what in ((dict(H0=64, W0=200, Ho=64, Wo=200), "4096 output pixels"),
                     (dict(H0=96, W0=64, Ho=32, Wo=64), "more than 4096 pixels"),
                     (dict(H0=15, W0=21, Ho=32, Wo=64), "multiple of 8"),
                     (dict(in0=24), "16-byte aligned"), (dict(g_in0=8), "16-byte aligned"),
                     (dict(g_out0=17), "2-byte aligned")):
        assert _bwd(lib, ops.IO_BF16, **kw) == -22
        msg = lib.tpspp_last_error().decode()
        assert "TPSPP_IO_BF16" in msg and what in msg, msg
        assert _bwd(lib, 0, **kw) == 0, lib.tpspp_last_error()          # (fp32: every one of these is served)


def test_backbone_training_blocks_widen_a_bf16_rectifier_output():
    """`TPS_PP.set_train_io_dtype(torch.bfloat16)` hands the backbone a bf16 `output`: its training blocks (fp32 parameters)
    widen it, and its gradient comes back bf16.  The PyTorch composition on the CPU, a stand-in rectifier."""
    from tps_pp_amd.resnet_v2_large import ResNetABI_v2_large
    torch.manual_seed(0)
    bb = ResNetABI_v2_large(arch_settings=[1, 1, 1, 1, 1], strides=[2, 1, 2, 1, 2]).train()
    seen = {}

    def rectifier(x, outs, **kw):
        seen["out"] = x.to(torch.bfloat16)
        seen["out"].retain_grad()
        return {"output": seen["out"]}
    res = bb._forward_torch(torch.randn(2, 3, 32, 128), rectifier)
    assert res["output"].dtype == torch.float32 and res["img_ref"].dtype == torch.bfloat16
    res["output"].square().mean().backward()
    assert seen["out"].grad.dtype == torch.bfloat16 and seen["out"].grad.float().abs().max() > 0
