"""CPU tests of the convolution backward's boundary (tpspp_conv2d_bwd_data / _bwd_weight / _bwd_weight_workspace_floats)
and of the training-backend switch: argument errors come back as -22 with a message before anything is launched, the
workspace query follows the sizes, and the switch leaves the module's state alone."""
import ctypes

import pytest
import torch

from tps_pp_amd import TPS_PP, _lib, build, ops

FAKE = 0x1000          # never dereferenced: every call here fails its checks before a launch (or returns for N = 0)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def dims(*srcs):
    flat = [v for s in srcs for v in s]
    return ctypes.cast((ctypes.c_int * len(flat))(*flat), ctypes.c_void_p)


def ptrs(*vals):
    return ctypes.cast((ctypes.c_void_p * len(vals))(*vals), ctypes.c_void_p)


def bwd_data(lib, dsrc, d, nsrc, weight=FAKE, dy=FAKE, y=FAKE, relu=1, N=2, Cout=64, K=3, sh=1, sw=1, Ho=16, Wo=64):
    return lib.tpspp_conv2d_bwd_data(dsrc, d, nsrc, weight, dy, y, relu, N, Cout, K, K, sh, sw, Ho, Wo, None)


def bwd_weight(lib, src, d, nsrc, ws_floats, ws=FAKE, N=2, Cout=64, K=3, sh=1, sw=1, Ho=16, Wo=64, dw=FAKE, db=FAKE,
               dy=FAKE, y=FAKE, relu=1):
    return lib.tpspp_conv2d_bwd_weight(src, d, nsrc, dy, y, relu, N, Cout, K, K, sh, sw, Ho, Wo, dw, db, ws, ws_floats,
                                       None)


def err(lib):
    return lib.tpspp_last_error().decode()


def test_data_gradient_argument_errors(lib):
    d = dims((64, 16, 64, 1, 1))
    assert bwd_data(lib, None, d, 1) == -22 and "null pointer" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), d, 1, weight=None) == -22 and "null pointer" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), d, 1, dy=None) == -22 and "null pointer" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), d, 1, y=None) == -22 and "mask" in err(lib)
    assert bwd_data(lib, ptrs(None), d, 1) == -22 and "no source gradient" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), None, 1) == -22 and "null pointer" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), d, 1, sh=3, Ho=6) == -22 and "stride" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), d, 1, K=5) == -22 and "kernel" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), d, 1, Ho=15) == -22 and "output size" in err(lib)
    assert bwd_data(lib, ptrs(FAKE), d, 1, relu=2) == -22 and "activation" in err(lib)
    assert bwd_data(lib, ptrs(FAKE, FAKE), dims((64, 16, 64, 1, 1), (64, 8, 64, 1, 1)), 2) == -22 \
        and "logical size" in err(lib)
    # relu = 0 does not need y; N = 0 returns before any launch
    assert bwd_data(lib, ptrs(FAKE), d, 1, y=None, relu=0, N=0) == 0


def test_weight_gradient_argument_errors(lib):
    d = dims((64, 16, 64, 1, 1))
    need = lib.tpspp_conv2d_bwd_weight_workspace_floats(d, 1, 2, 64, 3, 3, 16, 64)
    assert need > 0
    assert bwd_weight(lib, None, d, 1, need) == -22 and "null pointer" in err(lib)
    assert bwd_weight(lib, ptrs(None), d, 1, need) == -22 and "null pointer" in err(lib)
    assert bwd_weight(lib, ptrs(FAKE), d, 1, need, dw=None, db=None) == -22 and "null pointer" in err(lib)
    assert bwd_weight(lib, ptrs(FAKE), d, 1, need, dy=None) == -22 and "null pointer" in err(lib)
    assert bwd_weight(lib, ptrs(FAKE), d, 1, need, sw=0, Wo=64) == -22 and "stride" in err(lib)
    assert bwd_weight(lib, ptrs(FAKE), d, 1, need, K=2) == -22 and "kernel" in err(lib)
    assert bwd_weight(lib, ptrs(FAKE), d, 1, need - 1) == -22 and "ws too small" in err(lib)
    assert bwd_weight(lib, ptrs(FAKE), d, 1, need, ws=None) == -22 and "ws too small" in err(lib)
    # N = 0: no workspace needed, nothing launched
    assert bwd_weight(lib, ptrs(FAKE), d, 1, 0, ws=None, N=0) == 0


def test_workspace_query_follows_the_sizes(lib):
    d = dims((64, 16, 64, 1, 1), (64, 16, 64, 1, 1), (64, 16, 64, 1, 1))
    q = [lib.tpspp_conv2d_bwd_weight_workspace_floats(d, 3, n, 64, 3, 3, 16, 64) for n in (0, 1, 4, 32, 512)]
    assert q[0] == 0
    assert all(b >= a for a, b in zip(q, q[1:])) and q[-1] > q[1] > 0, q
    # at least the partial dW and db of one slice
    assert q[1] >= 64 * (192 * 9 + 1)
    assert lib.tpspp_conv2d_bwd_weight_workspace_floats(None, 1, 4, 64, 3, 3, 16, 64) == 0


def test_set_train_backend_rejects_unknown_modes():
    m = TPS_PP()
    with pytest.raises(ValueError):
        m.set_train_backend("bogus")
    with pytest.raises(ValueError):
        m.set_train_backend(None)
    assert m.train_backend == "torch"
    assert m.set_train_backend("hip").train_backend == "hip"


def test_set_train_backend_leaves_the_state_dict_alone():
    torch.manual_seed(0)
    m = TPS_PP()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = [id(p) for p in m.parameters()]
    m.set_train_backend("hip")
    after = m.state_dict()
    assert list(before) == list(after)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert [id(p) for p in m.parameters()] == params
    m.set_train_backend("torch")
    assert all(torch.equal(before[k], v) for k, v in m.state_dict().items())


def small_recognizer():
    import tps_pp_amd as P
    return P.build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                            strides=[2, 1, 2, 1, 2]),
                                 tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                                 decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                                 label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
                                 max_seq_len=8))


def test_recognizer_forwards_the_switch():
    r = small_recognizer()
    before = {k: v.clone() for k, v in r.state_dict().items()}
    assert r.tpsnet.train_backend == "torch"
    assert r.set_train_backend("hip") is r and r.tpsnet.train_backend == "hip"
    with pytest.raises(ValueError):
        r.set_train_backend("miopen")
    assert r.tpsnet.train_backend == "hip"
    assert all(torch.equal(before[k], v) for k, v in r.state_dict().items())


def test_conv2d_autograd_refuses_cpu_tensors():
    x = torch.randn(1, 8, 6, 6, requires_grad=True)
    w = torch.randn(4, 8, 3, 3, requires_grad=True)
    b = torch.randn(4, requires_grad=True)
    with pytest.raises(_lib.TpsppError):
        ops.conv2d_autograd([x], w, b, 1, relu=True)
    with pytest.raises(_lib.TpsppError):
        ops.conv2d_autograd([(x, 2, 2)], w, None, (2, 1), relu=False)
    with pytest.raises(_lib.TpsppError):
        ops.conv2d_bwd_data(torch.zeros(1, 4, 6, 6), w, [x], 1, relu=False)
