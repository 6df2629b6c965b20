"""CPU tests of the backbone's "hip" train backend (ResNetABI_v2_large's stem and BasicBlocks on the HIP kernels of
tpspp_bn_train.hip and the convolution kernels in the training graph): the switch on the backbone and the recogniser, the
workspace queries and the argument checks of the BatchNorm entry points.  No GPU: nothing is launched here."""
import ctypes

import pytest
import torch
import torch.nn as nn

from tps_pp_amd import ResNetABI_v2_large, _lib, build, ops
from test_conv_bwd_host import small_recognizer


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def small_backbone():
    torch.manual_seed(0)
    return ResNetABI_v2_large(arch_settings=[1, 1, 1, 1, 1], strides=[2, 1, 2, 1, 2])


def test_backbone_switch():
    m = small_backbone()
    assert m.train_backend == "torch"
    assert m.set_train_backend("hip") is m and m.train_backend == "hip"
    assert m.set_train_backend("torch") is m and m.train_backend == "torch"


@pytest.mark.parametrize("mode", ["bogus", None, "HIP", "hip_all", "cuda"])
def test_backbone_rejects_unknown_modes(mode):
    m = small_backbone().set_train_backend("hip")
    with pytest.raises(ValueError):
        m.set_train_backend(mode)
    assert m.train_backend == "hip"


def test_switching_leaves_the_state_dict_alone():
    m = small_backbone()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = [id(p) for p in m.parameters()]
    for mode in ("hip", "torch", "hip"):
        m.set_train_backend(mode)
        after = m.state_dict()
        assert list(before) == list(after)
        assert all(torch.equal(before[k], after[k]) for k in before)
        assert [id(p) for p in m.parameters()] == params


def test_recognizer_switch_keeps_the_backbone_by_default():
    r = small_recognizer()
    before = {k: v.clone() for k, v in r.state_dict().items()}
    r.set_train_backend("hip")
    assert r.tpsnet.train_backend == "hip" and r.backbone.train_backend == "torch"
    assert r.set_train_backend("hip_all", backbone="hip") is r
    assert r.tpsnet.train_backend == "hip_all" and r.backbone.train_backend == "hip"
    r.set_train_backend("torch")
    assert r.tpsnet.train_backend == "torch" and r.backbone.train_backend == "hip"
    r.set_train_backend("hip", backbone="torch")
    assert r.tpsnet.train_backend == "hip" and r.backbone.train_backend == "torch"
    with pytest.raises(ValueError):
        r.set_train_backend("hip_all", backbone="hip_all")
    assert r.tpsnet.train_backend == "hip" and r.backbone.train_backend == "torch"      # nothing changed
    assert all(torch.equal(before[k], v) for k, v in r.state_dict().items())


def test_cache_invalidation_is_available():
    from tps_pp_amd._prepared import prepared
    m = small_backbone()
    builds = []
    slot = lambda: prepared(m, ("train", "conv1"), [m.conv1.weight], lambda: builds.append(1))      # noqa: E731
    slot(), slot()
    assert len(builds) == 1
    assert m.invalidate_train_cache() is m and not any("_tpspp_prepared" in x.__dict__ for x in m.modules())
    slot()
    assert len(builds) == 2                 # nothing was left cached: the next use rebuilds


def _slices(M):
    return -(-M // 4096)


def test_workspace_sizes_follow_the_sizes_alone(lib):
    """S * C * 3, S = ceil(N*H*W / 4096) (include/tpspp.h)."""
    for q in (lib.tpspp_bn_stats_workspace_floats, lib.tpspp_bn_bwd_reduce_workspace_floats):
        assert q(512, 32, 32 * 128) == 512 * 32 * 3           # the stem at batch 512: 2^21 values per channel
        assert q(512, 512, 4 * 16) == 8 * 512 * 3             # the last stage
        assert q(1, 64, 7 * 9) == 64 * 3 and q(3, 64, 4097) == 4 * 64 * 3
        for N, C, HW in ((1, 1, 1), (3, 32, 1365), (8, 256, 8 * 32), (2, 5, 4096), (5, 7, 4095)):
            assert q(N, C, HW) == _slices(N * HW) * C * 3, (N, C, HW)
        assert q(0, 32, 64) == 0 and q(4, 0, 64) == 0 and q(4, 32, 0) == 0 and q(-1, 32, 64) == 0
    assert ops.bn_stats_workspace_floats(3, 64, 4097) == 4 * 64 * 3
    assert ops.bn_bwd_reduce_workspace_floats(3, 64, 4097) == 4 * 64 * 3


def test_argument_errors_come_back_as_codes(lib):
    """Every call fails its argument checks before it launches anything."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nbt = (ctypes.c_longlong * 1)()
    q = ctypes.cast(nbt, ctypes.c_void_p)
    err = lib.tpspp_last_error
    # statistics
    assert lib.tpspp_bn_train_stats(None, 2, 4, 16, 1e-5, 0.1, None, None, None, p, p, p, 1000, None) == -22
    assert b"null pointer" in err()
    assert lib.tpspp_bn_train_stats(p, 2, 4, 16, 1e-5, 0.1, None, None, None, p, p, p, 3, None) == -22
    assert b"ws too small" in err()
    assert lib.tpspp_bn_train_stats(p, 0, 4, 16, 1e-5, 0.1, None, None, None, p, p, p, 1000, None) == -22
    assert b"empty batch" in err()
    assert lib.tpspp_bn_train_stats(p, 1, 4, 1, 1e-5, 0.1, None, p, p, p, p, p, 1000, None) == -22
    assert b"more than 1 value" in err()
    assert lib.tpspp_bn_train_stats(p, 2, 4, 16, 1e-5, -1.0, None, p, p, p, p, p, 1000, None) == -22
    assert b"num_batches_tracked" in err()
    assert lib.tpspp_bn_train_stats(p, 2, 4, 16, 1e-5, 0.1, q, p, None, p, p, p, 1000, None) == -22
    assert lib.tpspp_bn_train_stats(p, 2, 0, 16, 1e-5, 0.1, None, None, None, p, p, p, 1000, None) == -22
    assert lib.tpspp_bn_train_stats(p, 2, 4, 16, -1.0, 0.1, None, None, None, p, p, p, 1000, None) == -22
    assert lib.tpspp_bn_train_stats(p, 2, 4, 16, 1e-5, 2.0, None, None, None, p, p, p, 1000, None) == -22
    assert lib.tpspp_bn_train_stats(p, 1 << 16, 64, 1 << 16, 1e-5, 0.1, None, None, None, p, p, p, 10 ** 12, None) == -22
    assert b"2^31" in err()
    assert lib.tpspp_bn_eval_stats(p, None, 4, 1e-5, p, p, None) == -22
    assert lib.tpspp_bn_eval_stats(p, p, 0, 1e-5, p, p, None) == -22
    # apply
    assert lib.tpspp_bn_apply_fwd(p, p, p, p, p, 3, None, None, None, None, None, None, 1, 2, 4, 16, p, None) == -22
    assert b"res_mode" in err()
    assert lib.tpspp_bn_apply_fwd(p, p, p, p, p, 1, None, None, None, None, None, None, 1, 2, 4, 16, p, None) == -22
    assert b"residual" in err()
    assert lib.tpspp_bn_apply_fwd(p, p, p, p, p, 2, None, p, p, None, p, p, 1, 2, 4, 16, p, None) == -22
    assert b"branch b" in err()
    assert lib.tpspp_bn_apply_fwd(p, p, p, p, p, 0, None, None, None, None, None, None, 2, 2, 4, 16, p, None) == -22
    assert lib.tpspp_bn_apply_fwd(p, p, p, p, None, 0, None, None, None, None, None, None, 1, 2, 4, 16, p, None) == -22
    assert lib.tpspp_bn_apply_fwd(p, p, p, p, p, 0, None, None, None, None, None, None, 1, 0, 4, 16, p, None) == 0  # N = 0
    # backward reduction
    assert lib.tpspp_bn_bwd_reduce(p, None, 1, p, p, p, None, None, None, 2, 4, 16, p, p, None, p, 1000, None) == -22
    assert b"y > 0" in err()
    assert lib.tpspp_bn_bwd_reduce(p, p, 1, p, p, p, None, None, None, 2, 4, 16, p, p, None, p, 3, None) == -22
    assert b"ws too small" in err()
    assert lib.tpspp_bn_bwd_reduce(p, p, 1, p, p, p, p, p, p, 2, 4, 16, p, p, None, p, 1000, None) == -22
    assert lib.tpspp_bn_bwd_reduce(p, p, 1, p, p, p, None, None, None, 2, 4, 16, p, p, p, p, 1000, None) == -22
    # backward data
    assert lib.tpspp_bn_bwd_data(p, p, 1, None, None, None, None, None, 1, None, None, None, None, None, None, 1, None,
                                 None, None, 0, 2, 4, 16, None) == -22
    assert b"nothing to compute" in err()
    assert lib.tpspp_bn_bwd_data(p, p, 1, p, p, p, p, None, 1, p, None, None, None, None, None, 1, None,
                                 p, None, 0, 2, 4, 16, None) == -22                       # training BN without its sums
    assert b"branch a" in err()
    assert lib.tpspp_bn_bwd_data(p, p, 1, None, None, None, None, None, 1, None, None, None, None, None, None, 1, None,
                                 None, None, 3, 2, 4, 16, None) == -22
    assert lib.tpspp_bn_bwd_data(p, None, 1, None, None, None, None, None, 1, None, None, None, None, None, None, 1, None,
                                 None, p, 2, 2, 4, 16, None) == -22
    assert lib.tpspp_bn_bwd_data(p, p, 1, None, None, None, None, None, 1, None, None, None, None, None, None, 1, None,
                                 None, p, 2, 0, 4, 16, None) == 0                       # N = 0: nothing to do


def test_autograd_functions_refuse_cpu_tensors():
    m = small_backbone()
    x = torch.randn(2, 3, 32, 128)
    with pytest.raises(_lib.TpsppError):
        ops.bn_stem_autograd(x, m.conv1, m.bn1)
    with pytest.raises(_lib.TpsppError):
        ops.bn_block_autograd(torch.randn(2, 32, 32, 128), m.layer1[0])
    with pytest.raises(_lib.TpsppError):
        m.train().set_train_backend("hip")(x)


@pytest.mark.parametrize("what", ["affine", "track_running_stats"])
def test_uncovered_batchnorm_raises_value_error_naming_it(what, monkeypatch):
    """Checked before anything reaches the device: a fake GPU check lets the CPU module get as far as the BN check."""
    m = small_backbone()
    blk = m.layer2[0]
    kw = {what: False}
    blk.bn2 = nn.BatchNorm2d(blk.bn2.num_features, **kw)
    monkeypatch.setattr(ops, "_chk_gpu", lambda who, x: None)
    with pytest.raises(ValueError, match=r"layer2\.0\.bn2"):
        ops.bn_block_autograd(torch.randn(2, 32, 16, 64), blk, name="layer2.0")
    stem_bn = nn.BatchNorm2d(32, **kw)
    with pytest.raises(ValueError, match="bn1"):
        ops.bn_stem_autograd(torch.randn(2, 3, 32, 128), m.conv1, stem_bn, name="bn1")


def test_bwd_data_sums_are_optional_only_for_eval_mode_branches(lib):
    """An eval-mode BatchNorm with frozen gamma and beta runs no reduction: sum_dr / sum_dr_xa = NULL is accepted with
    train_a = 0 (the kernel reads the sums only for a training-mode branch) and refused with train_a = 1.  N = 0: the
    argument checks run, nothing is launched."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.tpspp_last_error
    # eval-mode branch a, no sums
    assert lib.tpspp_bn_bwd_data(p, p, 1, p, p, p, p, None, 0, p, None, None, None, None, None, 1, None,
                                 None, None, 0, 0, 4, 16, None) == 0
    # eval-mode branches a and b, no sums, the shortcut's gradient as well
    assert lib.tpspp_bn_bwd_data(p, p, 1, p, p, p, p, None, 0, p, p, p, p, p, None, 0, p,
                                 None, p, 2, 0, 4, 16, None) == 0
    # a training-mode branch needs both of its sums
    assert lib.tpspp_bn_bwd_data(p, p, 1, p, p, p, p, p, 1, p, None, None, None, None, None, 1, None,
                                 None, None, 0, 0, 4, 16, None) == -22
    assert b"branch a" in err()
    assert lib.tpspp_bn_bwd_data(p, p, 1, p, p, p, p, None, 0, p, p, p, p, p, None, 1, p,
                                 p, None, 0, 0, 4, 16, None) == -22
    assert b"branch b" in err()
