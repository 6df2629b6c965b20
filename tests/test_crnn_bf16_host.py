"""Host side (no GPU) of VeryDeepVgg's reduced-precision modes: the argument checks of the blocked max-pool's entry point
(include/tpspp_crnn_bf16.h; host pointers: nothing is launched), the module's `compute_dtype` switch, and the
arithmetic of the two modes restated in float64 (tests/crnn_bf16_cases.py) against the golden features: the three-term split
must reach the project's 1e-4 bar by its arithmetic alone, and the plain-bf16 error printed here is the yardstick of
tests/test_gpu_crnn_bf16.py."""
import copy
import ctypes

import pytest
import torch

import crnn_bf16_cases as BC
from tps_pp_amd import _lib, build
from tps_pp_amd.crnn import VeryDeepVgg

CC = BC.CC


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def test_blocked_maxpool_refuses_bad_arguments_before_any_launch(lib):
    keep = (ctypes.c_float * 80)()
    p = (ctypes.addressof(keep) + 15) & ~15                        # host memory, 16-byte aligned: never dereferenced

    def refused(rc, text):
        assert rc == -22 and text.encode() in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())

    names = ("a", "layout", "N", "C", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "out", "Ho", "Wo", "s")
    base = dict(a=p, layout=2, N=1, C=8, H=4, W=6, kh=2, kw=2, sh=2, sw=1, ph=0, pw=1, out=p, Ho=2, Wo=7, s=None)

    def pool(**k):
        return lib.tpspp_crnn_maxpool_blk_fwd(*[{**base, **k}[n] for n in names])

    for layout in (2, 3):
        refused(pool(layout=layout, a=None), "null pointer")
        refused(pool(layout=layout, out=None), "null pointer")
        for c in (1, 4, 7, 9, 12):
            refused(pool(layout=layout, C=c), "multiple of 8 channels")
        refused(pool(layout=layout, C=0), "bad sizes")
        refused(pool(layout=layout, N=-1), "bad sizes")
        refused(pool(layout=layout, ph=2), "padding")               # ph > kh / 2
        refused(pool(layout=layout, pw=2), "padding")
        refused(pool(layout=layout, pw=-1), "padding")
        refused(pool(layout=layout, sh=0), "stride")
        refused(pool(layout=layout, kw=0), "kernel")
        refused(pool(layout=layout, Ho=3), "Ho x Wo must be 2 x 7")
        refused(pool(layout=layout, Wo=6), "Ho x Wo must be 2 x 7")
        refused(pool(layout=layout, H=1, ph=0, Ho=1), "smaller than the kernel")
        refused(pool(layout=layout, a=p + 4), "16-byte aligned")
        assert pool(layout=layout, N=0) == 0                        # nothing launched
    for layout in (0, 1, 4, -1):
        refused(pool(layout=layout), "layout must be 2")
    del keep


@pytest.mark.parametrize("env,want", [(None, None), ("bf16x3", "bf16x3"), ("bf16", torch.bfloat16), ("fp32", None)])
def test_vgg_compute_dtype_follows_the_environment(monkeypatch, env, want):
    if env is None:
        monkeypatch.delenv("TPSPP_COMPUTE_DTYPE", raising=False)
    else:
        monkeypatch.setenv("TPSPP_COMPUTE_DTYPE", env)
    assert VeryDeepVgg(leaky_relu=False, input_channels=1).compute_dtype == want


def test_recogniser_switch_reaches_the_vgg_and_adds_no_state(monkeypatch):
    monkeypatch.delenv("TPSPP_COMPUTE_DTYPE", raising=False)
    m = BC.build_model("crnn_tps")
    keys = list(m.state_dict())
    assert m.backbone.compute_dtype is None
    for mode in ("bf16x3", torch.bfloat16, None):
        assert m.set_compute_dtype(mode) is m and m.backbone.compute_dtype == mode
        assert list(m.state_dict()) == keys and not any("compute_dtype" in k for k in keys)
    with pytest.raises(ValueError, match="set_compute_dtype"):
        m.set_compute_dtype("fp16")
    assert not hasattr(m.decoder, "compute_dtype")                  # the decoder is exact fp32 in every mode


@pytest.mark.parametrize("mode", ["bf16x3", torch.bfloat16])
def test_host_batch_in_train_mode_is_the_pytorch_composition(mode):
    vgg = BC.build_model("crnn").backbone
    vgg.compute_dtype = mode
    img = torch.from_numpy(CC.images32())
    twin = copy.deepcopy(vgg)                                       # (train mode moves BatchNorm's running statistics)
    with torch.no_grad():
        want = twin.train()._forward_torch(img)
        got = vgg.train()(img)
        vgg.eval()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(_lib.TpsppError, match="GPU tensor"):        # eval on the host: no CPU path in any mode
        with torch.no_grad():
            vgg(img)
    leaky = VeryDeepVgg(leaky_relu=True, input_channels=1).eval()
    leaky.compute_dtype = mode
    with torch.no_grad():
        assert torch.equal(leaky(img), leaky._forward_torch(img))   # LeakyReLU: the PyTorch composition, also on the host


@pytest.mark.parametrize("name", ["crnn_tps", "crnn"])
def test_the_bar_is_reachable_in_float64(name):
    e = BC.route_errors(name)
    print(f"{name}: float64 restatement, features against the golden: bf16x3 max abs error {e['x3']:.3e} (bar 1e-4); "
          f"plain bf16 max abs error {e['bf16_abs']:.3e}, relative L2 {e['bf16_rel']:.3e} (printed: the GPU test's yardstick)")
    assert e["x3"] <= 1e-4
    assert 0 < e["bf16_rel"] < 1                                    # a yardstick, not a bar: it must only be a number
