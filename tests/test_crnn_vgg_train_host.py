"""Host side (no GPU) of VeryDeepVgg's HIP training graph (`set_vgg_train_backend("hip")`): the restated reference of
tests/crnn_vgg_train_cases.py against PyTorch's own max_pool2d backward on the CPU, bit for bit; the argument checks of
tpspp_crnn_maxpool_bwd (include/tpspp.h; host pointers: nothing is launched); and the switch."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import crnn_bf16_cases as BC
import crnn_vgg_train_cases as VC
import guarded_alloc as GA
import test_gpu_crnn_vgg_train as TG
import test_gpu_memory_safety as MS
from tps_pp_amd import _lib, build, build_detector
from tps_pp_amd.crnn import CRNNNet, VeryDeepVgg
from tps_pp_amd.registry import TrainBackendMixin


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


# ---- the restated reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VC.VARIANTS)
@pytest.mark.parametrize("case", VC.CASES, ids=VC.case_id)
def test_restated_reference_equals_pytorchs_backward_bit_for_bit(case, variant):
    k, s, p = case[4:7]
    y, dp = VC.make_case(case, variant)
    leaf = y.clone().requires_grad_(True)
    F.max_pool2d(leaf, k, s, p).backward(dp)
    plain = leaf.grad
    masked = torch.where(y > 0, plain, torch.zeros_like(plain))
    for relu_mask, want in ((0, plain), (1, masked)):
        ok, why = GA.same_bits(VC.restated_backward(y, dp, k, s, p, relu_mask), want)
        assert ok, f"{VC.case_id(case)} {variant} relu_mask={relu_mask}: {why}"
    if variant == "plain":                                          # the gradient is routed somewhere, and ties are there
        assert plain.abs().sum() > 0 and (masked != plain).any()


def test_the_case_table_covers_what_it_says():
    shapes = {c[:4] + (c[7],) for c in VC.CASES}
    assert len(VC.CASES) == 11 and (2, 3, 4, 8, "off1") in shapes and (1100, 64, 2, 2, "") in shapes
    assert 1100 * 64 > 65535
    y, _ = VC.make_case(VC.CASES[0], "pm0")
    assert (y.view(torch.int32) == -2 ** 31).any() and (y.view(torch.int32) == 0).any()
    y, _ = VC.make_case(VC.CASES[5], "nonfinite")
    assert torch.isnan(y).any() and (y == float("inf")).any() and (y == float("-inf")).any()
    t = VC.off_by_one(torch.arange(8.0).view(2, 4))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 and torch.equal(t, torch.arange(8.0).view(2, 4))


# ---- the entry point's argument checks ----------------------------------------------------------------------------------------
def test_maxpool_bwd_refuses_bad_arguments_before_any_launch(lib):
    keep = (ctypes.c_float * 80)()
    p = (ctypes.addressof(keep) + 15) & ~15                        # host memory, 16-byte aligned: never dereferenced
    names = ("dp", "y", "relu_mask", "N", "C", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dy", "Ho", "Wo", "s")
    base = dict(dp=p, y=p, relu_mask=1, N=2, C=3, H=8, W=25, kh=2, kw=2, sh=2, sw=1, ph=0, pw=1, dy=p, Ho=4, Wo=26, s=None)

    def call(**k):
        return lib.tpspp_crnn_maxpool_bwd(*[{**base, **k}[n] for n in names])

    def refused(rc, text):
        assert rc == -22 and text.encode() in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())

    for relu_mask in (0, 1):
        for ptr in ("dp", "y", "dy"):
            refused(call(relu_mask=relu_mask, **{ptr: None}), "null pointer")
        refused(call(relu_mask=relu_mask, Ho=5), "Ho x Wo must be 4 x 26")
        refused(call(relu_mask=relu_mask, Wo=25), "Ho x Wo must be 4 x 26")
        refused(call(relu_mask=relu_mask, Wo=0), "Ho x Wo must be 4 x 26")
        refused(call(relu_mask=relu_mask, pw=2, Wo=28), "padding must be 0 .. half the kernel size")
        refused(call(relu_mask=relu_mask, ph=2, Ho=6), "padding must be 0 .. half the kernel size")
        refused(call(relu_mask=relu_mask, pw=-1), "padding must be 0 .. half the kernel size")
        for zero in ("C", "H", "W"):
            refused(call(relu_mask=relu_mask, **{zero: 0}), "bad sizes")
        refused(call(relu_mask=relu_mask, N=-1), "bad sizes")
        for zero in ("kh", "kw", "sh", "sw"):
            refused(call(relu_mask=relu_mask, **{zero: 0}), "kernel and stride must be >= 1")
        refused(call(relu_mask=relu_mask, H=1, ph=0, Ho=0), "the padded map is smaller than the kernel")
        refused(call(relu_mask=relu_mask, N=1 << 20, C=1 << 10), "more than 2^31 - 1 elements")
        assert call(relu_mask=relu_mask, N=0) == 0                  # nothing launched
    refused(call(relu_mask=2), "relu_mask must be 0 or 1")
    del keep


def test_the_entry_point_is_in_the_memory_safety_sweep():
    assert TG.test_kernel_against_the_restated_reference_bit_for_bit.__name__ in MS.SWEPT["tpspp_crnn_maxpool_bwd"]
    assert "tpspp_crnn_maxpool_bwd" in _lib.symbols("tpspp.h")


# ---- the switch -------------------------------------------------------------------------------------------------------------
def test_switch_semantics():
    m = BC.build_model("crnn_tps")
    vgg = m.backbone
    keys, count = list(m.state_dict()), len(list(m.parameters()))
    assert isinstance(m, CRNNNet) and isinstance(vgg, VeryDeepVgg) and vgg.vgg_train_backend == "torch"
    assert VeryDeepVgg().vgg_train_backend == "torch"
    assert vgg.set_vgg_train_backend("hip") is vgg and vgg.vgg_train_backend == "hip"
    for bad in ("HIP", "hip_all", None, 1):
        with pytest.raises(ValueError, match="set_vgg_train_backend"):
            vgg.set_vgg_train_backend(bad)
        assert vgg.vgg_train_backend == "hip"                       # a call that fails changes nothing
    assert vgg.set_vgg_train_backend("torch").vgg_train_backend == "torch"
    # the recogniser's pass-through
    assert m.set_vgg_train_backend("hip") is m and vgg.vgg_train_backend == "hip"
    with pytest.raises(ValueError, match="set_vgg_train_backend"):
        m.set_vgg_train_backend("cuda")
    assert vgg.vgg_train_backend == "hip"
    assert list(m.state_dict()) == keys and len(list(m.parameters())) == count
    assert not any("train_backend" in k for k in m.state_dict())
    assert len(list(m.buffers())) == len(list(BC.build_model("crnn_tps").buffers()))
    # a copy keeps the switch; the other switches do not touch it, nor it them
    assert copy.deepcopy(vgg).vgg_train_backend == "hip"
    m.set_train_backend("torch", preprocessor="hip", decoder="hip", loss="hip")
    assert vgg.vgg_train_backend == "hip" and m.decoder.train_backend == "hip"
    m.set_vgg_train_backend("torch")
    assert m.decoder.train_backend == "hip" and m.preprocessor.train_backend == "hip"


def test_leaky_relu_refuses_the_hip_backend():
    vgg = VeryDeepVgg(leaky_relu=True)
    with pytest.raises(ValueError, match="leaky_relu=False"):
        vgg.set_vgg_train_backend("hip")
    assert vgg.vgg_train_backend == "torch" and vgg.set_vgg_train_backend("torch") is vgg


def test_the_backbone_refusal_of_set_train_backend_stays():
    """`CRNNNet.set_train_backend(..., backbone="hip")` tells a backbone with a HIP training path by the attribute
    `set_train_backend`: the VGG's switch has its own name, so that refusal stands."""
    assert not hasattr(VeryDeepVgg, "set_train_backend") and not hasattr(VeryDeepVgg(), "set_train_backend")
    assert not issubclass(VeryDeepVgg, TrainBackendMixin)
    m = BC.build_model("crnn_tps").set_vgg_train_backend("hip")
    with pytest.raises(ValueError, match="has no HIP training path"):
        m.set_train_backend("torch", backbone="hip")


def test_a_recogniser_without_a_vgg_does_not_take_the_switch():
    nrtr = build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                          strides=[2, 1, 2, 1, 2]),
                               tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                               decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                               label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True), max_seq_len=8))
    assert not hasattr(nrtr, "set_vgg_train_backend")
    m = BC.build_model("crnn")
    m.backbone = torch.nn.Identity()
    with pytest.raises(ValueError, match="Identity"):
        m.set_vgg_train_backend("hip")


def test_a_host_batch_with_the_backend_set_still_trains_through_pytorch():
    torch.manual_seed(3)
    vgg = VeryDeepVgg(leaky_relu=False, input_channels=1).train().set_vgg_train_backend("hip")
    twin = copy.deepcopy(vgg).set_vgg_train_backend("torch")
    x = torch.rand((2, 1, 32, 24), generator=torch.Generator().manual_seed(4))
    got = vgg(x.clone().requires_grad_(True))
    want = twin(x.clone().requires_grad_(True))
    assert got.grad_fn is not None and GA.same_bits(got.detach(), want.detach())[0]
    got.square().mean().backward()
    want.square().mean().backward()
    for (n, a), (_, b) in zip(vgg.named_parameters(), twin.named_parameters()):
        assert a.grad is not None and GA.same_bits(a.grad, b.grad)[0], n
    for (n, a), (_, b) in zip(vgg.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b), n
