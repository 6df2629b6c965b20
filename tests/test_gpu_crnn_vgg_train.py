"""-m gpu: VeryDeepVgg's HIP training graph (`set_vgg_train_backend("hip")`) -- the max-pool backward with the ReLU mask
(tpspp_crnn_maxpool_bwd, include/tpspp.h) bit for bit against the restated reference of tests/crnn_vgg_train_cases.py inside
tests/guarded_alloc.py's guard bands and poison; the convolution + ReLU + pool layers and conv6 + BatchNorm against float64
autograd on the CPU; the module; and the crnn_tps recogniser with every stage on its HIP backend.

Bar (tests/test_gpu_backbone_train.py's): relative L2 <= max(1e-5, 2 x the relative L2 of PyTorch's fp32 composition of the
same thing on the same inputs on the GPU), both measured against float64 on the CPU."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import crnn_bf16_cases as BC
import crnn_vgg_train_cases as VC
import guarded_alloc as GA
import test_gpu_memory_safety as MS
from test_gpu_backbone_train import bar, randomize_bn, rel
from tps_pp_amd import _lib, ops
from tps_pp_amd.crnn import VeryDeepVgg

pytestmark = pytest.mark.gpu
CC = BC.CC


def sweeps(*names):
    """tests/test_gpu_tps_train.py's pattern: enters a test of this file into the memory-safety sweep's table
    (tests/test_gpu_memory_safety.py: `SWEPT`, which tests/test_memory_safety_host.py holds against include/tpspp.h) as the
    guard case of the entry points `names`; the test must fetch every one of them from the library while it runs."""
    def deco(fn):
        for n in names:
            MS.SWEPT.setdefault(n, []).append(fn.__name__)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            real = _lib.lib()
            del MS._NOW[:]
            _lib._lib = MS._Spy(real)
            try:
                fn(*a, **kw)
            finally:
                _lib._lib = real
            missing = set(names) - set(MS._NOW)
            assert not missing, f"{fn.__name__} declares {sorted(missing)} but never called them"
        return wrapper
    return deco


def check(label, got, want, lib32):
    """{name: tensor} dicts; every entry of `want` within the bar.  The errors are printed before anything is asserted."""
    rows = {k: (rel(got[k], w), bar(lib32[k], w)) for k, w in want.items()}
    for k, (e, b) in rows.items():
        print(f"{label} {k}: rel L2 {e:.3e} (bar {b:.3e})")
    for k in want:
        assert torch.isfinite(got[k]).all(), f"{label}: {k} not finite"
    bad = {k: v for k, v in rows.items() if v[0] > v[1]}
    assert not bad, f"{label}: {bad}"


def assert_same_bits(a, b, what):
    ok, why = GA.same_bits(a, b)
    assert ok, f"{what}: {why}"


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(case, variant, relu_mask):
    """(y, dp, restated dy) on the CPU, computed once and shared; never modified."""
    y, dp = VC.make_case(case, variant)
    return y, dp, VC.restated_backward(y, dp, *case[4:7], relu_mask)


def put_case(g, case, y, dp):
    y_, dp_ = g.input(y), g.input(dp)
    if case[7] == "off1":
        y_, dp_ = VC.off_by_one(y_), VC.off_by_one(dp_)
        assert y_.data_ptr() % 16 == 4 and dp_.data_ptr() % 16 == 4
    return y_, dp_


@pytest.mark.parametrize("relu_mask", [0, 1])
@pytest.mark.parametrize("variant", VC.VARIANTS)
@pytest.mark.parametrize("case", VC.CASES, ids=VC.case_id)
@sweeps("tpspp_crnn_maxpool_bwd")
def test_kernel_against_the_restated_reference_bit_for_bit(cuda, case, variant, relu_mask):
    y, dp, want = reference(case, variant, relu_mask)
    with GA.guarded(cuda) as g:
        y_, dp_ = put_case(g, case, y, dp)
        dy = ops.crnn_maxpool_bwd(dp_, y_, *case[4:7], relu_mask=relu_mask)
        assert g.check(dy, require_guarded=True) >= 1               # guards intact, every element of dy written
    assert_same_bits(dy.cpu(), want, f"{VC.case_id(case)} {variant} relu_mask={relu_mask}")


@pytest.mark.parametrize("case", [VC.CASES[0], VC.CASES[2], VC.CASES[5], VC.CASES[9]], ids=VC.case_id)
def test_kernel_gives_the_same_bits_on_two_streams(cuda, case):
    y, dp, want = reference(case, "plain", 1)
    y_, dp_ = y.to(cuda), dp.to(cuda)
    first = ops.crnn_maxpool_bwd(dp_, y_, *case[4:7])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(cuda)
    with torch.cuda.stream(side):
        other = ops.crnn_maxpool_bwd(dp_, y_, *case[4:7])
    side.synchronize()
    assert_same_bits(first, other, "side stream")
    assert_same_bits(first.cpu(), want, "default stream")


def test_both_forms_agree_and_an_empty_batch_launches_nothing(cuda):
    """The float4 form (aligned) and the one-lane-per-element form (the same values one element off alignment) on a map
    with several blocks; the wrapper's shape checks; N = 0."""
    g0 = torch.Generator().manual_seed(2)
    y = torch.randn((3, 16, 6, 64), generator=g0).clamp_(min=0).to(cuda)
    dp = torch.randn((3, 16, 3, 32), generator=g0).to(cuda)
    vec = ops.crnn_maxpool_bwd(dp, y, 2, 2, 0)
    scalar = ops.crnn_maxpool_bwd(VC.off_by_one(dp), VC.off_by_one(y), 2, 2, 0)
    assert_same_bits(vec, scalar, "float4 form against the scalar form")
    leaf = y.clone().requires_grad_(True)
    F.max_pool2d(leaf, 2, 2).backward(dp)
    assert_same_bits(vec, torch.where(y > 0, leaf.grad, torch.zeros_like(y)), "against PyTorch's backward and mask")
    with pytest.raises(ValueError, match="dp must be"):
        ops.crnn_maxpool_bwd(dp[:, :, :, :31], y, 2, 2, 0)
    with pytest.raises(_lib.TpsppError):
        ops.crnn_maxpool_bwd(dp.cpu(), y.cpu(), 2, 2, 0)
    empty = ops.crnn_maxpool_bwd(dp[:0], y[:0], 2, 2, 0)
    assert empty.shape == (0, 16, 6, 64)


# ---- 2. convolution + ReLU + pool ------------------------------------------------------------------------------------------
# (Cin, Cout, H, W, pool): conv0 at 1 and 3 input channels, conv1, conv3 and conv5 at narrow widths
LAYERS = [(1, 64, 32, 24, VC.P22), (3, 64, 32, 24, VC.P22), (64, 128, 16, 12, VC.P22), (256, 256, 8, 7, VC.RECT),
          (512, 512, 4, 8, VC.RECT)]
LAYER_IDS = [f"{ci}to{co}-{h}x{w}" for ci, co, h, w, _ in LAYERS]


def layer_inputs(layer, N=2):
    cin, cout, H, W, pool = layer
    g0 = torch.Generator().manual_seed(cin + 7 * W)
    conv = nn.Conv2d(cin, cout, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g0) / (3 * cin ** 0.5))
        conv.bias.copy_(0.1 * torch.randn(cout, generator=g0))
    Ho, Wo = VC.out_size(H, W, *pool)
    gp = torch.randn((N, cout, Ho, Wo), generator=g0)
    conv64 = copy.deepcopy(conv).double()
    for seed in range(1000, 1200):          # the first input of a fixed sequence whose float64 layer is away from the kinks
        x = torch.randn((N, cin, H, W), generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            z = conv64(x.double())
        if min(VC.relu_margin(z), VC.pool_margin(F.relu(z), *pool)) >= VC.MARGIN:
            return conv, x, gp
    raise AssertionError(f"no input with margin {VC.MARGIN} in 200 seeds")


def layer_reference(conv, x, gp, pool, dtype, device):
    conv = copy.deepcopy(conv).to(device).to(dtype)
    xr = x.to(device).to(dtype).requires_grad_(True)
    p = F.max_pool2d(F.relu(conv(xr)), *pool)
    p.backward(gp.to(device).to(dtype))
    return dict(p=p.detach().cpu(), dx=xr.grad.cpu(), dW=conv.weight.grad.cpu(), db=conv.bias.grad.cpu())


@pytest.mark.parametrize("layer", LAYERS, ids=LAYER_IDS)
def test_conv_relu_pool_against_float64_autograd(cuda, layer):
    conv, x, gp = layer_inputs(layer)
    pool = layer[4]
    want = layer_reference(conv, x, gp, pool, torch.float64, "cpu")
    lib32 = layer_reference(conv, x, gp, pool, torch.float32, cuda)
    with GA.guarded(cuda) as g:
        mod = MS.put_module(conv, g.input)
        xg = g.input(x).requires_grad_(True)
        p = ops.conv_relu_pool_autograd(xg, mod, *pool)
        unfused = ops.crnn_maxpool(ops.conv2d([xg.detach()], ops.prep_conv_weight_device(mod.weight, mod.bias), 1, True), *pool)
        p.backward(g.input(gp))
        g.check((p.detach(), unfused, xg.grad, mod.weight.grad, mod.bias.grad))
    assert_same_bits(p.detach(), unfused, "forward against crnn_maxpool(conv2d(relu=True))")
    got = dict(p=p.detach(), dx=xg.grad, dW=mod.weight.grad, db=mod.bias.grad)
    for k in ("dx", "dW", "db"):
        assert want[k].abs().max() > 0, k
    check(f"conv+relu+pool {LAYER_IDS[LAYERS.index(layer)]}", got, want, lib32)


def test_conv_relu_pool_launches_nothing_for_what_needs_no_gradient(cuda, monkeypatch):
    conv, x, gp = layer_inputs(LAYERS[1])
    conv, x, gp = conv.to(cuda), x.to(cuda), gp.to(cuda)
    calls = []
    for name in ("crnn_maxpool_bwd", "conv2d_bwd_weight", "conv2d_bwd_data"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append((_n, k)), _r(*a, **k))[1])

    def run(x_grad, w_grad, b_grad):
        del calls[:]
        conv.weight.requires_grad_(w_grad)
        conv.bias.requires_grad_(b_grad)
        conv.weight.grad = conv.bias.grad = None
        xr = x.clone().requires_grad_(x_grad)
        p = ops.conv_relu_pool_autograd(xr, conv, 2, 2, 0)
        if p.requires_grad:
            p.backward(gp)
        return [n for n, _ in calls], xr.grad

    names, dx = run(True, True, True)
    assert names == ["crnn_maxpool_bwd", "conv2d_bwd_weight", "conv2d_bwd_data"] and dx is not None
    assert all(k.get("relu") is False for n, k in calls if n != "crnn_maxpool_bwd")     # the mask was folded into the pool
    assert calls[0][1] == {"relu_mask": True}
    names, dx = run(False, True, True)                              # the image without a rectifier in front
    assert names == ["crnn_maxpool_bwd", "conv2d_bwd_weight"] and dx is None and conv.weight.grad is not None
    names, dx = run(True, False, False)                             # a frozen layer
    assert names == ["crnn_maxpool_bwd", "conv2d_bwd_data"] and dx is not None and conv.weight.grad is None
    names, _ = run(True, False, True)
    assert names == ["crnn_maxpool_bwd", "conv2d_bwd_weight", "conv2d_bwd_data"]
    assert calls[1][1]["want_weight"] is False and conv.weight.grad is None and conv.bias.grad is not None
    names, _ = run(False, False, False)
    assert names == []


# ---- 3. conv6 + BatchNorm ---------------------------------------------------------------------------------------------------
def conv6_inputs(C=512, N=3, W=8):
    g0 = torch.Generator().manual_seed(66)
    conv = nn.Conv2d(C, C, 2, 1, 0)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g0) / (2 * C ** 0.5))
        conv.bias.copy_(0.1 * torch.randn(C, generator=g0))
    block = randomize_bn(nn.Sequential(conv, nn.BatchNorm2d(C), nn.ReLU(True)), 67).train()
    gy = torch.randn((N, C, 1, W - 1), generator=g0)
    head = copy.deepcopy(block[:2]).double()
    for seed in range(2000, 2200):          # the first input of a fixed sequence whose float64 block is away from the kink
        x = torch.randn((N, C, 2, W), generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            if VC.relu_margin(copy.deepcopy(head)(x.double())) >= VC.MARGIN:
                return block, x, gy
    raise AssertionError(f"no input with margin {VC.MARGIN} in 200 seeds")


def conv6_step(block, x, gy, hip):
    xr = x.clone().requires_grad_(True)
    y = ops.conv6_bn_autograd(xr, block[0], block[1]) if hip else block(xr)
    y.backward(gy)
    res = dict(y=y.detach(), dx=xr.grad, dW=block[0].weight.grad, db=block[0].bias.grad, dgamma=block[1].weight.grad,
               dbeta=block[1].bias.grad, running_mean=block[1].running_mean, running_var=block[1].running_var)
    return {k: v.detach().cpu() for k, v in res.items()}, int(block[1].num_batches_tracked)


def test_conv6_batchnorm_against_float64_autograd(cuda):
    block, x, gy = conv6_inputs()
    want, n64 = conv6_step(copy.deepcopy(block).double(), x.double(), gy.double(), False)
    lib32, n32 = conv6_step(copy.deepcopy(block).to(cuda), x.to(cuda), gy.to(cuda), False)
    with GA.guarded(cuda) as g:
        got, nh = conv6_step(MS.put_module(block, g.input).train(), g.input(x), g.input(gy), True)
        g.check()
    assert nh == n64 == n32 == 4
    assert got["y"].shape == (3, 512, 1, 7)
    check("conv6+bn", got, want, lib32)
    # the statistics are those of the sliced map: the W-wide map of the zero-extended kernel has other ones
    conv, bn = block[0].double(), block[1]
    with torch.no_grad():
        wide = F.conv2d(x.double(), F.pad(conv.weight, (1, 0, 1, 0)), conv.bias, (2, 1), 1)
        assert wide.shape[3] == 8 and rel(wide[:, :, :, :7], conv(x.double())) < 1e-12
        wrong = 0.9 * bn.running_mean.double() + 0.1 * wide.mean((0, 2, 3))
    print(f"running_mean against the W-wide map's: {rel(got['running_mean'], wrong):.3e}")
    assert rel(got["running_mean"], wrong) > 100 * bar(lib32["running_mean"], want["running_mean"])


def test_conv6_refuses_other_maps_and_convolutions(cuda):
    block, x, _ = conv6_inputs(C=16, N=2, W=4)
    block, x = block.to(cuda), x.to(cuda)
    with pytest.raises(ValueError, match="two-row map"):
        ops.conv6_bn_autograd(torch.zeros((2, 16, 4, 4), device=cuda), block[0], block[1])
    with pytest.raises(ValueError, match="nn.Conv2d"):
        ops.conv6_bn_autograd(x, nn.Conv2d(16, 16, 3, 1, 1).to(cuda), block[1])
    assert ops.conv6_bn_autograd(x, block[0], block[1]).shape == (2, 16, 1, 3)


# ---- 4. the module ----------------------------------------------------------------------------------------------------------
def vgg(channels, seed=0):
    torch.manual_seed(seed)
    return randomize_bn(VeryDeepVgg(leaky_relu=False, input_channels=channels), seed + 100)


def image(N, channels, seed, W=24):
    return torch.rand((N, channels, 32, W), generator=torch.Generator().manual_seed(seed))


# (channels, N, training) -> the first image seed from 21 / 23 / 6 on whose float64 forward keeps VC.MARGIN from every ReLU and
# pooling kink (tests/crnn_vgg_train_cases.py says why; found with `VC.vgg_margin`, which the tests assert again).  The
# seeds first used here, 21 and 23, did not: at 23 two activations of a pooling2 window lie 1.8e-7 of the map's RMS apart, and
# which of them an fp32 forward selects moved every gradient below conv3 by 3e-3.
CLEAR_IMAGE = {(1, 4, True): 327, (3, 4, True): 61, (1, 2, False): 68}


def clear_image(base, N, channels):
    img = image(N, channels, CLEAR_IMAGE[channels, N, base.training])
    margin = VC.vgg_margin(copy.deepcopy(base).double(), img.double())
    print(f"margin of the float64 reference from its ReLU and pooling kinks: {margin:.3e} of the map's RMS")
    assert margin >= VC.MARGIN
    return img


def vgg_step(m, img, gout, hip):
    x = img.clone().requires_grad_(True)
    out = m(x) if hip else m._forward_torch(x)
    out.backward(gout)
    res = {"features": out.detach(), "d_img": x.grad}
    res.update({"d_" + k: p.grad for k, p in m.named_parameters()})
    res.update({k: b for k, b in m.named_buffers() if not k.endswith("num_batches_tracked")})
    counters = [int(b) for k, b in m.named_buffers() if k.endswith("num_batches_tracked")]
    return {k: v.detach().cpu().clone() for k, v in res.items()}, counters


@pytest.mark.parametrize("channels", [1, 3])
def test_module_against_its_float64_composition(cuda, channels):
    N = 4
    gout = torch.randn((N, 512, 1, 7), generator=torch.Generator().manual_seed(30 + channels))
    base = vgg(channels).train()
    img = clear_image(base, N, channels)
    want, n64 = vgg_step(copy.deepcopy(base).double(), img.double(), gout.double(), False)
    lib32, _ = vgg_step(copy.deepcopy(base).to(cuda), img.to(cuda), gout.to(cuda), False)
    with GA.guarded(cuda) as g:
        mh = MS.put_module(base, g.input).train().set_vgg_train_backend("hip")
        got, nh = vgg_step(mh, g.input(img), g.input(gout), True)
        g.check()
    again, _ = vgg_step(copy.deepcopy(base).to(cuda).set_vgg_train_backend("hip"), img.to(cuda), gout.to(cuda), True)
    assert nh == n64 == [4, 4, 4]
    for k in want:
        if k.startswith("d_"):
            assert want[k].abs().max() > 0, f"{k}: the reference gradient is zero, the comparison shows nothing"
    check(f"vgg C={channels}", got, want, lib32)
    assert_same_bits([got[k] for k in sorted(got)], [again[k] for k in sorted(got)], "a second run")


def test_no_library_layer_runs_on_the_hip_backend(cuda, monkeypatch):
    m = vgg(1).to(cuda).train().set_vgg_train_backend("hip")
    x = image(2, 1, 1).to(cuda).requires_grad_(True)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the HIP training path")
        return f

    for name in ("conv2d", "batch_norm", "max_pool2d", "relu", "relu_", "threshold"):
        monkeypatch.setattr(F, name, refuse(f"F.{name}"))
    out = m(x)
    out.square().mean().backward()
    assert out.shape == (2, 512, 1, 7) and torch.isfinite(out).all() and x.grad.abs().max() > 0
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
    with pytest.raises(AssertionError, match="called on the HIP training path"):
        m.set_vgg_train_backend("torch")(x)


def test_eval_output_has_the_same_bits_before_and_after_the_switch(cuda):
    m = vgg(3).to(cuda).eval()
    x = image(3, 3, 5).to(cuda)
    with torch.no_grad():
        before = m(x)
        after = m.set_vgg_train_backend("hip")(x)
    assert_same_bits(before, after, "eval output across the switch")
    assert set(m.state_dict()) == set(vgg(3).state_dict())


def test_eval_mode_module_with_an_input_that_requires_grad_uses_running_statistics(cuda):
    base = vgg(1).eval()
    img = clear_image(base, 2, 1)
    gout = torch.randn((2, 512, 1, 7), generator=torch.Generator().manual_seed(8))
    want, n64 = vgg_step(copy.deepcopy(base).double(), img.double(), gout.double(), False)
    lib32, _ = vgg_step(copy.deepcopy(base).to(cuda), img.to(cuda), gout.to(cuda), False)
    mh = copy.deepcopy(base).to(cuda).set_vgg_train_backend("hip")
    x = img.to(cuda).requires_grad_(True)
    assert mh(x).grad_fn is not None                                # the graph, not the eval fast path
    got, nh = vgg_step(mh, img.to(cuda), gout.to(cuda), True)
    assert nh == n64 == [3, 3, 3]
    for k, b in base.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(got[k], b), k                       # running statistics were read, not moved
    check("vgg eval", got, want, lib32)


# ---- 5. the recogniser ------------------------------------------------------------------------------------------------------
def tail_step(m, rect, targets, metas, dtype, device):
    """VGG -> decoder -> CTC loss as PyTorch compositions from the rectified images `rect`, in `dtype` on `device`."""
    backbone = copy.deepcopy(m.backbone).to(device).to(dtype).train().set_vgg_train_backend("torch")
    decoder = copy.deepcopy(m.decoder).to(device).to(dtype).train().set_train_backend("torch")
    loss_fn = copy.deepcopy(m.loss).set_train_backend("torch")
    feat = backbone._forward_torch(rect.to(device).to(dtype))
    loss = loss_fn(decoder._forward_torch(feat), targets, metas)["loss_ctc"]
    loss.backward()
    res = {"loss": loss.detach().reshape(1)}
    res.update({"d_" + k: p.grad for k, p in backbone.named_parameters()})
    return {k: v.detach().cpu() for k, v in res.items()}


def test_one_step_of_crnn_tps_with_every_stage_on_hip(cuda):
    torch.manual_seed(0)
    m = BC.build_model("crnn_tps").to(cuda).train()
    m.set_train_backend("torch", preprocessor="hip", decoder="hip", loss="hip").set_vgg_train_backend("hip")
    img = torch.from_numpy(CC.images()).to(cuda)
    metas = [dict(resize_shape=(32, 100, 1), text=s) for s in CC.TEXTS]
    base = copy.deepcopy(m)                                         # before the step moves the running statistics
    seen = []
    hook = m.backbone.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().clone()))
    loss = m(img, metas, return_loss=True)["loss_ctc"]
    hook.remove()
    loss.backward()
    assert torch.isfinite(loss) and len(seen) == 1 and seen[0].shape == (3, 1, 32, 100)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    got = {"loss": loss.detach().reshape(1).cpu()}
    got.update({"d_" + k: p.grad.detach().cpu() for k, p in m.backbone.named_parameters()})
    targets = m.label_convertor.str2tensor(list(CC.TEXTS))
    want = tail_step(base, seen[0].cpu(), targets, metas, torch.float64, "cpu")
    lib32 = tail_step(base, seen[0], targets, metas, torch.float32, cuda)
    check("crnn_tps", got, want, lib32)
