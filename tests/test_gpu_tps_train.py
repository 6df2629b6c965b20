"""-m gpu: the classic rectifier's "hip" train backend -- the fused BatchNorm + ReLU + 2x2 max-pool kernels of
tpspp_bn_pool_train.hip alone (bit for bit against the unfused kernels, exactly against float64 where fp32 is exact, and
against float64 autograd on the shared cases of tests/tps_train_cases.py), the convolution backward kernels with 1 and 3
input channels, the localisation network as a whole against its own float64 composition on the CPU, and the module and
recogniser switches.  Every kernel call runs inside tests/guarded_alloc.py's guard bands and poison.

Bar (tests/test_gpu_backbone_train.py's): relative L2 <= max(1e-5, 2 x the relative L2 of PyTorch's fp32 composition of the
same thing on the same inputs on the GPU), both measured against float64 on the CPU."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import crnn_cases as CC
import guarded_alloc as GA
import test_gpu_memory_safety as MS
import tps_train_cases as cases
from tps_pp_amd import TPSPreprocessor, _lib, build_detector, ops
from tps_pp_amd.tps_preprocessor import LocalizationNetwork

pytestmark = pytest.mark.gpu

CASE_IDS = [cases.case_id(c) for c in cases.CASES]


def sweeps(*names):
    """Enters a test of this file into the memory-safety sweep's table (tests/test_gpu_memory_safety.py: `SWEPT`, which
    tests/test_memory_safety_host.py holds against include/tpspp.h) as the guard case of the entry points `names`.  As
    there, the declaration is checked: the test must fetch every one of them from the library while it runs."""
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


def rel(got, want):
    want = want.double().cpu()
    n = want.norm()
    d = (got.detach().cpu().double() - want).norm()
    return (d / n).item() if n > 0 else d.item()


def bar(lib32, want):
    return max(1e-5, 2 * rel(lib32, want))


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


def is_plus_zero(t):
    return bool((t.view(torch.int32) == 0).all())


def run_kernels(g, c, train, stats=None):
    """The fused kernels and the unfused pair on case dict `c` inside guard `g`."""
    z, dp, gamma, beta = (g.input(c[k]) for k in ("z", "dp", "gamma", "beta"))
    rm, rv = g.input(c["running_mean"]), g.input(c["running_var"])
    nbt = torch.tensor(3, device=g.device)
    if stats is None:
        stats = ops.bn_train_stats(z, cases.EPS, cases.MOMENTUM, rm, rv, nbt) if train else ops.bn_eval_stats(rm, rv, cases.EPS)
    p = ops.bn_pool2x2_fwd(z, stats, gamma, beta)
    unfused = ops.maxpool2x2(ops.bn_apply(z, stats, gamma, beta, relu=True))
    sums = ops.bn_pool2x2_bwd_reduce(dp, z, stats, gamma, beta)
    dz = ops.bn_pool2x2_bwd_data(dp, z, stats, gamma, beta, sums if train else None, train)
    g.check((p, unfused, sums, dz))
    return dict(p=p, unfused=unfused, dz=dz, dbeta=sums[0], dgamma=sums[1], running_mean=rm, running_var=rv, nbt=nbt,
                stats=stats)


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("case", cases.CASES, ids=CASE_IDS)
@sweeps("tpspp_bn_pool2x2_fwd", "tpspp_bn_pool2x2_bwd_reduce_workspace_floats", "tpspp_bn_pool2x2_bwd_reduce",
        "tpspp_bn_pool2x2_bwd_data")
def test_fused_kernels_against_the_unfused_bits_and_float64_autograd(cuda, case, train):
    c = cases.make_case(*case)
    with GA.guarded(cuda) as g:
        r = run_kernels(g, c, train)
    assert_same_bits(r["p"], r["unfused"], "fused forward against maxpool2x2(bn_apply)")
    want = cases.autograd_reference(*case, train)
    lib32 = cases.autograd_reference(*case, train, torch.float32, str(cuda))
    names = ["p", "dz", "dgamma", "dbeta"] + (["running_mean", "running_var"] if train else [])
    check(f"{cases.case_id(case)} {'train' if train else 'eval'}", r, {k: want[k] for k in names}, lib32)
    assert int(r["nbt"]) == (4 if train else 3)
    if not train:
        assert torch.equal(r["running_mean"].cpu(), c["running_mean"]) and torch.equal(r["running_var"].cpu(), c["running_var"])
        H, W = case[2:]
        dz = r["dz"]
        assert is_plus_zero(dz[:, :, 2 * (H // 2):].contiguous()) and is_plus_zero(dz[:, :, :, 2 * (W // 2):].contiguous())


@pytest.mark.parametrize("case", [(2, 5, 5, 7), (2, 4, 6, 8), (3, 64, 8, 25)], ids=cases.case_id)
def test_forward_with_explicit_statistics_and_non_finite_z(cuda, case):
    N, C, H, W = case
    g0 = torch.Generator().manual_seed(5)
    z = torch.randn(case, generator=g0)
    flat = z.view(-1)
    idx = torch.randperm(flat.numel(), generator=g0)[:max(6, flat.numel() // 7)]
    flat[idx] = torch.tensor([float("inf"), float("-inf"), float("nan")]).repeat(idx.numel() // 3 + 1)[:idx.numel()]
    c = dict(z=z, dp=torch.randn((N, C, H // 2, W // 2), generator=g0), gamma=torch.randn(C, generator=g0),
             beta=torch.randn(C, generator=g0), running_mean=torch.zeros(C), running_var=torch.ones(C))
    c["gamma"][0] = 0.0                                          # inf * 0 inside the activation
    with GA.guarded(cuda) as g:
        stats = (g.input(0.3 * torch.randn(C, generator=g0)), g.input(0.5 + torch.rand(C, generator=g0)))
        z_, gamma, beta = g.input(c["z"]), g.input(c["gamma"]), g.input(c["beta"])
        p = ops.bn_pool2x2_fwd(z_, stats, gamma, beta)
        unfused = ops.maxpool2x2(ops.bn_apply(z_, stats, gamma, beta, relu=True))
        dz = ops.bn_pool2x2_bwd_data(g.input(c["dp"]), z_, stats, gamma, beta, None, False)
        g.check((p, unfused, dz))
    assert_same_bits(p, unfused, "fused forward with inf / NaN in z")
    assert torch.isinf(p).any()
    assert dz.shape == z.shape


@pytest.mark.parametrize("shape", [(2, 4, 6, 8), (2, 4, 5, 7), (1, 4, 8, 25)], ids=cases.case_id)
def test_exact_case_equals_float64_bit_for_bit(cuda, shape):
    """Small-integer z, integer mean, power-of-two rstd, dyadic gamma / beta / dp, train = 0: every product and sum is exact
    in fp32, so dz, sum_dr and sum_dr_x must carry float64's value in every bit.  z in -3..3: ties everywhere."""
    N, C, H, W = shape
    g0 = torch.Generator().manual_seed(11)
    z = torch.randint(-3, 4, shape, generator=g0).float()
    mean = torch.tensor([1.0, -1.0, 0.0, 2.0])
    rstd = torch.tensor([0.5, 1.0, 2.0, 0.25])
    gamma = torch.tensor([1.5, -0.75, 1.0, 2.0])
    beta = torch.tensor([0.25, 0.5, -1.0, 0.125])
    dp = torch.randint(-8, 9, (N, C, H // 2, W // 2), generator=g0).float() / 4
    p64, dz64, sdr64, sdx64 = cases.restated_backward(z.double(), dp.double(), mean.double(), rstd.double(), gamma.double(),
                                                      beta.double(), False)
    a4 = cases.windows(cases.activation(z.double(), mean.double(), rstd.double(), gamma.double(), beta.double()))
    top = a4.sort(-1, descending=True).values
    assert int(((top[..., 0] == top[..., 1]) & (top[..., 0] > 0)).sum()) >= 4           # deliberate ties in positive values
    with GA.guarded(cuda) as g:
        stats = (g.input(mean), g.input(rstd))
        z_, dp_, ga, be = g.input(z), g.input(dp), g.input(gamma), g.input(beta)
        p = ops.bn_pool2x2_fwd(z_, stats, ga, be)
        sdr, sdx = ops.bn_pool2x2_bwd_reduce(dp_, z_, stats, ga, be)
        dz = ops.bn_pool2x2_bwd_data(dp_, z_, stats, ga, be, None, False)
        g.check((p, sdr, sdx, dz))
    for name, got, want in (("p", p, p64), ("dz", dz, dz64), ("sum_dr", sdr, sdr64), ("sum_dr_x", sdx, sdx64)):
        assert torch.equal(want.float().double(), want), name               # the float64 value is an fp32 number
        assert torch.equal(got.cpu().double(), want), name
    assert is_plus_zero(dz[dz == 0])                                         # no -0 from a negative gamma


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("case", [(2, 5, 5, 7), (3, 64, 8, 25), (2, 128, 16, 50)], ids=cases.case_id)
def test_zero_gradient_gives_plus_zero(cuda, case, train):
    c = dict(cases.make_case(*case))
    c["dp"] = torch.zeros_like(c["dp"])
    with GA.guarded(cuda) as g:
        r = run_kernels(g, c, train)
    assert is_plus_zero(r["dz"]) and is_plus_zero(r["dbeta"]) and is_plus_zero(r["dgamma"])


@pytest.mark.parametrize("case", [(3, 8, 37, 41), (2, 128, 16, 50)], ids=cases.case_id)
def test_bitwise_reproducible_across_calls_and_streams(cuda, case):
    c = cases.make_case(*case)
    with GA.guarded(cuda) as g:
        first = run_kernels(g, c, 1)
        again = run_kernels(g, c, 1)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(cuda)
        with torch.cuda.stream(side):
            other = run_kernels(g, c, 1)
        side.synchronize()
    keys = ("p", "dz", "dgamma", "dbeta", "running_mean", "running_var")
    assert_same_bits([first[k] for k in keys], [again[k] for k in keys], "second call")
    assert_same_bits([first[k] for k in keys], [other[k] for k in keys], "side stream")


@pytest.mark.parametrize("case", [(2, 5, 5, 7), (3, 64, 8, 25), (2, 128, 16, 50)], ids=cases.case_id)
def test_eval_mode_gradient_of_an_image_does_not_depend_on_the_batch(cuda, case):
    c = cases.make_case(*case)
    alone = {k: (v[:1].contiguous() if k in ("z", "dp") else v) for k, v in c.items() if k != "seed"}
    with GA.guarded(cuda) as g:
        whole = run_kernels(g, c, 0)
        one = run_kernels(g, alone, 0)
    assert_same_bits(whole["dz"][:1], one["dz"], "dz of image 0")
    assert_same_bits(whole["p"][:1], one["p"], "p of image 0")


@pytest.mark.parametrize("shape", [(2, 5, 1, 1), (3, 4, 2, 3), (2, 16, 4, 12), (1, 3, 5, 7)], ids=cases.case_id)
@sweeps("tpspp_global_avgpool_bwd")
def test_global_avgpool_bwd_is_the_broadcast_quotient(cuda, shape):
    N, C, H, W = shape
    gcpu = torch.randn((N, C), generator=torch.Generator().manual_seed(3))
    with GA.guarded(cuda) as g:
        dx = ops.global_avgpool_bwd(g.input(gcpu), (H, W))
        g.check(dx)
    want = (gcpu / torch.tensor(float(H * W))).view(N, C, 1, 1).expand(N, C, H, W).contiguous()
    assert_same_bits(dx.cpu(), want, "global_avgpool_bwd")
    x = torch.randn(shape, generator=torch.Generator().manual_seed(4)).to(cuda).requires_grad_(True)
    ops.global_avgpool_autograd(x).backward(gcpu.to(cuda))
    assert_same_bits(x.grad, dx, "global_avgpool_autograd")


# ---- 2. the convolution backward kernels with 1 and 3 input channels ----------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (32, 100)], ids=["5x7", "32x100"])
@pytest.mark.parametrize("cin", [1, 3])
def test_conv_backward_with_few_input_channels_against_float64(cuda, cin, hw):
    g0 = torch.Generator().manual_seed(17 + cin)
    N, cout = 3, 64
    x = torch.randn((N, cin, *hw), generator=g0)
    w = torch.randn((cout, cin, 3, 3), generator=g0) / 3
    dy = torch.randn((N, cout, *hw), generator=g0)

    def ref(dtype, device):
        xr = x.to(device).to(dtype).requires_grad_(True)
        wr = w.to(device).to(dtype).requires_grad_(True)
        F.conv2d(xr, wr, None, 1, 1).backward(dy.to(device).to(dtype))
        return dict(dx=xr.grad.cpu(), dw=wr.grad.cpu())

    with GA.guarded(cuda) as g:
        x_, w_, dy_ = g.input(x), g.input(w), g.input(dy)
        dw, _ = ops.conv2d_bwd_weight([x_], dy_, 3, (1, 1), relu=False, want_bias=False)
        dx = ops.conv2d_bwd_data(dy_, w_, [x_], (1, 1), relu=False)[0]
        g.check((dw, dx))
    check(f"conv bwd Cin={cin} {hw[0]}x{hw[1]}", dict(dx=dx, dw=dw), ref(torch.float64, "cpu"), ref(torch.float32, cuda))


# ---- 3. the localisation network -------------------------------------------------------------------------------------------
def randomize_bn(m, seed):
    """tests/test_gpu_backbone_train.py's recipe: non-trivial affine parameters and running statistics."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in m.modules():
            if isinstance(bn, nn.BatchNorm2d):
                c = bn.num_features
                bn.weight.copy_(1 + 0.3 * torch.randn(c, generator=g))
                bn.bias.copy_(0.2 * torch.randn(c, generator=g))
                bn.running_mean.copy_(0.1 * torch.randn(c, generator=g))
                bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
                bn.num_batches_tracked.fill_(3)
    return m


def loc_net(channels, seed=0):
    """A LocalizationNetwork whose fc2 weight is not the constructor's zero (every gradient below it would be exactly 0)."""
    torch.manual_seed(seed)
    m = randomize_bn(LocalizationNetwork(20, channels), seed + 100)
    with torch.no_grad():
        m.localization_fc2.weight.copy_(0.05 * torch.randn(m.localization_fc2.weight.shape))
    return m.train()


def loc_step(m, img, gout, hip):
    x = img.clone().requires_grad_(True)
    out = m._forward_train_hip(x) if hip else m._forward_torch(x)
    out.backward(gout)
    res = {"ctrl": out.detach(), "d_img": x.grad}
    res.update({"d_" + k: p.grad for k, p in m.named_parameters()})
    res.update({k: b for k, b in m.named_buffers() if not k.endswith("num_batches_tracked")})
    counters = [int(b) for k, b in m.named_buffers() if k.endswith("num_batches_tracked")]
    return {k: v.detach().cpu() for k, v in res.items()}, counters


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("hw", [(32, 100), (32, 64), (16, 24)], ids=["32x100", "32x64", "16x24"])
@pytest.mark.parametrize("channels", [1, 3])
def test_localisation_network_against_its_float64_composition(cuda, channels, hw, N):
    g0 = torch.Generator().manual_seed(N * 100 + hw[1] + channels)
    img = torch.randn((N, channels, *hw), generator=g0)
    gout = torch.randn((N, 20, 2), generator=g0)
    base = loc_net(channels)
    want, n64 = loc_step(copy.deepcopy(base).double(), img.double(), gout.double(), False)
    lib32, _ = loc_step(copy.deepcopy(base).to(cuda), img.to(cuda), gout.to(cuda), False)
    mh = copy.deepcopy(base).to(cuda)
    with GA.guarded(cuda) as g:
        got, nh = loc_step(mh, g.input(img), g.input(gout), True)
        g.check()
    assert nh == n64 == [4, 4, 4, 4]
    for k in want:
        if k.startswith("d_"):
            assert want[k].abs().max() > 0, f"{k}: the reference gradient is zero, the comparison shows nothing"
    check(f"loc C={channels} {hw[0]}x{hw[1]} N={N}", got, want, lib32)


def test_a_single_value_per_channel_raises_pytorchs_message(cuda):
    m = loc_net(1).to(cuda)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m._forward_train_hip(torch.randn((1, 1, 8, 8), device=cuda))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m._forward_torch(torch.randn((1, 1, 8, 8), device=cuda))


# ---- 4. the module ------------------------------------------------------------------------------------------------------
def preprocessor(channels=1, seed=0):
    torch.manual_seed(seed)
    m = randomize_bn(TPSPreprocessor(20, (32, 100), (32, 100), channels), seed + 100)
    with torch.no_grad():
        m.LocalizationNetwork.localization_fc2.weight.copy_(0.01 * torch.randn(40, 256))
    return m


def image(N, channels, seed):
    return torch.rand((N, channels, 32, 100), generator=torch.Generator().manual_seed(seed))


def test_no_library_layer_runs(cuda, monkeypatch):
    m = preprocessor(3).to(cuda).train().set_train_backend("hip")
    x = image(3, 3, 1).to(cuda).requires_grad_(True)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the HIP training path")
        return f

    for name in ("conv2d", "batch_norm", "max_pool2d", "adaptive_avg_pool2d", "linear", "relu", "grid_sample"):
        monkeypatch.setattr(F, name, refuse(f"F.{name}"))
    out = m(x)
    out.square().mean().backward()
    assert torch.isfinite(out).all() and x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
    with pytest.raises(AssertionError, match="called on the HIP training path"):
        m.set_train_backend("torch")(x)


def test_the_composition_warning_is_logged_on_the_torch_route_only(cuda, caplog):
    x = image(2, 1, 2).to(cuda)
    with caplog.at_level("WARNING", logger="tps_pp_amd"):
        preprocessor().to(cuda).train().set_train_backend("hip")(x)
        assert "PyTorch composition" not in caplog.text
        preprocessor().to(cuda).train()(x)
        assert "PyTorch composition" in caplog.text


def sgd_run(cuda, mode, steps, io=None, lr=0.01):
    m = preprocessor(1).to(cuda).train().set_train_backend(mode).set_train_io_dtype(io)
    x = image(4, 1, 13).to(cuda)
    target = image(4, 1, 14).to(cuda)
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = (m(x).float() - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, {k: v.detach().clone() for k, v in list(m.named_parameters()) + list(m.named_buffers())}


def test_five_sgd_steps_track_the_torch_backend(cuda):
    """The two backends differ by fp32 rounding in every step; five steps keep that difference at rounding's size only while
    the steps descend (a step size at which the loss bounces amplifies any perturbation, PyTorch's own included), so the
    reference run must descend monotonically.  Then: parameters and buffers within 1e-3 (tests/test_gpu_backbone_train.py's
    bound for the same kind of run), losses within 1e-4."""
    lt, final_t = sgd_run(cuda, "torch", 5)
    lh, final_h = sgd_run(cuda, "hip", 5)
    print("losses torch", lt, "hip", lh)
    print("largest deviation", max((rel(final_h[k], t), k) for k, t in final_t.items() if t.dtype != torch.int64))
    assert all(b < a for a, b in zip(lt, lt[1:])), lt
    for k, t in final_t.items():
        h = final_h[k]
        if t.dtype == torch.int64:
            assert torch.equal(t, h), k
        else:
            assert rel(h, t) <= 1e-3, (k, rel(h, t))
    assert all(abs(a - b) <= 1e-4 * abs(a) for a, b in zip(lt, lh))


def test_hip_backend_with_bf16_images_runs_and_descends(cuda):
    m = preprocessor(1).to(cuda).train().set_train_backend("hip").set_train_io_dtype(torch.bfloat16)
    assert m(image(2, 1, 3).to(cuda)).dtype == torch.bfloat16
    losses, final = sgd_run(cuda, "hip", 6, io=torch.bfloat16)
    print("bf16 losses", losses)
    assert all(torch.isfinite(v).all() for v in final.values() if v.is_floating_point())
    assert losses[-1] < losses[0]


def test_eval_output_has_the_same_bits_before_and_after_the_switch(cuda):
    m = preprocessor(3).to(cuda).eval()
    x = image(3, 3, 5).to(cuda)
    with torch.no_grad():
        before = m(x)
        m.set_train_backend("hip")
        after = m(x)
        m.train()
        m(x)                                                       # a training forward in between (moves running statistics)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m2 = preprocessor(3).to(cuda).eval()
    with torch.no_grad():
        untouched = m2(x)
    assert_same_bits(before, after, "eval output across the switch")
    assert_same_bits(before, untouched, "eval output of a module that never switched")
    assert set(state) == set(m2.state_dict())


def test_eval_mode_module_with_an_input_that_requires_grad_uses_running_statistics(cuda, monkeypatch):
    m = preprocessor(1).to(cuda).eval().set_train_backend("hip")
    buffers = {k: v.clone() for k, v in m.named_buffers()}
    seen = []
    real = ops.bn_pool2x2_bwd_data

    def spy(dp, z, stats, gamma, beta, sums=None, train=True):
        seen.append((bool(train), sums))
        return real(dp, z, stats, gamma, beta, sums, train)

    monkeypatch.setattr(ops, "bn_pool2x2_bwd_data", spy)
    for p in m.parameters():
        p.requires_grad_(False)
    x = image(2, 1, 6).to(cuda).requires_grad_(True)
    out = m(x)
    assert out.grad_fn is not None
    out.square().mean().backward()
    assert len(seen) == 3 and all(t is False and s is None for t, s in seen)   # frozen affine: no reduction either
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    for k, v in m.named_buffers():
        assert torch.equal(v, buffers[k]), k
    # the same gradient from the PyTorch composition
    x2 = x.detach().clone().requires_grad_(True)
    m.set_train_backend("torch")(x2).square().mean().backward()
    assert rel(x.grad, x2.grad) <= 1e-4, rel(x.grad, x2.grad)


# ---- 5. the recogniser ------------------------------------------------------------------------------------------------------
def crnn_step(cuda, **backends):
    torch.manual_seed(0)                 # whatever the golden state does not cover is initialised alike in every run
    m = build_detector(CC.models()["crnn_tps"]).eval()
    sd = CC.state(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    with torch.no_grad():
        m.preprocessor.LocalizationNetwork.localization_fc2.weight.copy_(
            0.01 * torch.randn((40, 256), generator=torch.Generator().manual_seed(7)))
    m = m.to(cuda).train().set_train_backend("torch", **backends)
    img = torch.from_numpy(CC.images()).to(cuda)
    metas = [dict(resize_shape=(32, 100, 1), text=s) for s in CC.TEXTS]
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    loss = m(img, metas, return_loss=True)["loss_ctc"]
    opt.zero_grad()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.preprocessor.named_parameters()}
    opt.step()
    return loss.item(), grads, {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_one_sgd_step_of_crnn_tps_against_the_torch_backends(cuda):
    """The step's results -- the loss and every parameter and buffer after it -- on the HIP backends against the same step on
    "torch": the loss within 1e-5, the state within 1e-3 (tests/test_gpu_backbone_train.py's bound for a state after SGD).
    The preprocessor's raw gradients are printed next to the deviation between two runs of the "torch" step itself and not
    held to a bar here: two "torch" runs of this very step were seen 2e-2 apart in them (relative L2, 5e-4 at best) on an
    MI355X, the "hip" step 1.8e-2 from a "torch" run -- presumably the smooth golden images: their pooling windows hold
    near-equal activations, and where a gradient goes then follows the last bits of a convolution that the library may
    compute with another algorithm from run to run.  What the HIP localisation network does with a given upstream gradient
    is held to float64 above."""
    lt, gt, st = crnn_step(cuda)
    _, gt2, _ = crnn_step(cuda)
    lh, gh, sh = crnn_step(cuda, preprocessor="hip", decoder="hip", loss="hip")
    print(f"loss_ctc torch {lt:.6f} hip {lh:.6f}")
    for k, t in gt.items():
        print(f"d {k}: hip against torch {rel(gh[k], t):.3e}, torch against torch {rel(gt2[k], t):.3e}")
        assert t.abs().max() > 0 and torch.isfinite(gh[k]).all() and gh[k].abs().max() > 0, k
    assert abs(lt - lh) <= 1e-5 * abs(lt)
    for k, t in st.items():
        if t.dtype == torch.int64:
            assert torch.equal(t, sh[k]), k
        else:
            assert rel(sh[k], t) <= 1e-3, (k, rel(sh[k], t))
