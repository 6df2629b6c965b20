"""-m gpu: backward of the fused convolution (tpspp_conv_bwd.hip) layer by layer against float64 PyTorch on the CPU, and
TPS_PP / NRTR training with `set_train_backend("hip")` against the float64 composition of the same module.

Bar of the layer tests: every element |g - g64| <= 4e-6 * A, A the same gradient computed in float64 from absolute
values (operands and dZ): about ten times the error of an fp32 MFMA accumulation chain.  Y comes from the HIP forward and
dZ = dY * [Y > 0] is formed from it exactly, so the reference and the kernels agree on the ReLU mask."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from tps_pp_amd import TPS_PP, ops

pytestmark = pytest.mark.gpu

# (name, sources [(C, H, W, uh, uw)], Cout, K, stride, relu, bias, N)
_S = 64
MODULE_LAYERS = [
    # ResNet45v2 wiring (tps_pp.py:537-552) and MSFA (tps_pp.py:126-131,149-169) at N = 4
    ("down0", [(32, 32, 128, 1, 1)], _S, 1, 1),
    ("down2", [(64, 16, 64, 1, 1)], _S, 1, 1),
    ("down0_1", [(64, 32, 128, 1, 1)], _S, 3, 2),
    ("down_feat", [(64, 32, 128, 1, 1), (64, 32, 128, 1, 1), (64, 16, 64, 2, 2)], _S, 1, 1),
    ("enc0", [(64, 16, 64, 1, 1)] * 3, _S, 3, 1),
    ("enc1", [(64, 16, 64, 1, 1)], _S, 3, 2),
    ("enc2", [(64, 8, 32, 1, 1)], _S, 3, 2),
    ("enc3", [(64, 4, 16, 1, 1)], _S, 3, (2, 1)),
    ("dec0", [(64, 2, 16, 2, 1)], _S, 3, 1),
    ("dec1", [(64, 4, 16, 2, 2)], _S, 3, 1),
    ("dec2", [(64, 8, 32, 2, 2)], _S, 3, 1),
    ("dec3", [(64, 16, 64, 1, 1)], _S, 3, 1),
    # the ResNet45 wiring's own layers (down1 / down1_1 repeat down0 / down0_1 above)
    ("v1.down0", [(32, 32, 128, 1, 1)], _S, 3, 2),
    ("v1.down1", [(32, 16, 64, 1, 1)], _S, 1, 1),
]
RAGGED = [
    # odd sizes, Cin = 20, Cout = 40, N = 1 / 3, no bias, no activation, 1 - 3 sources with (1,1) / (2,1) / (2,2)
    ("3x3.s2.odd", [(20, 7, 13, 1, 1)], 40, 3, 2, 1, True, 3),
    ("3x3.s21.nobias.noact", [(20, 9, 11, 1, 1)], 40, 3, (2, 1), 0, False, 1),
    ("3x3.s1.odd", [(20, 9, 13, 1, 1)], 40, 3, 1, 1, True, 3),
    ("1x1.s2.unread", [(20, 5, 6, 1, 1)], 40, 1, 2, 1, True, 3),
    ("1x1.s12", [(32, 6, 9, 1, 1)], 40, 1, (1, 2), 0, True, 1),
    ("3x3.two.up21", [(8, 6, 10, 2, 1), (20, 12, 10, 1, 1)], 40, 3, 1, 1, True, 3),
    ("3x3.three.up22.s2", [(8, 3, 5, 2, 2), (12, 6, 10, 1, 1), (4, 6, 5, 1, 2)], 40, 3, 2, 1, False, 3),
    ("1x1.two.noact", [(32, 5, 7, 1, 1), (64, 5, 7, 1, 1)], 40, 1, 1, 0, False, 1),
    ("1x1.up22.s2", [(32, 3, 4, 2, 2)], 24, 1, 2, 1, True, 3),
    ("3x3.up22.s21", [(20, 4, 7, 2, 2)], 40, 3, (2, 1), 1, True, 1),
]
CASES = [(n, s, co, k, st, 1, True, 4) for n, s, co, k, st in MODULE_LAYERS] + RAGGED

# Every distinct convolution of ResNetABI_v2_large(strides=[2, 1, 2, 1, 2]) on a 32x128 image -- what the backbone's "hip"
# train backend sends through these kernels (tests/test_memory_safety_host.py holds the table to a constructed model):
# several 64-channel tiles (blockIdx.y > 0), a Cout loop of up to 8 x 64, Kf up to 4608, Cin = 3 and the Cout = 32 layers.
# (name, Cin, Cout, K, stride, H, W, bias)
BACKBONE_LAYERS = [
    ("conv1", 3, 32, 3, (1, 1), 32, 128, True),
    ("layer1.0.conv1", 32, 32, 1, (1, 1), 32, 128, False),
    ("layer1.0.conv2", 32, 32, 3, (2, 2), 32, 128, False),
    ("layer1.0.downsample", 32, 32, 1, (2, 2), 32, 128, False),
    ("layer1.1.conv1", 32, 32, 1, (1, 1), 16, 64, False),
    ("layer1.1.conv2", 32, 32, 3, (1, 1), 16, 64, False),
    ("layer2.0.conv1", 32, 64, 1, (1, 1), 16, 64, False),
    ("layer2.0.conv2", 64, 64, 3, (1, 1), 16, 64, False),
    ("layer2.1.conv1", 64, 64, 1, (1, 1), 16, 64, False),
    ("layer3.0.conv1", 64, 128, 1, (1, 1), 16, 64, False),
    ("layer3.0.conv2", 128, 128, 3, (2, 2), 16, 64, False),
    ("layer3.0.downsample", 64, 128, 1, (2, 2), 16, 64, False),
    ("layer3.1.conv1", 128, 128, 1, (1, 1), 8, 32, False),
    ("layer3.1.conv2", 128, 128, 3, (1, 1), 8, 32, False),
    ("layer4.0.conv1", 128, 256, 1, (1, 1), 8, 32, False),
    ("layer4.0.conv2", 256, 256, 3, (1, 1), 8, 32, False),
    ("layer4.1.conv1", 256, 256, 1, (1, 1), 8, 32, False),
    ("layer5.0.conv1", 256, 512, 1, (1, 1), 8, 32, False),
    ("layer5.0.conv2", 512, 512, 3, (2, 2), 8, 32, False),
    ("layer5.0.downsample", 256, 512, 1, (2, 2), 8, 32, False),
    ("layer5.1.conv1", 512, 512, 1, (1, 1), 4, 16, False),
    ("layer5.1.conv2", 512, 512, 3, (1, 1), 4, 16, False),
]
# one ragged case with several channel tiles on both sides: odd map, stride (2, 1), Cin and Cout no multiple of 64
BACKBONE_RAGGED = ("ragged.200to136", 200, 136, 3, (2, 1), 7, 13, True)
# relu = 0 with dZ handed over as dY is how the backbone calls these layers (the BatchNorm kernels have applied the mask:
# include/tpspp.h); the ReLU-masked form as well; N = 3 and N = 5
BACKBONE_CASES = [(f"bb.{n}.N{N}.{'relu' if relu else 'dz'}", [(ci, H, W, 1, 1)], co, k, st, relu, bias, N)
                  for n, ci, co, k, st, H, W, bias in BACKBONE_LAYERS + [BACKBONE_RAGGED] for N in (3, 5) for relu in (0, 1)]


def make(spec, cout, k, bias, N, seed):
    g = torch.Generator().manual_seed(seed)
    srcs = [torch.randn((N, C, H, W), generator=g) for C, H, W, _, _ in spec]
    cin = sum(s[0] for s in spec)
    w = torch.randn((cout, cin, k, k), generator=g) * (1.0 / np.sqrt(cin * k * k))
    b = torch.randn((cout,), generator=g) * 0.1 if bias else None
    return srcs, w, b, g


def hip_forward(cuda, srcs, spec, w, b, stride, relu):
    ds = [s.to(cuda) for s in srcs]
    entries = [(d, uh, uw) for d, (_, _, _, uh, uw) in zip(ds, spec)]
    cw = ops.prep_conv_weight_device(w.to(cuda), None if b is None else b.to(cuda), [s[0] for s in spec])
    return entries, ops.conv2d(entries, cw, stride, relu=bool(relu))


def ref64(srcs, spec, w, dz, stride, k):
    """dX_i, dW, db in float64 by PyTorch's autograd on the CPU, upsampling by repetition (exact)."""
    xs = [s.double().requires_grad_(True) for s in srcs]
    wd = w.double().requires_grad_(True)
    X = torch.cat([x.repeat_interleave(uh, 2).repeat_interleave(uw, 3) for x, (_, _, _, uh, uw) in zip(xs, spec)], 1)
    st = (stride, stride) if isinstance(stride, int) else stride
    Z = F.conv2d(X, wd, None, st, (k - 1) // 2)
    grads = torch.autograd.grad(Z, xs + [wd], dz)
    return list(grads[:-1]), grads[-1], dz.sum((0, 2, 3))


def fwd64(srcs, spec, w, b, stride, k, relu):
    X = torch.cat([x.double().repeat_interleave(uh, 2).repeat_interleave(uw, 3)
                   for x, (_, _, _, uh, uw) in zip(srcs, spec)], 1)
    st = (stride, stride) if isinstance(stride, int) else stride
    z = F.conv2d(X, w.double(), None if b is None else b.double(), st, (k - 1) // 2)
    return z.clamp_min(0) if relu else z


def check(name, got, want, bound):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - want).abs()
    bad = err > 4e-6 * bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} elements over the bar, worst err {err.max().item():.3e}, "
                           f"bound there {(4e-6 * bound).flatten()[err.argmax()].item():.3e}")


def run_layer(cuda, spec, cout, k, stride, relu, bias, N, seed=0):
    srcs, w, b, g = make(spec, cout, k, bias, N, seed)
    entries, y = hip_forward(cuda, srcs, spec, w, b, stride, relu)
    dy = torch.randn(tuple(y.shape), generator=g)
    dyd, wd = dy.to(cuda), w.to(cuda)
    dx = ops.conv2d_bwd_data(dyd, wd, entries, stride, y=y, relu=bool(relu))
    dw, db = ops.conv2d_bwd_weight(entries, dyd, k, stride, y=y, relu=bool(relu), want_bias=bias)
    torch.cuda.synchronize()
    # the forward on the device-built weight layouts (tpspp_conv2d_prep_weight) against float64: same bar
    check("forward Y", y, fwd64(srcs, spec, w, b, stride, k, relu), fwd64([s.abs() for s in srcs], spec, w.abs(),
                                                                       None if b is None else b.abs(), stride, k, False))
    mask = (y.cpu() > 0).double() if relu else torch.ones(tuple(y.shape), dtype=torch.float64)
    dz = dy.double() * mask
    rx, rw, rb = ref64(srcs, spec, w, dz, stride, k)
    ax, aw, ab = ref64([s.abs() for s in srcs], spec, w.abs(), dz.abs(), stride, k)
    return dict(srcs=srcs, entries=entries, y=y, dyd=dyd, wd=wd, dx=dx, dw=dw, db=db, rx=rx, rw=rw, rb=rb, ax=ax,
                aw=aw, ab=ab)


@pytest.mark.parametrize("name,spec,cout,k,stride,relu,bias,N", CASES + BACKBONE_CASES,
                         ids=[c[0] for c in CASES + BACKBONE_CASES])
def test_layer_gradients_against_float64(cuda, name, spec, cout, k, stride, relu, bias, N):
    r = run_layer(cuda, spec, cout, k, stride, relu, bias, N)
    for i, (g, want, a) in enumerate(zip(r["dx"], r["rx"], r["ax"])):
        check(f"{name} dX_{i}", g, want, a)
    check(f"{name} dW", r["dw"], r["rw"], r["aw"])
    if bias:
        check(f"{name} db", r["db"], r["rb"], r["ab"])
    else:
        assert r["db"] is None


def test_unread_positions_are_exact_zeros(cuda):
    """1x1 at stride 2: odd rows and columns feed no output; 3x3 at stride 2 on an odd size reads every row."""
    r = run_layer(cuda, [(20, 5, 7, 1, 1)], 40, 1, 2, 1, True, 3, seed=5)
    g = r["dx"][0].cpu()
    assert torch.count_nonzero(g[:, :, 1::2, :]) == 0 and torch.count_nonzero(g[:, :, :, 1::2]) == 0
    assert torch.count_nonzero(g[:, :, ::2, ::2]) > 0


def test_needs_input_grad_is_honoured(cuda, monkeypatch):
    """No data-gradient launch when no source needs a gradient, no weight GEMM for a frozen layer (bias only: the
    reduction alone, same bits as the full call)."""
    calls = []
    real_data, real_weight = ops.conv2d_bwd_data, ops.conv2d_bwd_weight

    def data(*a, **k):
        calls.append(("data", tuple(k.get("need") or ())))
        return real_data(*a, **k)

    def weight(*a, **k):
        calls.append(("weight", k.get("want_weight"), k.get("want_bias")))
        return real_weight(*a, **k)

    monkeypatch.setattr(ops, "conv2d_bwd_data", data)
    monkeypatch.setattr(ops, "conv2d_bwd_weight", weight)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 16, 6, 10), generator=g).to(cuda).requires_grad_(True)
    x2 = torch.randn((2, 8, 6, 10), generator=g).to(cuda)                    # a second source without gradient
    w = (0.2 * torch.randn((24, 24, 3, 3), generator=g)).to(cuda)
    b = torch.randn((24,), generator=g).to(cuda)

    # frozen layer: the data gradient of the one source that needs it, no weight-gradient launch
    ops.conv2d_autograd([x, x2], w, b, 2, relu=True).square().sum().backward()
    assert calls == [("data", (True, False))] and x.grad is not None
    # input without gradient, trainable weight and bias: no data-gradient launch
    calls.clear()
    wt, bt = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ops.conv2d_autograd([x.detach(), x2], wt, bt, 2, relu=True).square().sum().backward()
    assert calls == [("weight", True, True)]
    # frozen weight, trainable bias: the bias reduction alone, bit for bit the full call's db
    calls.clear()
    bb = b.clone().requires_grad_(True)
    ops.conv2d_autograd([x.detach(), x2], w, bb, 2, relu=True).square().sum().backward()
    assert calls == [("weight", False, True)]
    assert torch.equal(bb.grad, bt.grad)


def test_bitwise_reproducible_across_calls_and_streams(cuda):
    spec = [(64, 16, 64, 1, 1), (64, 16, 64, 1, 1), (64, 8, 32, 2, 2)]
    r = run_layer(cuda, spec, 64, 3, 1, 1, True, 8, seed=11)

    def once():
        dx = ops.conv2d_bwd_data(r["dyd"], r["wd"], r["entries"], 1, y=r["y"], relu=True)
        dw, db = ops.conv2d_bwd_weight(r["entries"], r["dyd"], 3, 1, y=r["y"], relu=True)
        return dx, dw, db

    a = once()
    b = once()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = once()
    torch.cuda.synchronize()
    for other in (b, c):
        assert all(torch.equal(p, q) for p, q in zip(a[0], other[0]))
        assert torch.equal(a[1], other[1]) and torch.equal(a[2], other[2])
    assert all(torch.equal(p, q) for p, q in zip(a[0], r["dx"]))
    assert torch.equal(a[1], r["dw"])


def test_k_encoder0_large_batch_several_slices(cuda):
    """k_encoder.0 at N = 32: 32768 reduction terms, cut into several split-K slices."""
    spec = [(64, 16, 64, 1, 1)] * 3
    dims = [v for s in spec for v in s]
    need = ops.conv2d_bwd_weight_workspace_floats(dims, 32, 64, 3, 16, 64)
    assert need >= 2 * 64 * (192 * 9 + 1)            # more than one slice
    r = run_layer(cuda, spec, 64, 3, 1, 1, True, 32, seed=21)
    for i, (g, want, a) in enumerate(zip(r["dx"], r["rx"], r["ax"])):
        check(f"enc0 N=32 dX_{i}", g, want, a)
    check("enc0 N=32 dW", r["dw"], r["rw"], r["aw"])
    check("enc0 N=32 db", r["db"], r["rb"], r["ab"])


# ---- module level ---------------------------------------------------------------------------------------------------
def synth_module(variant):
    m = TPS_PP(variant=variant)
    sd = cases.synth_state(m.state_dict(), 4, cases.tpspp_state_rule, cases.TPSPP_KEEP)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


def grid64(at, ctrl, score):
    """Attention_Enhanced_TPS.build_P_prime (tps_pp.py:467-496) composed in PyTorch."""
    N, n, _ = score.shape
    P = torch.from_numpy(np.asarray(at.P)).to(score.dtype)[None].expand(N, -1, -1)
    ph = at.P_hat[None] * (score * at.thela + 1)
    ph = torch.cat([torch.ones((N, n, 1), dtype=score.dtype), P, ph], dim=2)
    T = torch.bmm(at.hat_C[None].expand(N, -1, -1), torch.cat([ctrl, torch.zeros((N, 3, 2), dtype=ctrl.dtype)], 1))
    return torch.bmm(ph, T)


def forward64(m64, x, outs, hw):
    cp, sc, fg = m64._regress_torch(x, outs)
    g = grid64(m64.atten_tps, cp, sc).reshape(x.shape[0], hw[0], hw[1], 2)
    o0 = F.grid_sample(fg, g, padding_mode="border", align_corners=True)
    o1 = F.grid_sample(x, g, padding_mode="border", align_corners=True)
    return o0, o1


# Gradients of a whole TPS_PP step against its float64 composition: fixed bars per parameter group.  1e-4 (the issue's
# bar) is not reachable in fp32 by this module with EITHER backend: the layers that stay PyTorch in both (CBAM, DGAB, the
# TPE's linear layers and tanh score) and the warp leave an fp32 floor on every gradient that flows through them.
# Measured relative L2 errors (both wirings, "torch" backend / "hip" backend):
#   down*, k_encoder.*, localization_fc*      0.6-6.8e-5 / 0.7-7.3e-5
#   x, outs (through the warp's fp32 grid)    5.3-11.0e-5 / 5.3-11.0e-5
#   k_decoder.* (feed DGAB and the score)     4.8-8.1e-4 / 4.7-8.0e-4
#   TPE p_linear / feat_linear / DGAB         0.9-19e-4  / 0.9-19e-4
#   CBAM                                      0.5-6.2e-3 / 0.5-6.2e-3
# The bars below are about three times the measured floor of each group; the kernels themselves are held to the
# layer bar (4e-6 x the absolute-value bound) INSIDE the module by test_module_conv_gradients_hold_the_layer_bar.
GROUP_BARS = [
    (lambda k: k.startswith("MSFA.conv.atten."), 2e-2),
    (lambda k: k.startswith("MSFA.conv.k_decoder."), 3e-3),
    (lambda k: k.startswith("TPE.") and not k.startswith("TPE.localization_"), 6e-3),
    (lambda k: True, 3e-4),          # down*, k_encoder.*, TPE.localization_*, x, outs
]


def group_bar(name):
    return next(b for match, b in GROUP_BARS if match(name))


def module_step(cuda, variant, g0, g1):
    m = synth_module(variant).to(cuda).train().set_train_backend("hip")
    inp = cases.g4_inputs(variant)
    x = torch.from_numpy(inp["x"]).to(cuda).requires_grad_(True)
    outs = [torch.from_numpy(o).to(cuda).requires_grad_(True) for o in inp["outs"]]
    res = m(x, outs)
    ((res["output"] * g0.to(cuda)).sum() + (res["mp_img"] * g1.to(cuda)).sum()).backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads.update({"x": x.grad, "outs[0]": outs[0].grad, "outs[1]": outs[1].grad})
    return m, x.detach(), [o.detach() for o in outs], res, grads


def head_grads(variant):
    hw = (16, 64)
    g = torch.Generator().manual_seed(17)
    return (torch.randn((cases.G4_N, 64) + hw, generator=g), torch.randn((cases.G4_N, 64) + hw, generator=g))


@pytest.mark.parametrize("variant", ["ResNet45v2", "ResNet45"])
def test_module_gradients_against_float64(cuda, variant):
    """Every parameter's gradient and those of x and outs with set_train_backend("hip") against the module's own
    composition in float64 on the CPU (`_regress_torch` + F.grid_sample on build_P_prime), relative L2 within the fixed
    bar of its group (GROUP_BARS); the forward output within 1e-4 of the eval path."""
    g0, g1 = head_grads(variant)
    m, x, outs, res, gh = module_step(cuda, variant, g0, g1)
    m64 = synth_module(variant).double().train()
    inp = cases.g4_inputs(variant)
    x64 = torch.from_numpy(inp["x"]).double().requires_grad_(True)
    outs64 = [torch.from_numpy(o).double().requires_grad_(True) for o in inp["outs"]]
    o0, o1 = forward64(m64, x64, outs64, m.rectified_img_size)
    ((o0 * g0.double()).sum() + (o1 * g1.double()).sum()).backward()
    g64 = {k: p.grad for k, p in m64.named_parameters()}
    g64.update({"x": x64.grad, "outs[0]": outs64[0].grad, "outs[1]": outs64[1].grad})
    bad = {}
    for k, want in g64.items():
        assert gh[k] is not None and torch.isfinite(gh[k]).all(), k
        if want.norm() == 0:
            continue
        e = ((gh[k].detach().cpu().double() - want).norm() / want.norm()).item()
        if e > group_bar(k):
            bad[k] = (e, group_bar(k))
    assert not bad, bad
    with torch.no_grad():
        ref = m.eval()(x, outs)
    assert (ref["output"] - res["output"].detach()).abs().max() <= 1e-4
    assert (ref["mp_img"] - res["mp_img"].detach()).abs().max() <= 1e-4


@pytest.mark.parametrize("variant", ["ResNet45v2", "ResNet45"])
def test_module_conv_gradients_hold_the_layer_bar(cuda, variant, monkeypatch):
    """Inside a whole TPS_PP training step, every convolution's dW, db and per-source dX against float64 computed from
    the fp32 tensors that convolution actually saw (its sources, weight, bias, the gradient reaching its output and its
    own Y for the ReLU mask): each element within 4e-6 x the absolute-value bound.  Deterministic: no library baseline,
    no dependence on the fp32 floor of the PyTorch layers around the convolutions."""
    recs = []
    real = ops.conv2d_autograd

    def spy(srcs, weight, bias, stride=(1, 1), relu=True, cw=None):
        views, spec = [], []
        for e in srcs:
            t, uh, uw = (e, 1, 1) if isinstance(e, torch.Tensor) else e
            views.append(t.view_as(t))           # a node of its own: its gradient is this convolution's share
            spec.append((t.shape[1], t.shape[2], t.shape[3], int(uh), int(uw)))
        y = real([(v, s[3], s[4]) for v, s in zip(views, spec)], weight, bias, stride, relu, cw)
        r = dict(srcs=[v.detach().clone() for v in views], spec=spec, w=weight.detach().clone(), param_w=weight,
                 param_b=bias, b=None if bias is None else bias.detach().clone(), stride=stride,
                 k=weight.shape[-1], y=y.detach().clone(), dy=None, dx=[None] * len(views))
        y.register_hook(lambda g: r.__setitem__("dy", g.detach().clone()))
        for i, v in enumerate(views):
            if v.requires_grad:
                v.register_hook(lambda g, i=i: r["dx"].__setitem__(i, g.detach().clone()))
        recs.append(r)
        return y

    monkeypatch.setattr(ops, "conv2d_autograd", spy)
    g0, g1 = head_grads(variant)
    module_step(cuda, variant, g0, g1)
    torch.cuda.synchronize()
    assert len(recs) == (14 if variant == "ResNet45v2" else 11)
    for j, r in enumerate(recs):
        name = f"conv {j}"
        srcs, spec, k, st = [t.cpu() for t in r["srcs"]], r["spec"], r["k"], r["stride"]
        check(f"{name} forward Y", r["y"], fwd64(srcs, spec, r["w"].cpu(), None if r["b"] is None else r["b"].cpu(), st,
                                                 k, True),
              fwd64([t.abs() for t in srcs], spec, r["w"].cpu().abs(), None if r["b"] is None else r["b"].cpu().abs(),
                    st, k, False))
        dz = r["dy"].cpu().double() * (r["y"].cpu() > 0).double()
        rx, rw, rb = ref64(srcs, spec, r["w"].cpu(), dz, st, k)
        ax, aw, ab = ref64([t.abs() for t in srcs], spec, r["w"].cpu().abs(), dz.abs(), st, k)
        check(f"{name} dW", r["param_w"].grad, rw, aw)
        check(f"{name} db", r["param_b"].grad, rb, ab)
        for i, (g, want, a) in enumerate(zip(r["dx"], rx, ax)):
            if g is not None:
                check(f"{name} dX_{i}", g, want, a)
        assert any(g is not None for g in r["dx"]), name


def test_sgd_steps_track_the_torch_backend(cuda):
    inp = cases.g4_inputs("ResNet45v2")
    x = torch.from_numpy(inp["x"]).to(cuda)
    outs = [torch.from_numpy(o).to(cuda) for o in inp["outs"]]
    losses = {}
    for mode in ("torch", "hip"):
        m = synth_module("ResNet45v2").to(cuda).train().set_train_backend(mode)
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        seq = []
        for _ in range(3):
            opt.zero_grad()
            res = m(x, outs)
            loss = res["output"].square().mean() + res["mp_img"].square().mean()
            loss.backward()
            opt.step()
            seq.append(loss.item())
        losses[mode] = seq
    t, h = np.array(losses["torch"]), np.array(losses["hip"])
    assert np.all(np.abs(h - t) <= 1e-3 * np.abs(t)), losses
    assert t[-1] != t[0]                               # the steps did change the weights


def test_nrtr_forward_train_with_the_hip_backend(cuda):
    import tps_pp_amd as P
    torch.manual_seed(0)
    m = P.build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                         strides=[2, 1, 2, 1, 2]),
                              tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                              decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                              label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
                              max_seq_len=8))
    m = m.to(cuda).train().set_train_backend("hip")
    assert m.tpsnet.train_backend == "hip"
    img = torch.randn((2, 3, 32, 128), device=cuda)
    metas = [dict(resize_shape=(32, 128, 3), text="ab"), dict(resize_shape=(32, 100, 3), text="tps")]
    losses = m.forward_train(img, metas)
    loss = sum(v.mean() for v in losses.values())          # TFLoss: reduction "none"
    loss.backward()
    convs = [(k, p) for k, p in m.tpsnet.named_parameters() if k.endswith("conv.weight") and p.dim() == 4
             and "atten" not in k]
    assert len(convs) >= 9
    for k, p in convs:
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert any(p.grad.abs().max() > 0 for _, p in convs)
