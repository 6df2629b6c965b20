"""-m gpu: the stage kernels of the TPS++ control-point regressor and of the classic localisation network, called directly
through their wrappers (ops.front, ops.down_fused_f32, ops.cbam, ops.tpe_points, ops.score, ops.dgab / ops.dgab_bf16,
ops.maxpool2x2, ops.global_avgpool, ops.linear) at the smallest shapes that reach every tile tail, trip count and idle
wavefront of their launchers (tests/test_stage_primitives_host.py recomputes the launchers' selection from the case tables
and asserts that every branch occurs).

Two kinds of comparison, the project's own (tests/test_gpu_train_primitives.py):

A. EXACT.  front and tpe_points are Linear / 1x1 convolution and ReLU only.  With small non-zero integer inputs, weights and
   biases every product and every partial sum, in any order, is an integer below 2^24 (the host file computes the bounds
   from the limits below and checks the operands actually used), so the fp32 MFMA and FMA chains must equal an integer
   NumPy reference bit for bit: a wrong index names its image, feature and pixel.  maxpool2x2 is a selection: bit equality
   with F.max_pool2d on the CPU for any floats -- negative maps, -inf, a NaN in each of the four window positions and in
   the row / column an odd map drops.

B. AGAINST FLOAT64 WITH THE PROJECT'S BAR: the relative L2 error against the module mirror's own PyTorch composition in
   float64 on the CPU (`copy.deepcopy(m).double()`; F.max_pool2d / mean / F.linear for the classic network's pieces) is
   <= max(1e-5, 2 x the error of PyTorch's fp32 composition of the same operation on the GPU against the same float64),
   per output tensor and again per image, so that one wrong image of a batch is not averaged away.  Every measured error
   is printed with its bar.  The three-term variants (score x3, dgab_bf16 x3) run at the same shapes under the absolute
   tolerances tests/test_gpu_dgab.py gives them (2e-5, 1e-4); their relative errors are printed.

Every weight and bias is drawn non-zero from a seeded generator (`stage_module`, `int_module`): a fresh TPS_PP has an
all-zero localization_fc2.weight, with which ctrl is its bias whatever the kernel does.  The scale is that of the project's
synthetic states (tps_pp_amd/synth.py: weights uniform in +-1 / sqrt(fan_in), biases in +-0.1, LayerNorm weights in 1 +-
0.25), and the inputs of the score and of DGAB are uniform in [-1, 1] like synth.dyadic: the absolute tolerances of the
three-term variants were set at that scale and mean nothing at another.  The rows of DGAB's mlp_w / mlp_h that feed the
two softmaxes are drawn with standard deviation 0.6, so that with y scaled by 30 logits pass 88.7, where expf overflows
unless the maximum is subtracted first; the last row (the two gate factors) with 0.02, so that the gated map stays of
order one.  In the saturated score case p is scaled until the largest |logit| is near 20: there the three-term variant is
held to what its number format can give, |error| <= 3 x 2^-16 x scale x sum_i |f_i| |p_i| per output (each operand of a
product keeps 16 bits, the lo x lo term is dropped, three chained products), which at that scale is above 2e-5; its
largest error is printed beside 2e-5.

The case tables and the reference builders are module-level and need no GPU: the host file imports them."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as GA
from test_gpu_train_primitives import assert_same_bits, rel, within_bar
from tps_pp_amd import TPS_PP, ops

pytestmark = pytest.mark.gpu

EXACT = 2 ** 24


# ---- the launchers' selection, restated (tps_pp_amd/csrc/tpspp_front.hip, _score.hip, _dgab.hip, _points.hip, _pool.hip) ----
def front_plan(H, W):
    """front_kernel: 256-pixel tiles, grid (gx, N), a workgroup walks tiles blockIdx.x, + gx, ..."""
    hw = H * W
    tiles = -(-hw // 256)
    gx = (tiles + 3) // 4 if tiles >= 8 else tiles
    trips = [len(range(b, tiles, gx)) for b in range(gx)]
    return dict(tiles=tiles, gx=gx, uneven=len(set(trips)) > 1, ragged=hw % 256 != 0, below_tile=hw < 256,
                odd_half_width=(W // 2) % 2 == 1, strided=gx < tiles)


def score_plan(n):
    """score_kernel / score_x3_kernel: one workgroup per image and 128 pixels."""
    return dict(blocks=-(-n // 128), ragged=n % 128 != 0, below_block=n < 128)


def dgab_plan(N, C, bf16=False):
    """The chain kernels: a wavefront takes a 32-row tile (two planes) per trip; 8 wavefronts and at most 256 workgroups
    (fp32 and the three-term split), 4 wavefronts and at most 512 (plain bf16)."""
    nwave, cap = (4, 512) if bf16 else (8, 256)
    wtiles = N * C // 2
    wgs = -(-wtiles // nwave)
    grid = min(wgs, cap)
    return dict(wtiles=wtiles, workgroups=wgs, cap=cap, idle_wavefronts=wtiles % nwave != 0,
                single_short_workgroup=wtiles < nwave, second_trip=wtiles > grid * nwave, gate_tail=(N * C) % 4 != 0)


def points_plan(N):
    """tpe_points_kernel: two images per workgroup and trip, at most 256 workgroups."""
    pairs = (N + 1) // 2
    return dict(pairs=pairs, second_trip=pairs > 256, odd_tail=N % 2 == 1)


def avgpool_plan(N, C, H, W):
    """global_avgpool_kernel: a wavefront per plane, four to a workgroup."""
    return dict(plane_tail=(N * C) % 4, hw=H * W, below_wave=H * W < 64, wave_tail=(H * W) % 64 != 0 and H * W > 64)


# ---- the modules: every weight and bias non-zero, from a seeded generator --------------------------------------------------
GATE_LOGIT_STD, GATE_LAST_STD = 0.6, 0.02


def uniform(shape, g):
    """Uniform in [-1, 1)."""
    return 2.0 * torch.rand(tuple(shape), generator=g) - 1.0


@functools.lru_cache(maxsize=None)
def stage_module():
    """TPS_PP (ResNet45v2 wiring) in float32 on the CPU with every parameter redrawn at the scale of synth.state_dict_like:
    weights uniform in +-1 / sqrt(fan_in), LayerNorm weights in 1 +- 0.25, biases in +-0.1; the gate layers of DGAB as the
    module docstring says."""
    m = TPS_PP().eval()
    g = torch.Generator().manual_seed(4100)
    with torch.no_grad():
        for name, p in m.named_parameters():
            r = uniform(p.shape, g)
            if ".norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.25 * r)
            elif name.endswith("bias"):
                p.copy_(0.1 * r)
            else:
                p.copy_(r / p[0].numel() ** 0.5)
        blk = m.TPE.atten[0]
        for lin in (blk.attn.mlp_w[0], blk.attn.mlp_h[0]):
            lin.weight[:-1] = GATE_LOGIT_STD * torch.randn(lin.weight[:-1].shape, generator=g)
            lin.weight[-1] = GATE_LAST_STD * torch.randn(lin.weight[-1].shape, generator=g)
    return m.requires_grad_(False)


@functools.lru_cache(maxsize=None)
def stage_module64():
    return copy.deepcopy(stage_module()).double()


@functools.lru_cache(maxsize=None)
def on_gpu(which, dev):
    """`stage_module` / `int_module` / a saturated-score module on the device, with the kernels' prepared weights."""
    m = copy.deepcopy({"stage": stage_module, "int": int_module, "saturated": saturated_module}[which]()).to(dev)
    k = dict(m=m, front=ops.FrontWeights(m), score=ops.ScoreWeights(m.TPE.feat_linear), dgab=ops.DgabWeights(m.TPE.atten[0]),
             dgab_bf16=ops.DgabWeightsBf16(m.TPE.atten[0]), dgab_x3=ops.DgabWeightsBf16(m.TPE.atten[0], x3=True),
             down0_1=ops.prep_conv_weight(m.down0_1.conv.weight, conv_bias=m.down0_1.conv.bias),
             down1_1=ops.prep_conv_weight(m.down1_1.conv.weight, conv_bias=m.down1_1.conv.bias))
    return k


# the limits of the exact cases: inputs, weights, biases (all integers, weights and biases non-zero)
FRONT_A_IN, FRONT_A_W, FRONT_A_B = 4, 2, 4
POINTS_A_IN, POINTS_A_W, POINTS_A_B = 2, 1, 1
FRONT_LAYERS = ("down0", "down1", "down2", "down_feat")
POINT_LAYERS = ("localization_fc1.0", "localization_fc1.2", "localization_fc2", "p_linear.0", "p_linear.1")


def nonzero_ints(rng, shape, lim):
    """Integers in [-lim, lim] without 0, as float32."""
    v = rng.integers(1, lim + 1, size=shape) * rng.choice(np.array([-1, 1]), size=shape)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def int_module():
    """TPS_PP whose pointwise front and point stages hold non-zero integers within the limits above."""
    m = copy.deepcopy(stage_module())
    rng = np.random.default_rng(4200)
    with torch.no_grad():
        for name in FRONT_LAYERS:
            conv = getattr(m, name).conv
            conv.weight.copy_(torch.from_numpy(nonzero_ints(rng, tuple(conv.weight.shape), FRONT_A_W)))
            conv.bias.copy_(torch.from_numpy(nonzero_ints(rng, tuple(conv.bias.shape), FRONT_A_B)))
        for name in POINT_LAYERS:
            lin = m.TPE.get_submodule(name)
            lin.weight.copy_(torch.from_numpy(nonzero_ints(rng, tuple(lin.weight.shape), POINTS_A_W)))
            lin.bias.copy_(torch.from_numpy(nonzero_ints(rng, tuple(lin.bias.shape), POINTS_A_B)))
    return m


def front_a_bounds():
    """(largest |value| of feat0 / feat1 / feat2, of feat_grid) the limits allow: a 1x1 layer of at most 64 inputs, then the
    192-deep one on top of it."""
    layer1 = max(32, 64) * FRONT_A_IN * FRONT_A_W + FRONT_A_B
    return layer1, 192 * FRONT_A_W * layer1 + FRONT_A_B


def points_a_bounds():
    """(hidden unit of fc1, its two outputs per point, ctrl; first and second layer of p_linear)."""
    hid = 64 * POINTS_A_IN * POINTS_A_W + POINTS_A_B
    v = 256 * POINTS_A_W * hid + POINTS_A_B
    return dict(hidden=hid, v=v, ctrl=64 * POINTS_A_W * v + POINTS_A_B, t1=hid, p=32 * POINTS_A_W * hid + POINTS_A_B)


def relu64(a):
    return np.maximum(a, 0)


def spread(label, t, relu=False):
    """A reference that is constant, or the output of a dead ReLU layer, proves nothing: refuse it."""
    t = t.detach().double().reshape(-1) if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t, np.float64)).reshape(-1)
    assert torch.isfinite(t).all(), f"{label}: the reference is not finite"
    if t.numel() == 1:
        assert float(t.abs()) > 0, f"{label}: the single reference value is 0"
        return
    assert float(t.std()) > 1e-2, f"{label}: the reference has no spread (std {float(t.std()):.3e})"
    if relu:
        live = float((t > 0).double().mean())
        assert 0.05 < live < 0.98, f"{label}: {live:.1%} of the ReLU outputs are positive"


def held(label, got, lib32, want, bad):
    """within_bar for the tensor and, in a batch, for every image on its own."""
    within_bar(label, got, lib32, want, bad)
    if want.shape[0] > 1:
        for b in range(want.shape[0]):
            within_bar(f"{label}, image {b}", got[b], lib32[b], want[b], bad)


def report_abs(label, got, want, tol, bad):
    """The three-term variants: an absolute tolerance; the relative L2 error is printed beside it."""
    assert torch.isfinite(got).all(), f"{label}: not finite"
    err = float((got.detach().cpu().double() - want).abs().max())
    print(f"{label}: max abs {err:.3e}, tolerance {tol:.1e}; rel L2 {rel(got, want):.3e}")
    if not err <= tol:
        bad[label] = (err, tol)


# ---- front -----------------------------------------------------------------------------------------------------------------
FRONT_CASES = ((1, 2, 2), (2, 2, 10), (3, 6, 46), (2, 18, 128), (1, 20, 128), (2, 32, 128))
FRONT_A_CASES = ((2, 2, 10), (3, 6, 46), (1, 20, 128))
FRONT_NAMES = ("feat0", "feat1", "feat2", "feat_grid")


def front_compose(m, o0, o1, x):
    """The four maps of `ops.front` as the module composes them (tps_pp.py: down0 / down1 / down2, grid())."""
    f0, f1, f2 = m.down0(o0), m.down1(o1), m.down2(x)
    return f0, f1, f2, m.grid(f0, f1, f2)


@functools.lru_cache(maxsize=None)
def front_case(N, H, W):
    g = torch.Generator().manual_seed(5000 + 1000 * N + 7 * H + W)
    o0, o1 = (torch.randn((N, 32, H, W), generator=g) for _ in range(2))
    x = torch.randn((N, 64, H // 2, W // 2), generator=g)
    want = front_compose(stage_module64(), o0.double(), o1.double(), x.double())
    return dict(o0=o0, o1=o1, x=x, want=want)


@functools.lru_cache(maxsize=None)
def front_a_case(N, H, W):
    rng = np.random.default_rng(5500 + 1000 * N + 7 * H + W)
    o0, o1 = (rng.integers(-FRONT_A_IN, FRONT_A_IN + 1, size=(N, 32, H, W)) for _ in range(2))
    x = rng.integers(-FRONT_A_IN, FRONT_A_IN + 1, size=(N, 64, H // 2, W // 2))
    m = int_module()
    w = {n: (getattr(m, n).conv.weight.numpy().reshape(64, -1).astype(np.int64), getattr(m, n).conv.bias.numpy().astype(np.int64))
         for n in FRONT_LAYERS}

    def pw(name, t):
        return relu64(np.einsum("oc,nchw->nohw", w[name][0], t) + w[name][1][None, :, None, None])
    f0, f1, f2 = pw("down0", o0), pw("down1", o1), pw("down2", x)
    fg = pw("down_feat", np.concatenate([f0, f1, f2.repeat(2, axis=2).repeat(2, axis=3)], axis=1))
    return dict(o0=o0.astype(np.float32), o1=o1.astype(np.float32), x=x.astype(np.float32), want=(f0, f1, f2, fg))


# ---- down_fused_f32 --------------------------------------------------------------------------------------------------------
DOWN_FUSED_CASES = ((3, 2), (2, 6), (1, 32))          # (N, H) at W = 128


@functools.lru_cache(maxsize=None)
def down_fused_case(N, H):
    g = torch.Generator().manual_seed(6000 + 100 * N + H)
    o = torch.randn((N, 32, H, 128), generator=g)
    m = stage_module64()
    return dict(o=o, want=(m.down0_1(m.down0(o.double())), m.down1_1(m.down1(o.double()))))


# ---- cbam ------------------------------------------------------------------------------------------------------------------
CBAM_BATCHES = (1, 2, 5)
CBAM_KINDS = ("signed", "one-image-negative", "one-positive-pixel")


@functools.lru_cache(maxsize=None)
def cbam_case(N, kind):
    """(N, 64, 2, 16); the last image of the batch is the special one: all negative, or negative but for one pixel per
    channel at +4 |N(0, 1)| + 1 (the channel max far from the channel mean)."""
    g = torch.Generator().manual_seed(6500 + 10 * N + CBAM_KINDS.index(kind))
    x = torch.randn((N, 64, 2, 16), generator=g)
    if kind != "signed":
        x[N - 1] = -x[N - 1].abs() - 0.01
    if kind == "one-positive-pixel":
        at = torch.randint(0, 32, (64,), generator=g)
        x[N - 1].view(64, 32)[torch.arange(64), at] = 4.0 * torch.randn(64, generator=g).abs() + 1.0
    return dict(x=x, want=stage_module64().MSFA.conv.atten(x.double()))


# ---- tpe_points ------------------------------------------------------------------------------------------------------------
POINTS_A_BATCHES = (1, 2, 3, 513, 515)
POINTS_B_BATCHES = (1, 3, 5)


def points_compose(tpe, en_map):
    """(ctrl, p) of `ops.tpe_points` as Transformation_Parameter_Estimation composes them."""
    n = en_map.shape[0]
    en = en_map.flatten(2).transpose(1, 2)
    return tpe.localization_fc2(tpe.localization_fc1(en).reshape(n, -1)).view(n, 32, 2), tpe.p_linear(en)


@functools.lru_cache(maxsize=None)
def points_case(N):
    g = torch.Generator().manual_seed(7000 + N)
    en = torch.randn((N, 64, 2, 16), generator=g)
    return dict(en=en, want=points_compose(stage_module64().TPE, en.double()))


@functools.lru_cache(maxsize=None)
def points_a_case(N):
    rng = np.random.default_rng(7500 + N)
    en = rng.integers(-POINTS_A_IN, POINTS_A_IN + 1, size=(N, 64, 2, 16))
    T = int_module().TPE
    w = {n: (T.get_submodule(n).weight.numpy().astype(np.int64), T.get_submodule(n).bias.numpy().astype(np.int64))
         for n in POINT_LAYERS}

    def lin(name, t):
        return t @ w[name][0].T + w[name][1]
    pts = en.reshape(N, 64, 32).transpose(0, 2, 1)                                   # (N, 32 points, 64 channels)
    hid = relu64(lin("localization_fc1.0", pts))
    v = relu64(lin("localization_fc1.2", hid))
    ctrl = lin("localization_fc2", v.reshape(N, 64)).reshape(N, 32, 2)
    t1 = lin("p_linear.0", pts)
    return dict(en=en.astype(np.float32), want=(ctrl, lin("p_linear.1", t1)), hidden=hid, v=v, t1=t1)


# ---- score -----------------------------------------------------------------------------------------------------------------
SCORE_N = 2
SCORE_SHAPES = ((1, 1), (1, 127), (1, 128), (3, 43), (5, 50), (16, 64))
SCORE_X3_TOL = 2e-5
SATURATED_SHAPE = (3, 43)
SATURATED_TARGET = 20.0
X3_SPLIT_BOUND = 3 * 2.0 ** -16        # three chained products, each with 16-bit operands and no lo x lo term


@functools.lru_cache(maxsize=None)
def score_case(H, W):
    g = torch.Generator().manual_seed(8000 + 100 * H + W)
    de = uniform((SCORE_N, 64, H, W), g)
    en = uniform((SCORE_N, 32, 64), g)
    return dict(de=de, en=en, want=stage_module64().TPE.get_score(en.double(), de.double()))


def score_logits(tpe, en, de):
    """What get_score hands to tanh: (N, H W, 32)."""
    f = tpe.feat_linear(de.flatten(2).transpose(1, 2))
    return torch.einsum("bnc,bmc->bmn", tpe.p_linear(en), f) * tpe.scale


@functools.lru_cache(maxsize=None)
def saturated_module():
    """`stage_module` with the second layer of p_linear scaled by a power of two (p itself is then scaled by it, exactly)
    such that the largest |logit| of `score_case(*SATURATED_SHAPE)` is within a factor sqrt(2) of 20."""
    k = score_case(*SATURATED_SHAPE)
    top = float(score_logits(stage_module64().TPE, k["en"].double(), k["de"].double()).abs().max())
    factor = 2.0 ** round(np.log2(SATURATED_TARGET / top))
    m = copy.deepcopy(stage_module())
    with torch.no_grad():
        m.TPE.p_linear[1].weight.mul_(factor)
        m.TPE.p_linear[1].bias.mul_(factor)
    return m


@functools.lru_cache(maxsize=None)
def saturated_case():
    k = score_case(*SATURATED_SHAPE)
    tpe = copy.deepcopy(saturated_module()).double().TPE
    de, en = k["de"].double(), k["en"].double()
    f, p = tpe.feat_linear(de.flatten(2).transpose(1, 2)), tpe.p_linear(en)
    return dict(de=k["de"], en=k["en"], want=tpe.get_score(en, de), top=float(score_logits(tpe, en, de).abs().max()),
                x3_bound=X3_SPLIT_BOUND * tpe.scale * torch.einsum("bnc,bmc->bmn", p.abs(), f.abs()))


# ---- dgab ------------------------------------------------------------------------------------------------------------------
DGAB_CASES = ((1, 8), (3, 24), (2, 64))
DGAB_KINDS = ("random", "constant-plane", "y-times-30")
DGAB_X3_TOL = 1e-4
DGAB_LIB32_LIMIT = 1e-4
DGAB_TRIP = (67, 64)
DGAB_TRIP_SLICES = ((0, 1), (31, 34), (63, 66), (66, 67))      # (63, 66): image 64 holds the first tile of the second trip


@functools.lru_cache(maxsize=None)
def dgab_case(N, C, kind):
    """x (N, C, 16, 64) and y (N, C, 32) as the kernels take them (the module takes y^T); constant-plane: plane (0, 1) of x
    is 3.0 everywhere (variance 0 in LayerNorm 1); y-times-30: large logits in both softmaxes."""
    g = torch.Generator().manual_seed(9000 + 100 * N + C)
    x = uniform((N, C, 16, 64), g)
    y = uniform((N, C, 32), g)
    if kind == "constant-plane":
        x[0, 1] = 3.0
    if kind == "y-times-30":
        y = 30.0 * y
    return dict(x=x, y=y, want=stage_module64().TPE.atten[0](x.double(), y.double().transpose(1, 2)))


# ---- the classic network's pieces -------------------------------------------------------------------------------------------
MAXPOOL_SHAPES = ((1, 1, 2, 2), (2, 3, 5, 7), (1, 5, 3, 2), (3, 64, 32, 100))
MAXPOOL_VARIANTS = ("negative-and-inf", "nan-at-0", "nan-at-1", "nan-at-2", "nan-at-3")
AVGPOOL_SHAPES = ((1, 1, 1, 1), (1, 3, 1, 63), (2, 5, 5, 13), (3, 512, 1, 6))
LINEAR_BATCHES = (1, 3, 77)
LINEAR_LAYERS = ((512, 256, True), (256, 40, False))


def maxpool_case(shape, variant):
    """Random normal values shifted to be negative in the first plane, a -inf in the first window, an all -inf window where
    there is a second one; `nan-at-k`: a NaN at position k (row-major in the 2x2 window) of the LAST window of every plane,
    and in the last row and the last column where the map is odd and drops them."""
    N, C, H, W = shape
    rng = np.random.default_rng(9500 + 1000 * H + 10 * W + MAXPOOL_VARIANTS.index(variant))
    x = rng.standard_normal(shape).astype(np.float32)
    x[0, 0] = -np.abs(x[0, 0]) - np.float32(0.5)
    x[0, 0, 0, 1] = -np.inf
    if W >= 4:
        x[0, 0, 0:2, 2:4] = -np.inf
    if variant != "negative-and-inf":
        k = MAXPOOL_VARIANTS.index(variant) - 1
        oy, ox = H // 2 - 1, W // 2 - 1
        x[:, :, 2 * oy + k // 2, 2 * ox + k % 2] = np.nan
        if H % 2:
            x[:, :, H - 1, :] = np.nan
        if W % 2:
            x[:, :, :, W - 1] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def avgpool_case(shape):
    g = torch.Generator().manual_seed(9700 + sum(shape))
    x = torch.randn(shape, generator=g) + torch.randn(shape[:2] + (1, 1), generator=g)        # a mean of its own per plane
    return dict(x=x, want=x.double().mean((2, 3)))


@functools.lru_cache(maxsize=None)
def linear_case(N, cin, cout, relu):
    g = torch.Generator().manual_seed(9800 + N + cin)
    x = torch.randn((N, cin), generator=g)
    w = torch.randn((cout, cin), generator=g) / cin ** 0.5
    b = 0.2 * torch.randn(cout, generator=g)
    z = F.linear(x.double(), w.double(), b.double())
    return dict(x=x, w=w, b=b, want=F.relu(z) if relu else z)


# =============================================================================================================================
# front, down_fused_f32
# =============================================================================================================================
@pytest.mark.parametrize("store01", [True, False], ids=["store01", "no-store01"])
@pytest.mark.parametrize("N,H,W", FRONT_A_CASES)
def test_front_is_exact_on_integers(cuda, N, H, W, store01):
    k = front_a_case(N, H, W)
    o0, o1, x = (torch.from_numpy(k[n]).to(cuda) for n in ("o0", "o1", "x"))
    got = ops.front(o0, o1, x, on_gpu("int", str(cuda))["front"], store01=store01)
    assert (got[0] is None) == (not store01) and (got[1] is None) == (not store01)
    for name, g, want in zip(FRONT_NAMES, got, k["want"]):
        spread(f"front integers {name}", want, relu=True)
        if g is not None:
            assert_same_bits(f"front ({N}, {H}, {W}) {name}, {front_plan(H, W)}", g.cpu().numpy(), want.astype(np.float32),
                             names=("image", "feature", "y", "x"))


@pytest.mark.parametrize("N,H,W", FRONT_CASES)
def test_front_against_float64(cuda, N, H, W):
    k = front_case(N, H, W)
    gm = on_gpu("stage", str(cuda))
    o0, o1, x = (k[n].to(cuda) for n in ("o0", "o1", "x"))
    lib32 = front_compose(gm["m"], o0, o1, x)
    bad = {}
    for store01 in (True, False):
        got = ops.front(o0, o1, x, gm["front"], store01=store01)
        assert (got[0] is None) == (not store01) and (got[1] is None) == (not store01)
        for name, g, l32, want in zip(FRONT_NAMES, got, lib32, k["want"]):
            spread(f"front {name}", want, relu=True)
            if g is not None:
                assert g.shape == want.shape
                held(f"front ({N}, {H}, {W}) store01 {store01} {name}", g, l32, want, bad)
    assert not bad, bad


@pytest.mark.parametrize("N,H", DOWN_FUSED_CASES)
def test_down_fused_f32_against_float64(cuda, N, H):
    k = down_fused_case(N, H)
    gm = on_gpu("stage", str(cuda))
    m, fw = gm["m"], gm["front"]
    o = k["o"].to(cuda)
    bad = {}
    for i, (w_slab, b, cw, lib32) in enumerate(((fw.w0, fw.b0, gm["down0_1"], m.down0_1(m.down0(o))),
                                                 (fw.w1, fw.b1, gm["down1_1"], m.down1_1(m.down1(o))))):
        spread(f"down_fused_f32 layer pair {i}", k["want"][i], relu=True)
        got = ops.down_fused_f32(o, w_slab, b, cw)
        assert got.shape == k["want"][i].shape
        held(f"down_fused_f32 ({N}, 32, {H}, 128) down{i} + down{i}_1", got, lib32, k["want"][i], bad)
    assert not bad, bad


# =============================================================================================================================
# cbam, tpe_points
# =============================================================================================================================
@pytest.mark.parametrize("kind", CBAM_KINDS)
@pytest.mark.parametrize("N", CBAM_BATCHES)
def test_cbam_against_float64(cuda, N, kind):
    k = cbam_case(N, kind)
    atten = on_gpu("stage", str(cuda))["m"].MSFA.conv.atten
    x = k["x"].to(cuda)
    spread(f"cbam {kind}", k["want"])
    bad = {}
    held(f"cbam N {N} {kind}", ops.cbam(x, atten), atten(x), k["want"], bad)
    assert not bad, bad


@pytest.mark.parametrize("N", POINTS_A_BATCHES)
def test_tpe_points_is_exact_on_integers(cuda, N):
    k = points_a_case(N)
    ctrl, p = ops.tpe_points(torch.from_numpy(k["en"]).to(cuda), on_gpu("int", str(cuda))["m"].TPE)
    spread("tpe_points integers ctrl", k["want"][0])
    spread("tpe_points integers p", k["want"][1])
    assert_same_bits(f"tpe_points N {N} ctrl, {points_plan(N)}", ctrl.cpu().numpy(), k["want"][0].astype(np.float32),
                     names=("image", "point", "xy"))
    assert_same_bits(f"tpe_points N {N} p, {points_plan(N)}", p.cpu().numpy(), k["want"][1].astype(np.float32),
                     names=("image", "point", "feature"))


@pytest.mark.parametrize("N", POINTS_B_BATCHES)
def test_tpe_points_against_float64(cuda, N):
    k = points_case(N)
    tpe = on_gpu("stage", str(cuda))["m"].TPE
    en = k["en"].to(cuda)
    got, lib32 = ops.tpe_points(en, tpe), points_compose(tpe, en)
    bad = {}
    for name, g, l32, want in zip(("ctrl", "p"), got, lib32, k["want"]):
        spread(f"tpe_points {name}", want)
        assert g.shape == want.shape
        held(f"tpe_points N {N} {name}", g, l32, want, bad)
    assert not bad, bad


# =============================================================================================================================
# score
# =============================================================================================================================
def _score_run(gm, k, x3, dev):
    de, en = k["de"].to(dev), k["en"].to(dev)
    tpe = gm["m"].TPE
    got = ops.score(de, tpe.p_linear(en).contiguous(), gm["score"], tpe.scale, x3=x3)
    return got, tpe.get_score(en, de)


@pytest.mark.parametrize("x3", [False, True], ids=["fp32", "x3"])
@pytest.mark.parametrize("H,W", SCORE_SHAPES)
def test_score_against_float64(cuda, H, W, x3):
    k = score_case(H, W)
    got, lib32 = _score_run(on_gpu("stage", str(cuda)), k, x3, cuda)
    assert got.shape == k["want"].shape == (SCORE_N, H * W, 32)
    spread("score", k["want"])
    bad = {}
    label = f"score n {H * W} ({H} x {W}) {'x3' if x3 else 'fp32'}, {score_plan(H * W)}"
    if x3:
        report_abs(label, got, k["want"], SCORE_X3_TOL, bad)
        print(f"{label}: PyTorch fp32 rel L2 {rel(lib32, k['want']):.3e}")
    else:
        held(label, got, lib32, k["want"], bad)
    assert not bad, bad


@pytest.mark.parametrize("x3", [False, True], ids=["fp32", "x3"])
def test_score_saturated(cuda, x3):
    """Logits near +-20: tanh is +-1 to the last bit for most of the map, never beyond."""
    k = saturated_case()
    got, lib32 = _score_run(on_gpu("saturated", str(cuda)), k, x3, cuda)
    assert SATURATED_TARGET / 2 ** 0.5 <= k["top"] <= SATURATED_TARGET * 2 ** 0.5
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    bad = {}
    label = f"score saturated (largest |logit| {k['top']:.1f}) {'x3' if x3 else 'fp32'}"
    if x3:
        err = (got.cpu().double() - k["want"]).abs()
        worst = float((err / k["x3_bound"]).max())
        print(f"{label}: max abs {float(err.max()):.3e} (beside {SCORE_X3_TOL:.1e} at the workload's scale), largest error / "
              f"format bound {worst:.3e}; rel L2 {rel(got, k['want']):.3e}")
        assert torch.isfinite(got).all() and worst <= 1.0
    else:
        held(label, got, lib32, k["want"], bad)
    assert not bad, bad


# =============================================================================================================================
# dgab
# =============================================================================================================================
@pytest.mark.parametrize("kind", DGAB_KINDS)
@pytest.mark.parametrize("N,C", DGAB_CASES)
def test_dgab_against_float64(cuda, N, C, kind):
    k = dgab_case(N, C, kind)
    gm = on_gpu("stage", str(cuda))
    x, y = k["x"].to(cuda), k["y"].to(cuda)
    want = k["want"]
    spread(f"dgab {kind}", want)
    lib32 = gm["m"].TPE.atten[0](x, y.transpose(1, 2))
    e_lib = rel(lib32, want)
    assert e_lib <= DGAB_LIB32_LIMIT, f"PyTorch's fp32 composition is {e_lib:.3e} from float64"
    bad = {}
    held(f"dgab ({N}, {C}) {kind} fp32, {dgab_plan(N, C)}", ops.dgab(x, y, gm["dgab"]), lib32, want, bad)
    report_abs(f"dgab ({N}, {C}) {kind} x3", ops.dgab_bf16(x, y, gm["dgab_x3"]), want, DGAB_X3_TOL, bad)
    assert not bad, bad


def test_dgab_second_trip_gives_what_slices_give(cuda):
    """(67, 64): 2144 wavefront tiles, 268 workgroups of 8 against 256 (fp32, x3), 536 of 4 against 512 (bf16): the first
    twelve (twenty-four) workgroups' wavefronts take a second tile, the first of them tile 2048 = image 64, channels 0 and
    1.  The whole batch equals its slices bit for bit; the slice (63, 66) holds the images on both sides of that wrap (a
    trip stride that is off by one tile skips tile 2048 and nothing else)."""
    N, C = DGAB_TRIP
    assert dgab_plan(N, C)["second_trip"] and dgab_plan(N, C, bf16=True)["second_trip"]
    gm = on_gpu("stage", str(cuda))
    g = torch.Generator(device=cuda).manual_seed(67)
    x = torch.randn((N, C, 16, 64), generator=g, device=cuda)
    y = torch.randn((N, C, 32), generator=g, device=cuda)
    for name, w, fn in (("fp32", gm["dgab"], ops.dgab), ("bf16", gm["dgab_bf16"], ops.dgab_bf16),
                        ("x3", gm["dgab_x3"], ops.dgab_bf16)):
        whole = fn(x, y, w)
        assert torch.isfinite(whole).all() and float(whole.std()) > 0.1, name
        for lo, hi in DGAB_TRIP_SLICES:
            part = fn(x[lo:hi].contiguous(), y[lo:hi].contiguous(), w)
            assert torch.equal(whole[lo:hi], part), f"dgab {name}: images [{lo}:{hi}) of {N} differ from the slice run alone"


# =============================================================================================================================
# maxpool2x2, global_avgpool, linear
# =============================================================================================================================
@pytest.mark.parametrize("shape", MAXPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool2x2_is_max_pool2d_bit_for_bit(cuda, shape):
    for variant in MAXPOOL_VARIANTS:
        x = torch.from_numpy(maxpool_case(shape, variant))
        want = F.max_pool2d(x, 2, 2)
        got = ops.maxpool2x2(x.to(cuda)).cpu()
        assert bool(torch.isnan(want).any()) == (variant != "negative-and-inf")
        assert_same_bits(f"maxpool2x2 {shape} {variant}", got.numpy(), want.numpy(), names=("image", "channel", "y", "x"))


@pytest.mark.parametrize("shape", AVGPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_global_avgpool_against_float64(cuda, shape):
    k = avgpool_case(shape)
    x = k["x"].to(cuda)
    spread("global_avgpool", k["want"])
    bad = {}
    held(f"global_avgpool {shape}, {avgpool_plan(*shape)}", ops.global_avgpool(x), x.mean((2, 3)), k["want"], bad)
    assert not bad, bad


@pytest.mark.parametrize("cin,cout,relu", LINEAR_LAYERS)
@pytest.mark.parametrize("N", LINEAR_BATCHES)
def test_linear_against_float64(cuda, N, cin, cout, relu):
    k = linear_case(N, cin, cout, relu)
    x, w, b = (k[n].to(cuda) for n in ("x", "w", "b"))
    cw = ops.prep_conv_weight(w.view(cout, cin, 1, 1), conv_bias=b)
    got = ops.linear(x, cw, relu=relu)
    lib32 = F.linear(x, w, b)
    spread("linear", k["want"], relu=relu)
    assert got.shape == (N, cout)
    bad = {}
    held(f"linear N {N} {cin} -> {cout} relu {relu}", got, F.relu(lib32) if relu else lib32, k["want"], bad)
    assert not bad, bad


# =============================================================================================================================
# refusals
# =============================================================================================================================
def test_wrappers_refuse_other_geometries(cuda):
    gm = on_gpu("stage", str(cuda))
    z = lambda *s: torch.zeros(s, device=cuda)         # noqa: E731
    for fn, w in ((ops.dgab, gm["dgab"]), (ops.dgab_bf16, gm["dgab_bf16"])):
        with pytest.raises(ValueError, match=r"needs x \(N, C, 16, 64\)"):
            fn(z(1, 8, 16, 32), z(1, 8, 32), w)
        with pytest.raises(ValueError, match=r"needs x \(N, C, 16, 64\)"):
            fn(z(1, 8, 16, 64), z(1, 8, 31), w)
        with pytest.raises(ValueError, match=r"needs x \(N, C, 16, 64\)"):
            fn(z(2, 8, 16, 64), z(1, 8, 32), w)
    with pytest.raises(ValueError, match="cbam: needs"):
        ops.cbam(z(2, 64, 2, 8), gm["m"].MSFA.conv.atten)
    with pytest.raises(ValueError, match="tpe_points: needs"):
        ops.tpe_points(z(2, 64, 2, 8), gm["m"].TPE)
    with pytest.raises(ValueError, match="score: needs"):
        ops.score(z(1, 32, 4, 4), z(1, 32, 128), gm["score"], 0.125)
    with pytest.raises(ValueError, match="front: needs"):
        ops.front(z(1, 32, 4, 4), z(1, 32, 4, 4), z(1, 64, 2, 4), gm["front"])
    with pytest.raises(ValueError, match="front: needs"):
        ops.front(z(1, 32, 4, 4), z(1, 32, 4, 4), z(2, 64, 2, 2), gm["front"])


# =============================================================================================================================
# guard bands: one ragged case per kernel; dead lanes read through clamped indices
# =============================================================================================================================
def _guarded_like_plain(cuda, label, run, inputs):
    """`run` on plain device copies of `inputs`, then on guarded copies with guarded outputs: guards and NaN bands intact,
    nothing left unwritten, and the same bits."""
    plain = run(*[t.to(cuda) for t in inputs])
    with GA.guarded(cuda) as g:
        out = run(*[g.input(t) for t in inputs])
        assert g.check(out, require_guarded=True) >= 1 and not g.fallthrough, g.fallthrough
    ok, why = GA.same_bits(plain, out)
    assert ok, f"{label}: {why}"
    return out


@pytest.mark.parametrize("store01", [True, False], ids=["store01", "no-store01"])
def test_guarded_front(cuda, store01):
    k = front_case(3, 6, 46)
    fw = on_gpu("stage", str(cuda))["front"]
    _guarded_like_plain(cuda, "front (3, 6, 46)", lambda o0, o1, x: ops.front(o0, o1, x, fw, store01=store01),
                        [k["o0"], k["o1"], k["x"]])


@pytest.mark.parametrize("x3", [False, True], ids=["fp32", "x3"])
def test_guarded_score(cuda, x3):
    k = score_case(3, 43)
    gm = on_gpu("stage", str(cuda))
    p = gm["m"].TPE.p_linear(k["en"].to(cuda)).contiguous().cpu()
    _guarded_like_plain(cuda, "score n 129", lambda de, pp: ops.score(de, pp, gm["score"], gm["m"].TPE.scale, x3=x3),
                        [k["de"], p])


@pytest.mark.parametrize("which", ["fp32", "bf16", "x3"])
def test_guarded_dgab(cuda, which):
    k = dgab_case(1, 8, "random")
    gm = on_gpu("stage", str(cuda))
    w, fn = {"fp32": (gm["dgab"], ops.dgab), "bf16": (gm["dgab_bf16"], ops.dgab_bf16), "x3": (gm["dgab_x3"], ops.dgab_bf16)}[which]
    _guarded_like_plain(cuda, f"dgab (1, 8) {which}", lambda x, y: fn(x, y, w), [k["x"], k["y"]])


def test_guarded_tpe_points(cuda):
    tpe = on_gpu("stage", str(cuda))["m"].TPE
    _guarded_like_plain(cuda, "tpe_points N 3", lambda en: ops.tpe_points(en, tpe), [points_case(3)["en"]])


def test_guarded_pools(cuda):
    _guarded_like_plain(cuda, "global_avgpool (2, 5, 5, 13)", ops.global_avgpool, [avgpool_case((2, 5, 5, 13))["x"]])
    x = torch.from_numpy(maxpool_case((2, 3, 5, 7), "nan-at-3"))
    out = _guarded_like_plain(cuda, "maxpool2x2 (2, 3, 5, 7)", ops.maxpool2x2, [x])
    assert_same_bits("guarded maxpool2x2 (2, 3, 5, 7)", out.cpu().numpy(), F.max_pool2d(x, 2, 2).numpy(),
                     names=("image", "channel", "y", "x"))
