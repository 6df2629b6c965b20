"""-m gpu: VeryDeepVgg in its reduced-precision modes (compute_dtype "bf16x3" / torch.bfloat16): the max-pools on blocked maps
(include/tpspp_crnn_bf16.h), the seven convolutions at the VGG's own shapes on `tpspp_conv2d_bf16_fwd`, and the module.

Every kernel output is allocated through tests/guarded_alloc.py: nothing is written outside it and every element of it is
written.  The convolutions' bars are those of tests/test_gpu_conv_bf16.py, restated: operands rounded to bf16 on both sides,
fp32 output: 1e-5 of the tensor's scale (fp32 summation order); bf16 output: within one bf16 ulp of the float64 value and more
than 98 % exactly rounded; bf16x3 against float64 on the unrounded operands: 2e-5 of the scale.  The module's bar in bf16x3 is
the project's 1e-4 against the golden (tests/test_crnn_bf16_host.py shows the arithmetic's own headroom under it); plain bf16
is held to 2 x the relative error its float64 restatement shows on the same batch (tests/crnn_bf16_cases.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crnn_bf16_cases as BC
import guarded_alloc as GA
from test_gpu_crnn import RECT, pool_inputs
from tps_pp_amd import _lib, ops, synth
from tps_pp_amd.crnn import VeryDeepVgg

pytestmark = pytest.mark.gpu

CC = BC.CC
SQUARE = ((2, 2), (2, 2), (0, 0))
MODES = ["bf16x3", torch.bfloat16]
MODE_IDS = ["bf16x3", "bf16"]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def blocked_of(x, x3, g=None):
    """NCHW -> the blocked map of the mode, values kept (bf16 mode: `x` holds bf16 values).  With a guard `g`: laid out on
    the host and copied between the guard's NaN bands."""
    cls = ops.Blocked32 if x3 else ops.Blocked
    return cls.from_nchw(x) if g is None else cls(g.input(cls.from_nchw(x.cpu()).t))


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {w.numel()} differ"


# ---- 1. the pools ----------------------------------------------------------------------------------------------------------
VGG_MAPS = [(64, 32, 100), (128, 16, 50), (256, 8, 25), (512, 4, 26)]
SMALL_MAPS = [(8, h, w) for h in (1, 2, 5) for w in (1, 2, 7)]


def pool_ok(shape, geo):
    (kh, kw), _, (ph, pw) = geo
    return shape[1] + 2 * ph >= kh and shape[2] + 2 * pw >= kw


POOL_CASES = [(m, g) for m in VGG_MAPS + SMALL_MAPS for g in (SQUARE, RECT) if pool_ok(m, g)]


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("chw,geo", POOL_CASES, ids=[f"{c}x{h}x{w}-{'rect' if g is RECT else 'square'}" for (c, h, w), g in POOL_CASES])
def test_blocked_maxpool_equals_torch_bit_for_bit(cuda, chw, geo, x3):
    """Both layouts, both of the VGG's geometries, the VGG's own maps at N = 2 and small ragged ones; the special values of
    test_gpu_crnn.py (negative maps, -inf, a NaN per window position and next to each padded column: the rectangular
    geometry's first and last output columns have one of their two window columns wholly in the padding)."""
    C, H, W = chw
    x = pool_inputs((2, C, H, W), geo)                 # (its variants are stacked along the batch)
    if not x3:
        x = x.to(torch.bfloat16)                       # NaN and inf stay; the negative values become bf16 values
        x.view(torch.int16)[torch.isnan(x)] = 0x7FC0   # (a vectorised cast may write NaN as 0xFFFF, the guards' poison word)
    want = F.max_pool2d(x.float(), *geo).to(x.dtype)   # (a max is one of its inputs: the bf16 round trip is exact)
    with GA.guarded(cuda) as g:
        src = blocked_of(x, x3, g)
        got = ops.crnn_maxpool_blocked(src, *geo)
        assert g.check(got.t, require_guarded=True) == 1
    assert type(got) is type(src) and got.shape == tuple(want.shape)
    assert torch.isnan(want).any() and torch.isinf(want).any()
    nan = torch.isnan(want)
    out = got.nchw().cpu()
    assert torch.equal(torch.isnan(out), nan)          # NaN by position
    same(torch.where(nan, torch.zeros_like(out), out), torch.where(nan, torch.zeros_like(want), want), f"pool {chw} {geo}")
    if x3:                                             # fp32: a NaN's bits pass through as well, as in tpspp_crnn_maxpool_fwd
        same(out, want, f"pool {chw} {geo}, NaN bits included")
    else:                                              # and F.max_pool2d on the bf16 NCHW view itself gives the same
        direct = F.max_pool2d(x, *geo)
        assert torch.equal(torch.isnan(direct), nan)
        same(torch.where(nan, torch.zeros_like(direct), direct), torch.where(nan, torch.zeros_like(want), want), "bf16 pool")


def test_blocked_maxpool_argument_checks(cuda):
    x = ops.Blocked.from_nchw(torch.zeros((1, 8, 4, 6), device=cuda))
    with pytest.raises(TypeError, match="Blocked"):
        ops.crnn_maxpool_blocked(x.nchw(), 2, 2, 0)
    with pytest.raises(ValueError, match="crnn_maxpool_blocked"):
        ops.crnn_maxpool_blocked(x, (5, 2), 2, 0)
    with pytest.raises(_lib.TpsppError, match="padding"):
        ops.crnn_maxpool_blocked(x, 2, 2, (0, 2))
    with pytest.raises(_lib.TpsppError, match="GPU tensor"):
        ops.crnn_maxpool_blocked(ops.Blocked(torch.zeros((1, 1, 4, 6, 8), dtype=torch.bfloat16)), 2, 2, 0)
    empty = ops.crnn_maxpool_blocked(ops.Blocked32(torch.zeros((0, 2, 4, 6, 8), device=cuda)), *RECT)
    assert isinstance(empty, ops.Blocked32) and empty.shape == (0, 16, 2, 7)


# ---- 3. each layer against float64 (the first launch of these shapes: before everything that runs the whole VGG) -----------
def layer_case(i, width):
    """Layer i's operands at image width `width`, N = 2: x fp32 NCHW in [-1, 1), w (Cout, Cin, 3, 3) at the fan-in scale, b."""
    cin, h, w_ = BC.layer_shapes(width)[i]
    cout = BC.CHANNELS[i]
    name = f"vgg.conv{i}.w{width}"
    x = torch.from_numpy(synth.dyadic((2, cin, h, w_), name + ".x", 1))
    w = torch.from_numpy(synth.dyadic((cout, cin, 3, 3), name + ".w", 1, 1.0 / np.sqrt(cin * 9)))
    b = torch.from_numpy(synth.dyadic((cout,), name + ".b", 1, 0.1))
    return x, w, b


def ref64(x, w, b, stride):
    return F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1)).float()


def vgg_call(i, x, cw, x3, blocked=True, g=None):
    """The call VeryDeepVgg makes for layer i (`blocked=False`: the NCHW route of the same arithmetic).  x: the image
    (layer 0) or the map, NCHW in the mode's dtype; with a guard `g`, x is on the host and the source is copied into it."""
    dt = torch.float32 if x3 else torch.bfloat16
    if i == 0 or not blocked:
        src = x if g is None else g.input(x)
    else:
        src = blocked_of(x, x3, g)
    if i == 6:
        return ops.conv2d_bf16([src], cw, (2, 1), True, out_dtype=torch.float32)
    return ops.conv2d_bf16([src], cw, 1, True, out_dtype=dt, out_blocked=blocked)


@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("i", range(7))
def test_each_layer_against_float64(cuda, i, width):
    x, w, b = layer_case(i, width)
    stride = (2, 1) if i == 6 else (1, 1)
    # plain bf16: operands rounded on both sides
    ref = ref64(BC.rb(x), BC.rb(w), b, stride)
    scale = float(ref.abs().max())
    with GA.guarded(cuda) as g:
        cw = ops.prep_conv_weight_bf16(w.to(cuda), conv_bias=b.to(cuda))
        got = vgg_call(i, x if i == 0 else x.to(torch.bfloat16), cw, False, g=g)        # conv0 reads the fp32 image
        g.check(got if i == 6 else got.t, require_guarded=True)
    if i == 6:
        err = float((got.cpu() - ref).abs().max())
        print(f"conv{i} width {width} bf16, fp32 output: max abs error {err:.3e}, bar {1e-5 * scale:.3e} (1e-5 of the scale)")
        assert got.dtype == torch.float32 and err <= 1e-5 * scale
    else:
        assert isinstance(got, ops.Blocked) and not isinstance(got, ops.Blocked32)
        out = got.nchw().float().cpu()
        e = (out - ref).abs()
        exact = float((out == BC.rb(ref)).float().mean())
        print(f"conv{i} width {width} bf16, bf16 output: max abs error {float(e.max()):.3e} (bar: one ulp, 2^-8 relative + "
              f"{1e-6 * scale:.1e}); exactly rounded {100 * exact:.2f} % (bar > 98 %)")
        assert bool((e <= ref.abs() * 2.0 ** -8 + 1e-6 * scale).all()) and exact > 0.98
    # the three-term split: against float64 on the unrounded operands
    ref = ref64(x, w, b, stride)
    scale = float(ref.abs().max())
    with GA.guarded(cuda) as g:
        cw = ops.prep_conv_weight_bf16(w.to(cuda), conv_bias=b.to(cuda), x3=True)
        got = vgg_call(i, x, cw, True, g=g)
        g.check(got if i == 6 else got.t, require_guarded=True)
    assert i == 6 or isinstance(got, ops.Blocked32)
    out = (got if i == 6 else got.nchw()).cpu()
    err = float((out - ref).abs().max())
    print(f"conv{i} width {width} bf16x3: max abs error {err:.3e}, bar {2e-5 * scale:.3e} (2e-5 of the scale)")
    assert out.dtype == torch.float32 and err <= 2e-5 * scale


# ---- 4. the wide-tile kernel equals the generic one --------------------------------------------------------------------------
@pytest.mark.parametrize("i", [2, 3])
def test_wide_tile_layers_equal_the_generic_kernel(cuda, i):
    """Image width 128: the 8 x 32 map sends conv2 (128 -> 256) and conv3 (256 -> 256) to tpspp_conv3_wide.hip in bf16 mode;
    tpspp_conv_set_tuning bit 2 switches that kernel off."""
    x, w, b = layer_case(i, 128)
    assert tuple(x.shape[2:]) == (8, 32)
    cw = ops.prep_conv_weight_bf16(w.to(cuda), conv_bias=b.to(cuda))
    with GA.guarded(cuda) as g:
        xin = blocked_of(x.to(torch.bfloat16), False, g)
        conv = lambda: ops.conv2d_bf16([xin], cw, 1, True, out_blocked=True)      # noqa: E731  (the VGG's call)
        try:
            _lib.lib().tpspp_conv_set_tuning(4)
            want = conv()
        finally:
            _lib.lib().tpspp_conv_set_tuning(0)
        got = conv()
        g.check([got.t, want.t], require_guarded=True)
    same(got.t, want.t, f"conv{i} wide against generic")


# ---- 2. blocked route == NCHW route ------------------------------------------------------------------------------------------
def nchw_route(vgg, x, x3):
    """The same seven `conv2d_bf16` calls with NCHW outputs, `ops.crnn_maxpool` on the fp32 view (re-rounded to bf16 in bf16
    mode: exact, a max is one of its inputs) -> the list of every layer's and every pool's NCHW result."""
    cw = vgg._hip_weights_bf16(x3)
    dt = torch.float32 if x3 else torch.bfloat16
    steps = []
    for i in range(7):
        x = vgg_call(i, x, cw[i], x3, blocked=False)
        steps.append(x)
        if i in BC.POOLS:
            x = ops.crnn_maxpool(x.float(), *BC.POOLS[i]).to(dt)
            steps.append(x)
    return steps


def blocked_route(vgg, x, x3):
    """`VeryDeepVgg._forward_hip_bf16`'s calls, one by one, keeping every result."""
    cw = vgg._hip_weights_bf16(x3)
    dt = torch.float32 if x3 else torch.bfloat16
    steps = []
    for i in range(6):
        x = ops.conv2d_bf16([x], cw[i], 1, True, out_dtype=dt, out_blocked=True)
        steps.append(x)
        if i in BC.POOLS:
            x = ops.crnn_maxpool_blocked(x, *BC.POOLS[i])
            steps.append(x)
    steps.append(ops.conv2d_bf16([x], cw[6], (2, 1), True, out_dtype=torch.float32))
    return steps


@pytest.fixture(scope="module")
def vggs(cuda):
    """{name: the golden model on the device}; the tests set the mode they need."""
    return {name: BC.build_model(name, cuda) for name in ("crnn_tps", "crnn")}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("width", [100, 128, 32])
def test_blocked_route_equals_nchw_route_bit_for_bit(cuda, vggs, mode, width):
    x3 = mode == "bf16x3"
    vgg = vggs["crnn_tps"].backbone
    img = torch.from_numpy(synth.smooth_image((2, 1, 32, width), f"crnn.route{width}", 1))
    with torch.no_grad(), GA.guarded(cuda) as g:
        xin = g.input(img)
        a = blocked_route(vgg, xin, x3)
        b = nchw_route(vgg, xin, x3)
        g.check([t.t if isinstance(t, ops.Blocked) else t for t in a], require_guarded=True)
        vgg.compute_dtype = mode
        try:
            whole = vgg(xin)
        finally:
            vgg.compute_dtype = None
    assert len(a) == len(b) == 11
    for k, (s, t) in enumerate(zip(a, b)):
        same(s.nchw() if isinstance(s, ops.Blocked) else s, t, f"step {k} width {width}")
    assert whole.dtype == torch.float32 and tuple(whole.shape) == (2, 512, 1, width // 4 + 1)
    same(whole, b[-1][:, :, :, :width // 4 + 1], "the module's forward")


# ---- 5. / 6. the module ------------------------------------------------------------------------------------------------------
def ragged(idx):
    return [r[r >= 0].tolist() for r in idx]


def run_model(m, cuda, name, G):
    """(features, logits, decoded indices) of the golden batch: the preprocessor (crnn_tps), the VGG, the decoder."""
    img = torch.from_numpy(CC.images() if name == "crnn_tps" else CC.images32())
    with torch.no_grad(), GA.guarded(cuda) as g:
        x = g.input(img)
        if name == "crnn_tps":
            x = m.preprocessor(x)
        feat = m.backbone(x)
        logits = m.decoder(feat, None, None, None, train_mode=False)
        g.check([feat._base if feat._base is not None else feat, logits], require_guarded=True)
    idx, _ = m.label_convertor.tensor2idx(logits, CC.img_metas(img.shape[0]))
    return feat.cpu(), logits.cpu(), idx


@pytest.mark.parametrize("name,fk,lk,ik", [("crnn_tps", "feat", "logits", "idx_full"), ("crnn", "feat32", "logits32", "idx32")])
def test_module_bf16x3_against_the_golden(cuda, vggs, name, fk, lk, ik):
    G = BC.golden()
    m = vggs[name]
    exact, _, _ = run_model(m, cuda, name, G)
    try:
        m.set_compute_dtype("bf16x3")
        assert m.backbone.compute_dtype == "bf16x3"
        feat, logits, idx = run_model(m, cuda, name, G)
    finally:
        m.set_compute_dtype(None)
    e_feat, e_logits = np.abs(feat.numpy() - G[fk]).max(), np.abs(logits.numpy() - G[lk]).max()
    print(f"{name} bf16x3: max abs error feat {e_feat:.3e}, logits {e_logits:.3e} (bar 1e-4; the arithmetic's own error in "
          f"float64: {BC.route_errors(name)['x3']:.3e})")
    assert tuple(feat.shape) == G[fk].shape and e_feat <= 1e-4 and e_logits <= 1e-4
    assert idx == ragged(G[ik])
    assert m.label_convertor.idx2str(idx) == m.label_convertor.idx2str(ragged(G[ik]))
    assert (bits(feat) != bits(exact)).any(), "the switch was ignored: every feature has the bits of the exact fp32 path"


def test_module_bf16_against_its_float64_restatement(cuda, vggs):
    G = BC.golden()
    m = vggs["crnn_tps"]
    # the VGG alone on the golden rectified images, which is what the restatement reads
    img, key = BC.vgg_input("crnn_tps", G)
    want = torch.from_numpy(G[key]).double()
    m.backbone.compute_dtype = torch.bfloat16
    try:
        with torch.no_grad(), GA.guarded(cuda) as g:
            feat = m.backbone(g.input(img))
            g.check(feat._base, require_guarded=True)
            logits = m.decoder(feat, None, None, None, train_mode=False)
    finally:
        m.backbone.compute_dtype = None
    rel = ((feat.cpu().double() - want).norm() / want.norm()).item()
    host = BC.route_errors("crnn_tps")["bf16_rel"]
    print(f"crnn_tps bf16: relative L2 error of the features {rel:.3e}; float64 restatement of the bf16 route {host:.3e}; "
          f"bar 2 x that = {2 * host:.3e}")
    idx, _ = m.label_convertor.tensor2idx(logits, CC.img_metas(CC.N))
    strings, golden = m.label_convertor.idx2str(idx), m.label_convertor.idx2str(ragged(G["idx_full"]))
    print(f"crnn_tps bf16: strings {strings} against the golden {golden} (compared, not asserted)")
    assert rel <= 2 * host


# ---- 7. the contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("width", [128, 32])
def test_bf16_image_at_widths_of_whole_16_byte_pieces(cuda, vggs, mode, width):
    """A bf16 image whose rows are whole 16-byte pieces sends conv0 (one channel of a 16-channel chunk) to the tiled kernel's
    wide-staging form in bf16 mode: the same bits as the fp32 image holding the same values, which takes the gather."""
    vgg = vggs["crnn_tps"].backbone
    as16 = torch.from_numpy(synth.smooth_image((3, 1, 32, width), f"crnn.bf16img{width}", 3)).to(torch.bfloat16)
    vgg.compute_dtype = mode
    try:
        with torch.no_grad(), GA.guarded(cuda) as g:
            a, b = vgg(g.input(as16)), vgg(g.input(as16.float()))
            g.check([a._base, b._base], require_guarded=True)
    finally:
        vgg.compute_dtype = None
    assert tuple(a.shape) == (3, 512, 1, width // 4 + 1)
    same(a, b, f"a bf16 image against the fp32 image of the same values, width {width}")



@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_contract_checks(cuda, vggs, mode):
    vgg = vggs["crnn_tps"].backbone
    batch = torch.from_numpy(synth.smooth_image((5, 1, 32, 100), "crnn.contract", 2))
    vgg.compute_dtype = mode
    try:
        with torch.no_grad(), GA.guarded(cuda) as g:
            five = vgg(g.input(batch))
            alone = vgg(g.input(batch[3:4]))
            g.check([five._base, alone._base], require_guarded=True)
            same(alone[0], five[3], "image 3 alone against image 3 of 5")
            empty = vgg(torch.zeros((0, 1, 32, 100), device=cuda))
            assert tuple(empty.shape) == (0, 512, 1, 26) and empty.dtype == torch.float32
            as16 = batch.to(torch.bfloat16)                     # the same values in both dtypes
            same(vgg(g.input(as16)), vgg(g.input(as16.float())), "a bf16 image against the fp32 image of the same values")
            with pytest.raises(ValueError, match="image height of 32"):
                vgg(torch.zeros((1, 1, 48, 100), device=cuda))
            # .train() and LeakyReLU: the PyTorch composition whatever the mode says
            # (PyTorch's GPU convolutions and batch statistics are not reproducible from call to call on this stack -- two
            # calls of `_forward_torch` differ in their last bits --, so "bit for bit" is held by identity: the tensor the
            # module returns IS the one `_forward_torch`'s composition, `self.cnn`, produced in that call)
            x = batch[:2].to(cuda)
            leaky = VeryDeepVgg(leaky_relu=True, input_channels=1).to(cuda).eval()
            leaky.compute_dtype = mode
            for mod, what in ((vgg.train(), ".train()"), (leaky, "leaky_relu=True")):
                made = []
                hook = mod.cnn.register_forward_hook(lambda _m, _i, out: made.append(out))
                try:
                    out = mod(x)
                    assert len(made) == 1 and out is made[0], f"{what} with a reduced mode set left the PyTorch composition"
                    assert mod._forward_torch(x) is made[1] and made[1].shape == out.shape
                finally:
                    hook.remove()
            vgg.eval()
            vgg.load_state_dict(BC.build_model("crnn_tps").backbone.state_dict())       # (BatchNorm's statistics moved)
            # the prepared weights follow the parameters
            before = vgg(x)
            same(vgg(x), before, "the same call twice")
            vgg.cnn.conv3.weight.mul_(1.5)
            after = vgg(x)
            assert (bits(after) != bits(before)).any(), "a weight changed in place and the result did not"
    finally:
        vgg.compute_dtype = None
        vgg.eval()
        vgg.load_state_dict(BC.build_model("crnn_tps").backbone.state_dict())
