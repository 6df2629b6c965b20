"""-m gpu: CRNNDecoder's training graph on the bf16 matrix cores (`set_train_compute_dtype("bf16x3")`): the saving recurrence
`tpspp_crnn_lstm_bf16_train_fwd`, the backward through time `tpspp_crnn_lstm_bf16_bwd`, the weight gradient
`tpspp_linear_bwd_weight_bf16` (include/tpspp.h), the layer `ops.crnn_bilstm_autograd(mode="bf16x3")` and the module.

Every kernel output is allocated through tests/guarded_alloc.py.  The references are the float64 restatements of
tests/crnn_dec_bf16_train_cases.py, whose docstring states the bars (`DC.bars`, unchanged); every error is printed with its
bar before it is asserted.  The kernels' split3 = 0 form is held at the kernel level only, on identical stored inputs."""

import pytest
import torch

import crnn_dec_bf16_cases as DC
import crnn_dec_bf16_train_cases as TC
import guarded_alloc as GA
import test_gpu_memory_safety as MS
import tps_pp_amd
from tps_pp_amd import _lib, ops
from tps_pp_amd.losses import CTCLoss

pytestmark = pytest.mark.gpu

BC, CC = DC.BC, DC.CC
H = DC.H
GROUPS = ops.CRNN_LSTM_GROUPS
MODES, MODE_IDS = DC.MODES, DC.MODE_IDS
SWEEP_NAMES = ("tpspp_crnn_lstm_bf16_train_fwd", "tpspp_crnn_lstm_bf16_bwd", "tpspp_linear_bwd_weight_bf16",
               "tpspp_linear_bwd_weight_bf16_workspace_floats")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def on_device(g, mw):
    return ops.MfmaWeight(g.input(mw.arranged), None if mw.bias is None else g.input(mw.bias), mw.rows, mw.k, mw.x3)


def image_bars(got, refs, mode, label, dim=1):
    bad = DC.bars(got, refs, mode, label)
    for n in range(got.shape[dim]):
        bad += DC.bars(got.select(dim, n), {k: v.select(dim, n) for k, v in refs.items()}, mode, f"{label} image {n}")
    return bad


def no_product_route(run, got):
    """T = 1: h_0 = 0 and nothing reads dh_rec, so no route rounds anything but zeros and the plain-bf16 restatement's error
    is fp32 storage rounding alone -- bars hung on it (2 x, 0.25 x) would ask fp32 kernels for float64 accuracy.  What is
    asked there instead: the plain-bf16 kernel gives the bits of the bf16x3 kernel, which is then held to the bf16x3 bar
    (whose floor, 2e-5, is an fp32-level bar).  -> the route to take the bars of."""
    for a, b in zip(got, run("bf16x3")):
        assert torch.equal(bits(a), bits(b)), "T = 1: the plain-bf16 kernel differs from the bf16x3 kernel"
    return "bf16x3"


# ---- 1. the saving forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("T,N,group", [(1, 1, 4), (2, 5, 0), (26, 17, 16), (27, 33, 8)])
def test_train_forward_keeps_the_eval_bits_and_stores_gates_and_cell(cuda, T, N, group, mode):
    xg, w_hh, _, fwd = TC.rec_case(T, N)
    mw = ops.arrange_mfma16(w_hh, x3=mode == "bf16x3")
    with GA.guarded(cuda) as g:
        a, x = on_device(g, mw), g.input(xg)
        want = ops.crnn_lstm_bf16(x, a, group)
        out, gates, cell = ops.crnn_lstm_bf16_train_fwd(x, a, group)
        g.check([want, out, gates, cell], require_guarded=True)
    assert tuple(gates.shape) == (T, N, 2, 4 * H) and tuple(cell.shape) == (T, N, 2, H)
    assert torch.equal(bits(out), bits(want)), "the saving forward's out differs from tpspp_crnn_lstm_bf16_fwd's"
    label = f"train fwd T={T} N={N} g={group}"
    if T == 1 and mode != "bf16x3":
        mode = no_product_route(lambda m: ops.crnn_lstm_bf16_train_fwd(xg.to(cuda), ops.arrange_mfma16(w_hh.to(cuda), x3=m == "bf16x3"),
                                                                     group), (out, gates, cell))
    bad = []
    for i, name in ((1, "gates"), (2, "cell"), (0, "out")):
        bad += DC.bars((out, gates, cell)[i].cpu(), {None: fwd[None][i], mode: fwd[mode][i]}, mode, f"{label} {name}")
    assert not bad, bad


# ---- 2. the backward through time ----------------------------------------------------------------------------------------------
BWD_CASES = [(T, 5, 0) for T in (1, 2, 9, 26)] + [(9, N, 0) for N in (1, 17, 33)] + \
            [(2, N, g) for g in GROUPS for N in (5, 17, 33) if N % g]


def run_bwd(cuda, d_out, gates, cell, w_hh, mode, group=0, stream=None):
    mw = ops.arrange_mfma16(w_hh.transpose(1, 2), x3=mode == "bf16x3")
    with GA.guarded(cuda) as g:
        args = (g.input(d_out), g.input(gates), g.input(cell), on_device(g, mw))
        if stream is None:
            d_xg = ops.crnn_lstm_bf16_bwd(*args, group)
        else:
            stream.wait_stream(torch.cuda.current_stream(cuda))
            with torch.cuda.stream(stream):
                d_xg = ops.crnn_lstm_bf16_bwd(*args, group)
            stream.synchronize()
        g.check(d_xg, require_guarded=True)
    return d_xg.cpu()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("T,N,group", BWD_CASES, ids=[f"T{T}-N{N}-g{g}" for T, N, g in BWD_CASES])
def test_backward_recurrence_against_the_bars(cuda, T, N, group, mode):
    d_out, gates, cell, w_hh, refs = TC.bwd_case(T, N, mode)
    got = run_bwd(cuda, d_out, gates, cell, w_hh, mode, group)
    assert tuple(got.shape) == (T, N, 2, 4 * H) and torch.isfinite(got).all()
    if T == 1 and mode != "bf16x3":
        mode = no_product_route(lambda m: (run_bwd(cuda, d_out, gates, cell, w_hh, m, group),), (got,))
        refs = {None: refs[None], mode: TC.bwd64(d_out, gates, cell, w_hh, mode)}
    bad = image_bars(got, refs, mode, f"bwd T={T} N={N} g={group}")
    assert not bad, bad


@pytest.fixture(scope="module")
def bwd_batch():
    """A batch that spans three blocks of the largest group, T = 3: the stored inputs of the bf16x3 route."""
    return TC.bwd_case(3, 2 * max(GROUPS) + 3, "bf16x3")[:4]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_backward_zero_gradient_gives_zero_bit_for_bit(cuda, bwd_batch, mode):
    d_out, gates, cell, w_hh = bwd_batch
    for zero in (torch.zeros_like(d_out), -torch.zeros_like(d_out)):
        for g in (0,) + GROUPS:
            got = run_bwd(cuda, zero, gates, cell, w_hh, mode, g)
            assert not bits(got).any(), f"g={g}: {int((bits(got) != 0).sum())} words are not +0.0"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_backward_image_is_independent_of_batch_position_and_group(cuda, bwd_batch, mode):
    d_out, gates, cell, w_hh = bwd_batch
    N = d_out.shape[1]

    def one(lo, hi, g=0):
        return run_bwd(cuda, d_out[:, lo:hi].contiguous(), gates[:, lo:hi].contiguous(), cell[:, lo:hi].contiguous(), w_hh, mode, g)
    alone = torch.cat([one(n, n + 1) for n in range(N)], 1)
    for g in (0,) + GROUPS:
        got = run_bwd(cuda, d_out, gates, cell, w_hh, mode, g)
        ne = (bits(got) != bits(alone)).flatten(2).any(2).any(0)
        assert not ne.any(), f"g={g}: images {ne.nonzero().flatten().tolist()} differ from their N = 1 run"
    for n in (0, 17, N - 1):
        for g in GROUPS:
            assert torch.equal(bits(one(n, n + 1, g)), bits(alone[:, n:n + 1])), (n, g)
    sub = one(16, 19, 4)
    assert torch.equal(bits(sub), bits(alone[:, 16:19]))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_backward_is_reproducible_over_calls_and_streams(cuda, bwd_batch, mode):
    d_out, gates, cell, w_hh = bwd_batch
    first = run_bwd(cuda, d_out, gates, cell, w_hh, mode)
    again = run_bwd(cuda, d_out, gates, cell, w_hh, mode)
    side = run_bwd(cuda, d_out, gates, cell, w_hh, mode, stream=torch.cuda.Stream(cuda))
    assert torch.equal(bits(first), bits(again)) and torch.equal(bits(first), bits(side))


# ---- 2b. one body for every precision --------------------------------------------------------------------------------------------
# At T = 1 neither recurrence multiplies anything that matters (the forward's h_0 is zero, the backward leaves before its
# product), so all that runs is the part the fp32 and the bf16 kernels share -- and they must agree to the bit.  N = 5 with
# g = 4 has a partial block, N = 17 with g = 16 one full block plus one image.
T1_CASES = [(N, g) for N in (1, 5, 17) for g in (0, 4, 16)]


def t1_case(N):
    gen = torch.Generator().manual_seed(7100 + N)
    xg = torch.randn((1, N, 2, 4 * H), generator=gen)
    assert not (xg == 0).any()          # the sign of a zero pre-activation may differ between an fp32 and a bf16 sum of zeros
    return xg, torch.randn((2, 4 * H, H), generator=gen) / 16, torch.randn((1, N, 2 * H), generator=gen)


@pytest.mark.parametrize("N,group", T1_CASES)
def test_one_step_forward_gives_the_same_bits_in_every_precision(cuda, N, group):
    xg, w_hh, _ = t1_case(N)
    with GA.guarded(cuda) as g:
        x, w = g.input(xg), g.input(w_hh)
        want, plain = ops.crnn_lstm_train_fwd(x, w, group), ops.crnn_lstm(x, w, group)
        got = {}
        for mode in MODES:
            a = on_device(g, ops.arrange_mfma16(w_hh, x3=mode == "bf16x3"))
            got[mode] = ops.crnn_lstm_bf16_train_fwd(x, a, group) + (ops.crnn_lstm_bf16(x, a, group),)
        g.check(list(want) + [plain] + [t for v in got.values() for t in v], require_guarded=True)
    assert torch.equal(bits(plain), bits(want[0])), "crnn_lstm's out differs from crnn_lstm_train_fwd's"
    for mode, v in got.items():
        for name, a, b in zip(("out", "gates", "cell", "out of crnn_lstm_bf16"), want + (plain,), v):
            assert torch.equal(bits(a), bits(b)), f"{mode}: {name} differs from the fp32 kernel's"


@pytest.mark.parametrize("N,group", T1_CASES)
def test_one_step_backward_gives_the_same_bits_in_every_precision(cuda, N, group):
    xg, w_hh, d_out = t1_case(N)
    _, gates, cell = ops.crnn_lstm_train_fwd(xg.to(cuda), w_hh.to(cuda), group)
    gates, cell = gates.cpu(), cell.cpu()
    with GA.guarded(cuda) as g:
        d_xg, d_dir = ops.crnn_lstm_bwd(g.input(d_out), g.input(gates), g.input(cell), g.input(w_hh.transpose(1, 2).contiguous()),
                                        group, direction_major=True)
        g.check([d_xg, d_dir], require_guarded=True)
    assert torch.equal(bits(d_dir), bits(d_xg.permute(2, 0, 1, 3))), "d_xg_dir is not d_xg, direction-major"
    for mode in MODES:
        got = run_bwd(cuda, d_out, gates, cell, w_hh, mode, group)
        assert torch.equal(bits(got), bits(d_xg)), f"{mode}: d_xg differs from the fp32 kernel's"


# ---- 3. the weight gradient ---------------------------------------------------------------------------------------------------
def run_wg(cuda, make, batch, M, O, K, mode, stream=None):
    """`make(put)` -> (dy view, dy strides, x view, x strides) on the device."""
    with GA.guarded(cuda) as g:
        dy, sd, x, sx = make(g.input)
        if stream is None:
            dw = ops.linear_bwd_weight_bf16(dy, sd, x, sx, batch, M, O, K, mode == "bf16x3")
        else:
            stream.wait_stream(torch.cuda.current_stream(cuda))
            with torch.cuda.stream(stream):
                dw = ops.linear_bwd_weight_bf16(dy, sd, x, sx, batch, M, O, K, mode == "bf16x3")
            stream.synchronize()
        g.check(dw, require_guarded=True)
    return dw.cpu()


def wg_refs(dy2, x2, mode):
    return {m: TC.dweight64(dy2.double() if m is None else dy2, x2.double() if m is None else x2, m) for m in (None, mode)}


def dense_case(batch, M, O, K, seed):
    dy, x = DC.rnd((batch, M, O), seed), DC.rnd((batch, M, K), seed + 1)
    return (lambda put: (put(dy), (M * O, O, 1), put(x), (M * K, K, 1))), dy.reshape(-1, O), x.reshape(-1, K)


def sliced_case(batch, M, O, K, seed):
    """Views with non-unit row strides: every second row of a wider tensor, columns cut out of wider rows."""
    dy, x = DC.rnd((batch, 2 * M, O + 8), seed), DC.rnd((batch, 2 * M, K + 4), seed + 1)

    def make(put):
        a, b = put(dy)[:, ::2, 4:4 + O], put(x)[:, ::2, :K]
        return a, a.stride(), b, b.stride()
    return make, dy[:, ::2, 4:4 + O].reshape(-1, O), x[:, ::2, :K].reshape(-1, K)


def shifted_case(T, N, d, seed):
    """The two operand pairs of d w_hh: d_xg (T, N, 2, 4H) and out (T, N, 2H), shifted by one step against each other."""
    d_xg, out = DC.rnd((T, N, 2, 4 * H), seed), DC.rnd((T, N, 2 * H), seed + 1)
    pick = (lambda a, b: (a[1:, :, 0], b[:-1, :, :H])) if d == 0 else (lambda a, b: (a[:-1, :, 1], b[1:, :, H:]))

    def make(put):
        a, b = pick(put(d_xg), put(out))
        return a, a.stride(), b, b.stride()
    a, b = pick(d_xg, out)
    return make, a.reshape(-1, 4 * H), b.reshape(-1, H)


def nchw_case(W, N, O, K, seed):
    """X read as the tokens (t, n, c) = feat[n, c, 0, t] of an (N, K, 1, W + 1) map sliced to W; dy dense (W, N, O)."""
    dy, full = DC.rnd((W, N, O), seed), DC.rnd((N, K, 1, W + 1), seed + 1)

    def make(put):
        feat = put(full)[:, :, :, :W]
        sn, sc, _, sw = feat.stride()
        return put(dy), (N * O, O, 1), feat, (sw, sn, sc)
    return make, dy.reshape(-1, O), full[:, :, 0, :W].permute(2, 0, 1).reshape(-1, K)


WG_CASES = {"1x1-128x128": lambda: (1, 1, 128, 128) + dense_case(1, 1, 128, 128, 40),
            "1x5-128x256": lambda: (1, 5, 128, 256) + dense_case(1, 5, 128, 256, 42),
            "3x17-256x128-sliced": lambda: (3, 17, 256, 128) + sliced_case(3, 17, 256, 128, 44),
            "9x17-1024x256-shifted-fwd": lambda: (9, 17, 1024, 256) + shifted_case(10, 17, 0, 46),
            "9x17-1024x256-shifted-rev": lambda: (9, 17, 1024, 256) + shifted_case(10, 17, 1, 48),
            "26x5-2048x512-nchw": lambda: (26, 5, 2048, 512) + nchw_case(26, 5, 2048, 512, 50)}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", list(WG_CASES))
def test_weight_gradient_against_the_bars(cuda, case, mode):
    batch, M, O, K, make, dy2, x2 = WG_CASES[case]()
    got = run_wg(cuda, make, batch, M, O, K, mode)
    assert tuple(got.shape) == (O, K)
    bad = DC.bars(got, wg_refs(dy2, x2, mode), mode, f"dW {case}")
    assert not bad, bad
    again = run_wg(cuda, make, batch, M, O, K, mode)
    side = run_wg(cuda, make, batch, M, O, K, mode, stream=torch.cuda.Stream(cuda))
    assert torch.equal(bits(got), bits(again)) and torch.equal(bits(got), bits(side)), "not reproducible over calls and streams"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_weight_gradient_of_no_rows_is_plus_zero(cuda, mode):
    dy, x = torch.zeros((1, 1, 256)), torch.zeros((1, 1, 128))
    for batch, M in ((0, 5), (3, 0)):
        got = run_wg(cuda, lambda put: (put(dy), (256, 256, 1), put(x), (128, 128, 1)), batch, M, 256, 128, mode)
        assert tuple(got.shape) == (256, 128) and not bits(got).any()
    assert ops.linear_bwd_weight_bf16_workspace_floats(0, 5, 256, 128) == 0


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("batch,M", [(1, 1), (3, 17), (1, 64), (2, 31)])
def test_weight_gradient_of_small_integers_is_exact(cuda, batch, M, mode):
    """Integers in [-4, 4] are bf16 numbers and every partial sum is an fp32 number: the float64 product, bit for bit."""
    O, K = 256, 128
    g = torch.Generator().manual_seed(60 + M)
    dy = torch.randint(-4, 5, (batch, M, O), generator=g).float()
    x = torch.randint(-4, 5, (batch, M, K), generator=g).float()
    got = run_wg(cuda, lambda put: (put(dy), (M * O, O, 1), put(x), (M * K, K, 1)), batch, M, O, K, mode)
    want = (dy.reshape(-1, O).double().t() @ x.reshape(-1, K).double()).float()
    assert torch.equal(bits(got), bits(want + 0.0))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_weight_gradient_does_not_depend_on_how_the_rows_are_cut(cuda, mode):
    R, O, K = 9 * 17 * 4, 1024, 256                                 # 612 rows: more than one slice
    assert ops.linear_bwd_weight_bf16_workspace_floats(1, R, O, K) > 0
    dy, x = DC.rnd((R, O), 70), DC.rnd((R, K), 71)
    outs = []
    for batch, M in ((1, R), (R, 1), (36, 17), (4, 153)):
        outs.append(run_wg(cuda, lambda put: (put(dy), (M * O, O, 1), put(x), (M * K, K, 1)), batch, M, O, K, mode))
    assert all(torch.equal(bits(o), bits(outs[0])) for o in outs[1:])
    bad = DC.bars(outs[0], wg_refs(dy, x, mode), mode, f"dW {R} rows, sliced")
    assert not bad, bad


# ---- 4. the layer ---------------------------------------------------------------------------------------------------------------
def lstm_on(cuda, K):
    w_ih, b, w_hh = DC.pytorch_lstm(K)
    m = TC.lstm_module64((w_ih, b, w_hh)).float()
    with torch.no_grad():                                           # b_ih + b_hh = b with both halves non-zero
        for sfx in ("", "_reverse"):
            half = getattr(m, "bias_ih_l0" + sfx) * 0.5
            getattr(m, "bias_ih_l0" + sfx).copy_(half)
            getattr(m, "bias_hh_l0" + sfx).copy_(half)
    return m.to(cuda)


PARAMS = ("weight_ih_l0", "weight_ih_l0_reverse", "weight_hh_l0", "weight_hh_l0_reverse", "bias_ih_l0", "bias_hh_l0",
          "bias_ih_l0_reverse", "bias_hh_l0_reverse")


LAYER_CASES = [(K, T, N, False) for K in (256, 512) for T, N in ((1, 1), (2, 5), (26, 17))] + \
              [(512, T, N, True) for T, N in ((1, 1), (2, 5), (26, 17))]           # the feature map is layer 0's operand


@pytest.mark.parametrize("K,T,N,nchw", LAYER_CASES, ids=[f"K{K}-T{T}-N{N}-{'nchw' if v else 'dense'}" for K, T, N, v in LAYER_CASES])
def test_layer_bf16x3_against_float64_autograd(cuda, K, T, N, nchw):
    mode = "bf16x3"
    x, d_out, grads, _ = TC.layer_case(K, T, N)
    m = lstm_on(cuda, K)
    with GA.guarded(cuda) as g:
        if nchw:
            full = torch.cat([x.permute(1, 2, 0).unsqueeze(2), DC.rnd((N, K, 1, 1), 5)], 3)         # (N, K, 1, T + 1)
            leaf = g.input(full).requires_grad_(True)
            feat = leaf[:, :, :, :T]
            sn, sc, _, sw = feat.stride()
            out = ops.crnn_bilstm_autograd(feat, (T, N, sw, sn, sc), T, N, m, mode=mode)
        else:
            leaf = g.input(x).requires_grad_(True)
            out = ops.crnn_bilstm_autograd(leaf, (T, N, N * K, K, 1), T, N, m, mode=mode)
        out.backward(g.input(d_out))
        g.check([out, leaf.grad])
    dx = leaf.grad.cpu()
    if nchw:
        assert not bits(dx[:, :, :, T:]).any(), "the column outside the view receives no gradient"
        dx = dx[:, :, 0, :T].permute(2, 0, 1)
    p = {n: getattr(m, n).grad.cpu() for n in PARAMS}
    got = {"dx": dx, "dw_ih": torch.cat([p["weight_ih_l0"], p["weight_ih_l0_reverse"]]),
           "dw_hh": torch.stack([p["weight_hh_l0"], p["weight_hh_l0_reverse"]]),
           "db": torch.cat([p["bias_ih_l0"], p["bias_ih_l0_reverse"]])}
    label = f"layer K={K} T={T} N={N} {'nchw' if nchw else 'dense'}"
    bad = []
    for key in TC.GRAD_KEYS:
        if key == "dw_hh" and T == 1:
            assert not bits(got[key]).any(), "T = 1: d w_hh is +0"
            continue
        bad += DC.bars(got[key], {None: grads[None][key], mode: grads[mode][key]}, mode, f"{label} {key}")
    for sfx in ("", "_reverse"):
        a, b = getattr(m, "bias_ih_l0" + sfx).grad, getattr(m, "bias_hh_l0" + sfx).grad
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), "b_ih and b_hh: equal values in tensors of their own"
    assert not bad, bad


# ---- 5. the module --------------------------------------------------------------------------------------------------------------
def test_module_bf16x3_training_on_the_golden_features(cuda):
    mode = "bf16x3"
    G = BC.golden()
    m = BC.build_model("crnn_tps", cuda).train()
    assert m.set_train_backend("torch", decoder="hip", loss="hip") is m
    dec, loss_mod = m.decoder, m.loss
    conv = tps_pp_amd.CTCConvertor(dict_type="DICT36", with_unknown=False, lower=True)
    td, metas = conv.str2tensor(CC.TEXTS), CC.img_metas(CC.N)
    feat = torch.from_numpy(G["feat"]).float()

    def run(leaf):
        dec.zero_grad()
        with GA.guarded(cuda) as g:
            loss = loss_mod(dec(leaf, None, None, None, train_mode=True), td, metas)["loss_ctc"]
            loss.backward()
            g.check([loss, leaf.grad, [p.grad for p in dec.parameters()]])
        return loss.detach().cpu(), {k: p.grad.cpu().clone() for k, p in dec.named_parameters()}

    def called(fn):
        """(result of fn, names of the library functions it fetched): the sweep's call recorder around one run."""
        real = _lib.lib()
        del MS._NOW[:]
        _lib._lib = MS._Spy(real)
        try:
            return fn(), set(MS._NOW)
        finally:
            _lib._lib = real

    before, names = called(lambda: run(feat.to(cuda).requires_grad_(True)))
    assert "tpspp_crnn_lstm_bwd" in names and not names & set(SWEEP_NAMES), "None: no new entry point is called"
    assert m.set_train_compute_dtype(decoder=mode) is m and dec.train_lstm_dtype == mode
    got, names = called(lambda: run(feat.to(cuda).requires_grad_(True)))
    assert set(SWEEP_NAMES) <= names and not names & {"tpspp_crnn_lstm_bwd", "tpspp_crnn_lstm_train_fwd"}, sorted(names)
    m.set_train_compute_dtype(decoder=None)
    after = run(feat.to(cuda).requires_grad_(True))
    assert torch.equal(bits(after[0]), bits(before[0])) and all(torch.equal(bits(after[1][k]), bits(before[1][k])) for k in before[1]), \
        "the fp32 training graph moved after a mode round trip"
    assert any((bits(got[1][k]) != bits(before[1][k])).any() for k in got[1]), "the switch was ignored"

    host = BC.build_model("crnn_tps").decoder
    ctc = CTCLoss()
    refs = {r: TC.decoder_grads64(host, feat, lambda lg: ctc(lg, td, metas)["loss_ctc"], r) for r in (None, mode)}
    assert set(refs[None][1]) == set(got[1]) and len(got[1]) == 20
    bad = DC.bars(got[0], {r: refs[r][0] for r in refs}, mode, "module loss_ctc")
    for k in sorted(got[1]):
        bad += DC.bars(got[1][k], {r: refs[r][1][k] for r in refs}, mode, f"module d {k}")
    assert not bad, bad

    # one SGD step in the mode lowers the loss
    m.set_train_compute_dtype(decoder=mode)
    leaf = feat.to(cuda)
    opt = torch.optim.SGD(dec.parameters(), lr=1e-3)
    opt.zero_grad()
    loss0 = loss_mod(dec(leaf, None, None, None, train_mode=True), td, metas)["loss_ctc"]
    loss0.backward()
    opt.step()
    loss1 = loss_mod(dec(leaf, None, None, None, train_mode=True), td, metas)["loss_ctc"]
    print(f"loss_ctc {loss0.item():.4f} -> {loss1.item():.4f}")
    assert loss1.item() < loss0.item()
    # the eval path ignores the switch
    dec.eval()
    twin = BC.build_model("crnn_tps", cuda).decoder.eval()
    twin.load_state_dict(dec.state_dict())
    with torch.no_grad():
        assert torch.equal(bits(dec(leaf, None, None, None, train_mode=False)), bits(twin(leaf, None, None, None, train_mode=False)))


# ---- 6. the four entry points in the memory-safety sweep ------------------------------------------------------------------------
# As tests/test_gpu_crnn_dec_bf16.py does: entered in the registry when this module is imported, and one case through the
# sweep's own `run_twice` whose guarded run really reaches all four (the Python wrapper calls the workspace query).
for _name in SWEEP_NAMES:
    if "test_decoder_bf16_training_entry_points_in_the_sweep" not in MS.SWEPT.setdefault(_name, []):
        MS.SWEPT[_name].append("test_decoder_bf16_training_entry_points_in_the_sweep")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("T,N,group", [(26, 5, 0), (3, 17, 16), (1, 1, 4)])
def test_decoder_bf16_training_entry_points_in_the_sweep(cuda, T, N, group, mode):
    """The saving forward, the backward and the weight gradients of one layer on the sliced NCHW operand of layer 0, ragged
    against the 32-row k step, the 128-wide tile and the group."""
    w_ih, b, w_hh = DC.pytorch_lstm(512)
    x3 = mode == "bf16x3"
    full = DC.rnd((N, 512, 1, T + 1), 400 + N)
    d_out = DC.rnd((T, N, 2 * H), 401 + N)

    def fn(put):
        a_ih, a_hh = ops.arrange_mfma16(w_ih, b, x3=x3), ops.arrange_mfma16(w_hh, x3=x3)
        a_t = ops.arrange_mfma16(w_hh.transpose(1, 2), x3=x3)
        a_ih = ops.MfmaWeight(put(a_ih.arranged), put(a_ih.bias), a_ih.rows, a_ih.k, x3)
        a_hh = ops.MfmaWeight(put(a_hh.arranged), None, a_hh.rows, a_hh.k, x3)
        a_t = ops.MfmaWeight(put(a_t.arranged), None, a_t.rows, a_t.k, x3)
        feat = put(full)[:, :, :, :T]
        sn, sc, _, sw = feat.stride()
        xg = ops.linear_bf16_fwd(feat, (T, N, sw, sn, sc), a_ih).view(T, N, 2, 4 * H)
        out, gates, cell = ops.crnn_lstm_bf16_train_fwd(xg, a_hh, group)
        d_xg = ops.crnn_lstm_bf16_bwd(put(d_out), gates, cell, a_t, group)
        dw_ih = ops.linear_bwd_weight_bf16(d_xg, (N * 8 * H, 8 * H, 1), feat, (sw, sn, sc), T, N, 8 * H, 512, x3)
        res = [xg, out, gates, cell, d_xg, dw_ih]
        if T > 1:
            sd, sx = (N * 8 * H, 8 * H, 1), (N * 2 * H, 2 * H, 1)
            res.append(ops.linear_bwd_weight_bf16(d_xg[1:, :, 0], sd, out[:-1, :, :H], sx, T - 1, N, 4 * H, H, x3))
            res.append(ops.linear_bwd_weight_bf16(d_xg[:-1, :, 1], sd, out[1:, :, H:], sx, T - 1, N, 4 * H, H, x3))
        return res
    del MS._NOW[:]
    MS.run_twice(cuda, fn)
    assert set(SWEEP_NAMES) <= set(MS._NOW), f"the guarded run never called {sorted(set(SWEEP_NAMES) - set(MS._NOW))}"


def test_the_sweep_registry_names_all_four_entry_points():
    from test_capi_symbols import header_functions
    assert set(SWEEP_NAMES) <= set(header_functions()) and all(MS.SWEPT.get(n) for n in SWEEP_NAMES)
