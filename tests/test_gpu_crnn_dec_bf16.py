"""-m gpu: CRNNDecoder's reduced-precision eval path (`set_compute_dtype("bf16x3" | torch.bfloat16)`): the recurrence on
`tpspp_crnn_lstm_bf16_fwd`, the input projection on `tpspp_mm_bf16` (include/tpspp.h), and the module.

Every kernel output is allocated through tests/guarded_alloc.py: nothing is written outside it and every element of it is
written.  The references are the float64 restatements of tests/crnn_dec_bf16_cases.py, whose docstring states the bars; every
error is printed with its bar before it is asserted."""
import numpy as np
import pytest
import torch

import crnn_dec_bf16_cases as DC
import guarded_alloc as GA
from tps_pp_amd import _lib, ops

pytestmark = pytest.mark.gpu

BC, CC = DC.BC, DC.CC
H = DC.H
GROUPS = ops.CRNN_LSTM_GROUPS
MODES, MODE_IDS = DC.MODES, DC.MODE_IDS


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def on_device(g, mw):
    """An `ops.MfmaWeight` made on the host, copied between the guard's NaN bands."""
    return ops.MfmaWeight(g.input(mw.arranged), None if mw.bias is None else g.input(mw.bias), mw.rows, mw.k, mw.x3)


def arranged(weights, mode):
    w_ih, b, w_hh = weights
    x3 = mode == "bf16x3"
    return ops.arrange_mfma16(w_ih, b, x3=x3), ops.arrange_mfma16(w_hh, x3=x3)


# ---- 1. the recurrence, behind its projection, against the bars ------------------------------------------------------------
LAYER_CASES = [(K, T, 5, 0) for K in (256, 512) for T in (1, 2, 26, 27)] + \
              [(K, 26, N, 0) for K in (256, 512) for N in (1, 17, 33)] + \
              [(256, 2, N, g) for g in GROUPS for N in (5, 17, 33) if N % g] + \
              [(512, 27, 17, g) for g in GROUPS]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K,T,N,group", LAYER_CASES, ids=[f"K{K}-T{T}-N{N}-g{g}" for K, T, N, g in LAYER_CASES])
def test_layer_against_the_bars(cuda, K, T, N, group, mode):
    x, refs = DC.layer_case(K, T, N)
    a_ih, a_hh = arranged(DC.pytorch_lstm(K), mode)
    with GA.guarded(cuda) as g:
        xg = ops.linear_bf16_fwd(g.input(x), (T, N, N * K, K, 1), on_device(g, a_ih)).view(T, N, 2, 4 * H)
        got = ops.crnn_lstm_bf16(xg, on_device(g, a_hh), group)
        g.check([xg, got], require_guarded=True)
    got = got.cpu()
    assert tuple(got.shape) == (T, N, 2 * H) and torch.isfinite(got).all()
    label = f"layer K={K} T={T} N={N} g={group}"
    bad = DC.bars(got, refs, mode, label)
    for n in range(N):
        bad += DC.bars(got[:, n], {k: v[:, n] for k, v in refs.items()}, mode, f"{label} image {n}")
    assert not bad, bad


# ---- 2. the recurrence's properties -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def xg_batch():
    """A batch that spans three blocks of the largest group: xg (3, 35, 2, 4H), and w_hh at twice PyTorch's scale."""
    return DC.rnd((3, 2 * max(GROUPS) + 3, 2, 4 * H), 77, 2.0), 2.0 * DC.pytorch_lstm(256)[2]


def run_lstm(cuda, xg, w_hh, mode, group=0):
    mw = ops.arrange_mfma16(w_hh, x3=mode == "bf16x3")
    with GA.guarded(cuda) as g:
        out = ops.crnn_lstm_bf16(g.input(xg), on_device(g, mw), group)
        g.check(out, require_guarded=True)
    return out.cpu()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_zero_input_gives_zero_output_bit_for_bit(cuda, xg_batch, mode):
    xg, w_hh = xg_batch
    for g in (0,) + GROUPS:
        out = run_lstm(cuda, torch.zeros_like(xg), w_hh, mode, g)
        assert not bits(out).any(), f"g={g}: {int((bits(out) != 0).sum())} words are not +0.0"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_image_is_independent_of_batch_position_and_group(cuda, xg_batch, mode):
    xg, w_hh = xg_batch
    N = xg.shape[1]
    alone = torch.cat([run_lstm(cuda, xg[:, n:n + 1].contiguous(), w_hh, mode) for n in range(N)], 1)
    for g in (0,) + GROUPS:
        out = run_lstm(cuda, xg, w_hh, mode, g)
        ne = (bits(out) != bits(alone)).flatten(2).any(2).any(0)
        assert not ne.any(), f"g={g}: images {ne.nonzero().flatten().tolist()} differ from their N = 1 run"
    for n in (0, 17, N - 1):                                       # ... and alone under every group size, and mid-batch
        for g in GROUPS:
            assert torch.equal(bits(run_lstm(cuda, xg[:, n:n + 1].contiguous(), w_hh, mode, g)), bits(alone[:, n:n + 1])), (n, g)
        sub = run_lstm(cuda, xg[:, n:n + 2].contiguous() if n + 2 <= N else xg[:, n - 1:n + 1].contiguous(), w_hh, mode, 4)
        assert torch.equal(bits(sub[:, 0 if n + 2 <= N else 1]), bits(alone[:, n]))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_directions_run_the_right_way(cuda, xg_batch, mode):
    _, w_hh = xg_batch
    T, N = 5, 6
    xg = DC.rnd((T, N, 2, 4 * H), 78, 2.0)
    t0, n0 = 2, 4
    base = run_lstm(cuda, xg, w_hh, mode)
    pert = xg.clone()
    pert[t0, n0] += 0.5
    out = run_lstm(cuda, pert, w_hh, mode)
    same = bits(out) == bits(base)
    others = [n for n in range(N) if n != n0]
    assert same[:, others].all(), "another image changed"
    fwd, rev = same[:, n0, :H], same[:, n0, H:]
    assert fwd[:t0].all() and not fwd[t0:].all(1).any(), "forward half: identical before t0, changed from t0 on"
    assert rev[t0 + 1:].all() and not rev[:t0 + 1].all(1).any(), "reverse half: identical after t0, changed up to t0"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_saturated_gates_stay_finite_and_within_the_bar(cuda, xg_batch, mode):
    _, w_hh = xg_batch
    xg = DC.rnd((4, 5, 2, 4 * H), 79, 400.0)                       # most pre-activations beyond +-100
    assert (xg.abs() > 100).float().mean() > 0.7
    refs = {m: DC.lstm64(xg.double() if m is None else xg, w_hh, m) for m in (None, mode)}
    got = run_lstm(cuda, xg, w_hh, mode)
    assert torch.isfinite(got).all()
    bad = DC.bars(got, refs, mode, "lstm saturated")
    huge = run_lstm(cuda, torch.where(xg > 0, torch.tensor(3.0e38), torch.tensor(-3.0e38)), w_hh, mode)
    assert torch.isfinite(huge).all() and huge.abs().max() <= 1.0
    assert not bad, bad


def test_wrapper_argument_checks(cuda):
    w_hh = DC.pytorch_lstm(256)[2]
    mw = ops.arrange_mfma16(w_hh.to(cuda))
    xg = torch.zeros((2, 3, 2, 4 * H), device=cuda)
    with pytest.raises(TypeError, match="MfmaWeight"):
        ops.crnn_lstm_bf16(xg, w_hh.to(cuda))
    with pytest.raises(TypeError, match="MfmaWeight"):
        ops.crnn_lstm_bf16(xg, ops.arrange_mfma16(w_hh[0].to(cuda)))
    with pytest.raises(ValueError, match="crnn_lstm_bf16"):
        ops.crnn_lstm_bf16(xg[..., :512].contiguous(), mw)
    with pytest.raises(_lib.TpsppError, match="GPU tensor"):
        ops.crnn_lstm_bf16(xg.cpu(), mw)
    with pytest.raises(_lib.TpsppError, match="images_per_group"):
        ops.crnn_lstm_bf16(xg, mw, 5)
    assert tuple(ops.crnn_lstm_bf16(xg[:, :0].contiguous(), mw).shape) == (2, 0, 2 * H)
    with pytest.raises(TypeError, match="MfmaWeight"):
        ops.mm_bf16(xg, (0, 1024, 1), mw, xg, (0, 1024, 1), 1, 4)
    with pytest.raises(_lib.TpsppError, match="N a multiple of 128"):
        w = ops.arrange_mfma16(torch.zeros((64, 32), device=cuda))
        ops.linear_bf16_fwd(torch.zeros((4, 32), device=cuda), ops._dense(4, 32), w)


# ---- the two entry points in the memory-safety sweep ------------------------------------------------------------------------
# tests/test_memory_safety_host.py holds every entry point of include/tpspp.h to a guard case named in
# `test_gpu_memory_safety.SWEPT`.  These two have theirs here: the case below goes through the sweep's own `run_twice`
# (a plain run, then a guarded run behind the call recorder: guards intact, nothing unwritten, the same bits), and it is
# entered in the registry when this module is imported, which collecting the suite does.
import test_gpu_memory_safety as MS  # noqa: E402

SWEEP_NAMES = ("tpspp_mm_bf16", "tpspp_crnn_lstm_bf16_fwd")
for _name in SWEEP_NAMES:
    if "test_decoder_bf16_entry_points_in_the_sweep" not in MS.SWEPT.setdefault(_name, []):
        MS.SWEPT[_name].append("test_decoder_bf16_entry_points_in_the_sweep")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("T,N,W,group", [(26, 5, 26, 0), (3, 17, 9, 16), (1, 1, 1, 4)])
def test_decoder_bf16_entry_points_in_the_sweep(cuda, T, N, W, group, mode):
    """One layer on the sliced NCHW operand of layer 0 (T = W tokens per image) and on a dense one, ragged against the 64-row
    tile and the group."""
    w_ih, b, w_hh = DC.pytorch_lstm(512)
    x3 = mode == "bf16x3"
    full = DC.rnd((N, 512, 1, W + 1), 300 + N)
    dense = DC.rnd((T, N, 512), 301 + N)

    def fn(put):
        a_ih = ops.arrange_mfma16(w_ih, b, x3=x3)
        a_hh = ops.arrange_mfma16(w_hh, x3=x3)
        a_ih = ops.MfmaWeight(put(a_ih.arranged), put(a_ih.bias), a_ih.rows, a_ih.k, x3)
        a_hh = ops.MfmaWeight(put(a_hh.arranged), None, a_hh.rows, a_hh.k, x3)
        feat = put(full)[:, :, :, :W]
        sn, sc, _, sw = feat.stride()
        xg0 = ops.linear_bf16_fwd(feat, (W, N, sw, sn, sc), a_ih)
        xg1 = ops.linear_bf16_fwd(put(dense), (T, N, N * 512, 512, 1), a_ih)
        return (xg0, xg1, ops.crnn_lstm_bf16(xg0.view(W, N, 2, 4 * H), a_hh, group),
                ops.crnn_lstm_bf16(xg1.view(T, N, 2, 4 * H), a_hh, group))
    del MS._NOW[:]
    MS.run_twice(cuda, fn)
    assert set(SWEEP_NAMES) <= set(MS._NOW), f"the guarded run never called {sorted(set(SWEEP_NAMES) - set(MS._NOW))}"


def test_the_sweep_registry_names_both_entry_points():
    from test_capi_symbols import header_functions
    assert set(SWEEP_NAMES) <= set(header_functions()) and all(MS.SWEPT.get(n) for n in SWEEP_NAMES)


# ---- 3. the projection against its float64 restatement -----------------------------------------------------------------------
def proj_refs(x, w, b):
    return {m: DC.proj64(x.double() if m is None else x, w, b, m) for m in [None] + MODES}


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K,rows", [(256, 26 * 5), (512, 67), (256, 1), (512, 64)])
def test_projection_of_a_dense_operand(cuda, K, rows, mode):
    w_ih, b, _ = DC.pytorch_lstm(K)
    x = DC.rnd((rows, K), 31 + rows)
    refs = proj_refs(x, w_ih, b)
    with GA.guarded(cuda) as g:
        mw = on_device(g, ops.arrange_mfma16(w_ih, b, x3=mode == "bf16x3"))
        got = ops.linear_bf16_fwd(g.input(x), ops._dense(rows, K), mw)
        # the same rows one float off the 16-byte alignment: the staging that reads float by float
        shifted = g.input(torch.cat([torch.zeros(1), x.flatten()]))[1:].view(rows, K)
        again = ops.linear_bf16_fwd(shifted, ops._dense(rows, K), mw)
        g.check([got, again], require_guarded=True)
    assert tuple(got.shape) == (rows, 8 * H) and shifted.data_ptr() % 16 == 4
    assert torch.equal(bits(again), bits(got)), "a misaligned operand of the same values"
    bad = DC.bars(got.cpu(), refs, mode, f"projection dense K={K} rows={rows}")
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("W", [9, 26])
def test_projection_reads_the_sliced_nchw_map(cuda, W, N, mode):
    """Layer 0's operand: token (t, n, c) = feat[n, c, 0, t] of the (N, 512, 1, W) view of a (N, 512, 1, W + 1) map -- k at a
    stride of W + 1 floats, t at a stride of 1 -- written into a C whose rows are wider than the product: only the addressed
    elements may change."""
    K = 512
    w_ih, b, _ = DC.pytorch_lstm(K)
    full = DC.rnd((N, K, 1, W + 1), 900 + 10 * W + N)
    tokens = full[:, :, 0, :W].permute(2, 0, 1).contiguous()           # (W, N, K)
    refs = proj_refs(tokens.reshape(W * N, K), w_ih, b)
    O, ld = 8 * H, 8 * H + 24
    with GA.guarded(cuda) as g:
        feat = g.input(full)[:, :, :, :W]
        sn, sc, _, sw = feat.stride()
        assert (sw, sc) == (1, W + 1)
        mw = on_device(g, ops.arrange_mfma16(w_ih, b, x3=mode == "bf16x3"))
        dense = ops.linear_bf16_fwd(feat, (W, N, sw, sn, sc), mw)
        wide = g.input(torch.full((W * N, ld), 7.0))
        ops.mm_bf16(feat, (sw, sn, sc), mw, wide, (N * ld, ld, 1), W, N)
        g.check([dense, wide], require_guarded=True)
    dense, wide = dense.cpu(), wide.cpu()
    assert torch.equal(bits(wide[:, :O]), bits(dense)) and (wide[:, O:] == 7.0).all()
    bad = DC.bars(dense, refs, mode, f"projection NCHW W={W} N={N}")
    assert not bad, bad


# ---- 4. the module -------------------------------------------------------------------------------------------------------------
KEYS = {"crnn_tps": ("feat", "logits", "idx_full"), "crnn": ("feat32", "logits32", "idx32")}


@pytest.fixture(scope="module")
def models(cuda):
    return {name: BC.build_model(name, cuda) for name in KEYS}


def ragged(idx):
    return [r[r >= 0].tolist() for r in idx]


def vgg_and_decoder(m, cuda, img):
    """(features, logits, decoded indices): the VGG on `img`, the decoder's eval path on its features."""
    with torch.no_grad(), GA.guarded(cuda) as g:
        feat = m.backbone(g.input(img))
        logits = m.decoder(feat, None, None, None, train_mode=False)
        g.check([feat._base if feat._base is not None else feat, logits], require_guarded=True)
    idx, _ = m.label_convertor.tensor2idx(logits, CC.img_metas(img.shape[0]))
    return feat.cpu(), logits.cpu(), idx


@pytest.mark.parametrize("name", list(KEYS))
def test_module_bf16x3_in_vgg_and_decoder_against_the_golden(cuda, models, name):
    G = BC.golden()
    fk, lk, ik = KEYS[name]
    m = models[name]
    img, _ = BC.vgg_input(name, G)
    _, exact, _ = vgg_and_decoder(m, cuda, img)
    try:
        m.set_compute_dtype("bf16x3", decoder="bf16x3")
        assert m.backbone.compute_dtype == "bf16x3" and m.decoder.lstm_dtype == "bf16x3"
        _, logits, idx = vgg_and_decoder(m, cuda, img)
    finally:
        m.set_compute_dtype(None, decoder=None)
    e = np.abs(logits.numpy() - G[lk]).max()
    print(f"{name} bf16x3 in VGG and decoder: logits max abs error {e:.3e} (bar 1e-4)")
    assert e <= 1e-4
    assert idx == ragged(G[ik])
    assert m.label_convertor.idx2str(idx) == m.label_convertor.idx2str(ragged(G[ik]))
    assert (bits(logits) != bits(exact)).any(), "the switch was ignored: every logit has the bits of the exact fp32 path"


@pytest.mark.parametrize("name", list(KEYS))
def test_module_decoder_bf16_on_exact_features(cuda, models, name):
    G = BC.golden()
    fk, lk, ik = KEYS[name]
    m = models[name]
    img, _ = BC.vgg_input(name, G)
    try:
        m.set_compute_dtype(None, decoder=torch.bfloat16)
        assert m.backbone.compute_dtype is None and m.decoder.lstm_dtype == torch.bfloat16
        _, logits, idx = vgg_and_decoder(m, cuda, img)
    finally:
        m.set_compute_dtype(None, decoder=None)
    routes, golden = DC.golden_decoder(name)
    r_err = DC.rel(routes[torch.bfloat16], golden)
    e = DC.rel(logits, golden)
    print(f"{name} decoder bf16 on the exact VGG: logits against the golden {e:.3e}, bar {2 * r_err:.3e} "
          f"(2 x the restatement's error {r_err:.3e}); max abs {np.abs(logits.numpy() - G[lk]).max():.3e}")
    assert idx == ragged(G[ik])
    assert m.label_convertor.idx2str(idx) == m.label_convertor.idx2str(ragged(G[ik]))
    assert e <= 2 * r_err


@pytest.mark.parametrize("name", list(KEYS))
def test_module_bf16_in_vgg_and_decoder(cuda, models, name):
    G = BC.golden()
    fk, lk, ik = KEYS[name]
    m = models[name]
    img, _ = BC.vgg_input(name, G)
    golden = torch.from_numpy(G[lk]).double()
    host = BC.build_model(name)
    with torch.no_grad():
        restated = DC.decoder64(host.decoder, BC.vgg64(host.backbone, img, False).float(), torch.bfloat16)
    r_err = DC.rel(restated, golden)
    try:
        m.set_compute_dtype(torch.bfloat16, decoder=torch.bfloat16)
        _, logits, idx = vgg_and_decoder(m, cuda, img)
    finally:
        m.set_compute_dtype(None, decoder=None)
    e = DC.rel(logits, golden)
    strings, want = m.label_convertor.idx2str(idx), m.label_convertor.idx2str(ragged(G[ik]))
    print(f"{name} bf16 in VGG and decoder: logits against the golden {e:.3e}, bar {2 * r_err:.3e} (2 x the error of vgg64(bf16) "
          f"followed by the decoder restatement, {r_err:.3e}); strings {strings} against the golden {want} (compared, not "
          f"asserted: {'equal' if strings == want else 'DIFFERENT'})")
    assert e <= 2 * r_err


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_module_contract(cuda, models, mode):
    dec = models["crnn_tps"].decoder
    full = DC.rnd((5, 512, 1, 27), 55).relu()
    with torch.no_grad(), GA.guarded(cuda) as g:
        feat = g.input(full)[:, :, :, :26]                          # the sliced view conv6 hands over
        before = dec._forward_hip(feat)                             # mode None: the route the parent commit takes
        try:
            dec.set_compute_dtype(mode)
            five = dec(feat, None, None, None, train_mode=False)
            alone = dec(g.input(full[3:4])[:, :, :, :26], None, None, None, train_mode=False)
            dense = dec(g.input(full[:, :, :, :26]), None, None, None, train_mode=False)
            empty = dec(torch.zeros((0, 512, 1, 26), device=cuda), None, None, None, train_mode=False)
            twice = dec(feat, None, None, None, train_mode=False)
        finally:
            dec.set_compute_dtype(None)
        after = dec._forward_hip(feat)
        g.check([before, five, alone, dense, twice, after], require_guarded=True)
    assert tuple(five.shape) == (5, 26, 37) and five.dtype == torch.float32
    assert tuple(empty.shape) == (0, 26, 37) and empty.dtype == torch.float32
    assert torch.equal(bits(alone[0]), bits(five[3])), "image 3 alone against image 3 of 5"
    assert torch.equal(bits(dense), bits(five)), "a contiguous map against the sliced view of the same values"
    assert torch.equal(bits(twice), bits(five)), "the same call twice"
    assert torch.equal(bits(after), bits(before)), "the default path moved after a mode round trip"
    assert (bits(five) != bits(before)).any(), "the switch was ignored"
    assert {"lstm", "lstm_bf16x3" if mode == "bf16x3" else "lstm_bf16"} <= set(dec.decoder[0].__dict__["_tpspp_prepared"])
