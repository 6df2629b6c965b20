"""-m gpu: the CRNN recogniser's kernels (include/tpspp_crnn.h) and modules (tps_pp_amd/crnn.py).

Every kernel output is allocated through tests/guarded_alloc.py: nothing is written outside it and every element of it is
written.  Comparisons against float64 use the project's bar, restated unchanged in tests/test_gpu_train_primitives.py
(`rel`, `within_bar`): relative L2 error <= max(1e-5, 2 x the error of PyTorch's fp32 composition of the same operation on
the GPU against the same float64); every error is printed with its bar.  The LSTM's fp32 composition is the cell written
out with F.linear (`cell`), the float64 reference `nn.LSTM(...).double()` on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import guarded_alloc as GA
import tps_pp_amd
from test_gpu_train_primitives import rel, within_bar
from tps_pp_amd import build_detector, ops
from tps_pp_amd.crnn import VeryDeepVgg

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import crnn_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

H = ops.CRNN_HIDDEN
GROUPS = ops.CRNN_LSTM_GROUPS


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


# ---- pool --------------------------------------------------------------------------------------------------------------
RECT = ((2, 2), (2, 1), (0, 1))
POOL_CASES = [((2, 3, 8, 25), RECT), ((1, 5, 4, 26), RECT), ((3, 2, 5, 7), RECT), ((1, 1, 2, 1), RECT),
              ((2, 3, 7, 9), ((2, 2), (2, 2), (0, 0)))]


def pool_inputs(shape, geo):
    """Negative maps (a zero-padded pool would show), -inf, and a NaN in each window position and next to each padded
    column: one map per variant, stacked along the batch."""
    (kh, kw), (sh, sw), (ph, pw) = geo
    N, C, Hh, W = shape
    base = -0.5 - rnd(shape, 11).abs()
    out = [base, torch.full(shape, float("-inf")), torch.where(rnd(shape, 12) > 0.5, torch.tensor(float("-inf")), base)]
    spots = {(y, x) for y in range(min(kh, Hh)) for x in range(min(kw, W))}                 # each window position
    spots |= {(y, x) for y in (0, Hh - 1) for x in (0, W - 1)}                              # next to the padded columns
    spots |= {(Hh // 2, W // 2), (Hh - 1, W // 2)}
    for (y, x) in sorted(spots):
        t = base.clone()
        t[:, :, y, x] = float("nan")
        out.append(t)
    return torch.cat(out, 0)


@pytest.mark.parametrize("shape,geo", POOL_CASES)
def test_maxpool_equals_torch_bit_for_bit(cuda, shape, geo):
    x = pool_inputs(shape, geo)
    want = F.max_pool2d(x, *geo)
    with GA.guarded(cuda) as g:
        got = ops.crnn_maxpool(g.input(x), *geo)
        assert g.check(got, require_guarded=True) == 1
    assert got.shape == want.shape and torch.isnan(want).any() and torch.isinf(want).any()
    assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {want.numel()} differ"
    if geo[1] == (2, 2):
        assert torch.equal(bits(ops.maxpool2x2(x.to(cuda))), bits(want))


# ---- LSTM ----------------------------------------------------------------------------------------------------------------
def cell(xg, w_hh):
    """The recurrence written out, in xg's dtype on xg's device: xg (T, N, 2, 4H), w_hh (2, 4H, H) -> (T, N, 2H)."""
    T, N = xg.shape[:2]
    out = xg.new_zeros((T, N, 2 * H))
    for d in range(2):
        h, c = xg.new_zeros((N, H)), xg.new_zeros((N, H))
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            i, f, gg, o = (xg[t, :, d] + F.linear(h, w_hh[d])).chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[t, :, d * H:(d + 1) * H] = h
    return out


@pytest.fixture(scope="module")
def lstms():
    """{input width: (nn.LSTM fp32, its float64 copy, (w_ih (8H, K), bias (8H), w_hh (2, 4H, H)) fp32)} with weights twice
    PyTorch's initial scale, so that the gates leave their linear range."""
    out = {}
    for K in (512, 256):
        torch.manual_seed(K)
        m = nn.LSTM(K, H, bidirectional=True)
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(2.0)
        m64 = nn.LSTM(K, H, bidirectional=True).double()
        m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
        w = (torch.cat([m.weight_ih_l0, m.weight_ih_l0_reverse]).detach(),
             torch.cat([m.bias_ih_l0 + m.bias_hh_l0, m.bias_ih_l0_reverse + m.bias_hh_l0_reverse]).detach(),
             torch.stack([m.weight_hh_l0, m.weight_hh_l0_reverse]).detach())
        out[K] = (m, m64, w)
    return out


def lstm_case(cuda, lstms, K, T, N, group, bad, label):
    m, m64, (w_ih, b, w_hh) = lstms[K]
    x = rnd((T, N, K), 1000 * T + N)
    with torch.no_grad():
        want = m64(x.double())[0]
        xg32 = (F.linear(x.to(cuda), w_ih.to(cuda), b.to(cuda))).view(T, N, 2, 4 * H)
        lib32 = cell(xg32, w_hh.to(cuda))
        # the cell restated in float64 is nn.LSTM's: the float64 references of the exact-property tests rest on it
        ref64 = cell(F.linear(x.double(), w_ih.double(), b.double()).view(T, N, 2, 4 * H), w_hh.double())
        assert (ref64 - want).abs().max() < 1e-12
    with GA.guarded(cuda) as g:
        xd, wd = g.input(x), g.input(w_hh)
        xg = ops.linear_fwd(xd, (T, N, N * K, K, 1), w_ih.to(cuda), b.to(cuda)).view(T, N, 2, 4 * H)
        got = ops.crnn_lstm(xg, wd, group)
        g.check([xg, got], require_guarded=True)
    assert tuple(got.shape) == (T, N, 2 * H)
    within_bar(label, got, lib32, want, bad)
    for n in range(N):
        within_bar(f"{label} image {n}", got[:, n], lib32[:, n], want[:, n], bad)
    return got


@pytest.mark.parametrize("K", (512, 256))
@pytest.mark.parametrize("T", (1, 2, 9, 26, 33))
def test_lstm_against_float64_over_T(cuda, lstms, K, T):
    bad = {}
    lstm_case(cuda, lstms, K, T, 3, 0, bad, f"lstm K={K} T={T} N=3")
    assert not bad, bad


@pytest.mark.parametrize("g", GROUPS)
def test_lstm_against_float64_over_group_edges(cuda, lstms, g):
    bad = {}
    for N in (1, g - 1, g + 1, 2 * g + 3):
        lstm_case(cuda, lstms, 256, 3, N, g, bad, f"lstm K=256 T=3 N={N} g={g}")
    lstm_case(cuda, lstms, 512, 3, 2 * g + 3, g, bad, f"lstm K=512 T=3 N={2 * g + 3} g={g}")
    assert not bad, bad


@pytest.fixture(scope="module")
def xg_batch(lstms):
    """A batch that spans three blocks of the largest group: xg (3, 35, 2, 4H) and w_hh."""
    return rnd((3, 2 * max(GROUPS) + 3, 2, 4 * H), 77, 2.0), lstms[256][2][2]


def run_lstm(cuda, xg, w_hh, group=0):
    with GA.guarded(cuda) as g:
        out = ops.crnn_lstm(g.input(xg), g.input(w_hh), group)
        g.check(out, require_guarded=True)
    return out.cpu()


def test_lstm_zero_input_gives_zero_output_bit_for_bit(cuda, xg_batch):
    xg, w_hh = xg_batch
    for g in (0,) + GROUPS:
        out = run_lstm(cuda, torch.zeros_like(xg), w_hh, g)
        assert not bits(out).any(), f"g={g}: {int((bits(out) != 0).sum())} words are not +0.0"


def test_lstm_image_is_independent_of_batch_position_and_group(cuda, xg_batch):
    xg, w_hh = xg_batch
    N = xg.shape[1]
    alone = torch.cat([run_lstm(cuda, xg[:, n:n + 1].contiguous(), w_hh, 0) for n in range(N)], 1)
    for g in (0,) + GROUPS:
        out = run_lstm(cuda, xg, w_hh, g)
        ne = (bits(out) != bits(alone)).flatten(2).any(2).any(0)
        assert not ne.any(), f"g={g}: images {ne.nonzero().flatten().tolist()} differ from their N = 1 run"
    for n in (0, 17, N - 1):                                       # ... and alone under every group size, and mid-batch
        for g in GROUPS:
            assert torch.equal(bits(run_lstm(cuda, xg[:, n:n + 1].contiguous(), w_hh, g)), bits(alone[:, n:n + 1])), (n, g)
        sub = run_lstm(cuda, xg[:, n:n + 2].contiguous() if n + 2 <= N else xg[:, n - 1:n + 1].contiguous(), w_hh, 4)
        assert torch.equal(bits(sub[:, 0 if n + 2 <= N else 1]), bits(alone[:, n]))


def test_lstm_directions_run_the_right_way(cuda, xg_batch):
    xg, w_hh = xg_batch
    T, N = 5, 6
    xg = rnd((T, N, 2, 4 * H), 78, 2.0)
    t0, n0 = 2, 4
    base = run_lstm(cuda, xg, w_hh)
    pert = xg.clone()
    pert[t0, n0] += 0.5
    out = run_lstm(cuda, pert, w_hh)
    same = bits(out) == bits(base)
    others = [n for n in range(N) if n != n0]
    assert same[:, others].all(), "another image changed"
    fwd, rev = same[:, n0, :H], same[:, n0, H:]
    assert fwd[:t0].all() and not fwd[t0:].all(1).any(), "forward half: identical before t0, changed from t0 on"
    assert rev[t0 + 1:].all() and not rev[:t0 + 1].all(1).any(), "reverse half: identical after t0, changed up to t0"


def test_lstm_saturated_gates_stay_finite_and_within_the_bar(cuda, xg_batch):
    _, w_hh = xg_batch
    xg = rnd((4, 5, 2, 4 * H), 79, 400.0)                         # most pre-activations beyond +-100
    assert (xg.abs() > 100).float().mean() > 0.7
    want = cell(xg.double(), w_hh.double())
    lib32 = cell(xg.to(cuda), w_hh.to(cuda))
    got = run_lstm(cuda, xg, w_hh)
    assert torch.isfinite(got).all()
    bad = {}
    within_bar("lstm saturated", got, lib32, want, bad)
    huge = run_lstm(cuda, torch.where(xg > 0, torch.tensor(3.0e38), torch.tensor(-3.0e38)), w_hh)
    assert torch.isfinite(huge).all() and huge.abs().max() <= 1.0
    assert not bad, bad


# ---- conv6 -----------------------------------------------------------------------------------------------------------------
def test_conv6_route_against_float64(cuda):
    torch.manual_seed(6)
    vgg = VeryDeepVgg(leaky_relu=False, input_channels=1).eval()
    bn = vgg.cnn.batchnorm6
    with torch.no_grad():
        bn.running_mean.copy_(rnd((512,), 61, 0.1))
        bn.running_var.copy_(1 + rnd((512,), 62, 0.25))
        bn.weight.copy_(1 + rnd((512,), 63, 0.25))
        bn.bias.copy_(rnd((512,), 64, 0.1))
    x = rnd((2, 512, 2, 27), 65).relu()
    tail = nn.Sequential(vgg.cnn.conv6, bn, nn.ReLU())
    with torch.no_grad():
        want = tail.double()(x.double())
        tail.float()
        lib32 = tail.to(cuda)(x.to(cuda))
        with GA.guarded(cuda) as g:
            got = VeryDeepVgg.conv6(g.input(x), vgg._hip_weights()[6])
            g.check(got._base if got._base is not None else got, require_guarded=True)
    assert tuple(got.shape) == tuple(want.shape) == (2, 512, 1, 26)
    bad = {}
    within_bar("conv6 (2,512,2,27)", got, lib32, want, bad)
    assert not bad, bad


# ---- CTC decode ------------------------------------------------------------------------------------------------------------
T_DEC = 8
NAMED = [  # (arg-max per position over classes {0 = blank, 1}, decode_len, kept positions)
    ([1, 1, 1, 1, 1, 1, 1, 1], 8, [0]),                    # a run collapses
    ([1, 1, 0, 1, 0, 0, 1, 1], 8, [0, 3, 6]),              # a a blank a
    ([0, 1, 1, 0, 1, 0, 0, 0], 8, [1, 4]),                 # a leading blank
    ([0, 0, 0, 0, 0, 0, 0, 0], 8, []),                     # all blank
    ([1, 1, 1, 1, 0, 1, 0, 1], 2, [0]),                    # decode_len cuts a run in the middle
    ([0, 0, 1, 1, 1, 0, 1, 1], 3, [2]),
    ([1, 0, 1, 0, 1, 0, 1, 0], 1, [0]),                    # decode_len 1
    ([0, 1, 0, 1, 0, 1, 0, 1], 8, [1, 3, 5, 7]),           # decode_len T
    ([1, 0, 1, 0, 1, 0, 1, 0], 0, []),                     # valid_ratio 0
]


def decode_case(N, C, T, seed):
    """Integer-valued logits with one maximum per position: rows 0.. hold NAMED (T = 8), the rest random runs."""
    g = torch.Generator().manual_seed(seed)
    am = torch.randint(0, C, (N, T), generator=g)
    am = torch.where(torch.rand((N, T), generator=g) < 0.5, am.roll(1, 1), am)           # runs
    am = torch.where(torch.rand((N, T), generator=g) < 0.3, torch.zeros_like(am), am)    # blanks
    lens = torch.randint(1, T + 1, (N,), generator=g)
    if T == T_DEC:
        for r, (seq, ln, _) in enumerate(NAMED[:N]):
            am[r], lens[r] = torch.tensor(seq), ln
    logits = torch.randint(-4, 1, (N, T, C), generator=g).float()
    logits.scatter_(2, am[:, :, None], 3.0)
    return logits, am, lens


@pytest.mark.parametrize("C", (2, 37, 92))
@pytest.mark.parametrize("N", (1, 65, 130))
def test_ctc_decode_equals_the_host_path(cuda, N, C):
    conv = tps_pp_amd.CTCConvertor(dict_type="DICT36", with_unknown=False)
    bad = {}
    for T in (T_DEC, 1, 26):
        logits, am, lens = decode_case(N, C, T, 100 * N + C + T)
        metas = [dict(valid_ratio=max(0.0, (int(ln) - 0.5) / T)) for ln in lens]
        assert conv._decode_lens(metas, T) == lens.tolist()
        wi, ws = conv._scan(logits, metas)                                     # the host path (test_crnn_host.py pins it)
        if T == T_DEC:
            for r, (_, _, kept) in enumerate(NAMED[:N]):
                assert np.flatnonzero(wi[r] >= 0).tolist() == kept
        with GA.guarded(cuda) as g:
            idx, score = ops.crnn_ctc_decode_device(g.input(logits), g.input(lens.to(torch.int32)), conv.blank_idx)
            g.check([idx, score], require_guarded=True)
        assert np.array_equal(idx.cpu().numpy(), wi), f"N={N} C={C} T={T}"
        hi, hs = conv._scan(logits.to(cuda), metas)                            # the convertor's own GPU path: one copy
        assert np.array_equal(hi, wi) and np.array_equal(hs, score.cpu().numpy())
        keep = torch.from_numpy(wi >= 0)
        want = torch.where(keep, F.softmax(logits.double(), 2).max(2).values, torch.zeros((), dtype=torch.float64))
        lib32 = torch.where(keep.to(cuda), F.softmax(logits.to(cuda), 2).max(2).values, torch.zeros((), device=cuda))
        if keep.any():
            within_bar(f"ctc score N={N} C={C} T={T}", score, lib32, want, bad)
        err = (score.cpu().double() - want).abs().max().item()
        print(f"ctc score N={N} C={C} T={T}: max abs error {err:.3e}, floor 1e-6")
        assert err <= 1e-6 and not (score.cpu()[~keep] != 0).any()
    assert not bad, bad


def test_ctc_decode_tie_takes_the_lowest_index(cuda):
    logits = torch.full((2, 3, 5), -1.0)
    logits[0, :, 3] = logits[0, :, 1] = 2.0                                      # classes 1 and 3 tie: 1 wins, the run collapses
    logits[1, 0, 4] = logits[1, 0, 0] = 2.0                                      # blank ties with 4: blank wins
    logits[1, 1, 4] = logits[1, 1, 2] = 2.0
    logits[1, 2, :] = 0.0                                                        # all equal: class 0
    idx, score = ops.crnn_ctc_decode(logits.to(cuda), [3, 3], 0)
    assert idx.tolist() == [[1, -1, -1], [-1, 2, -1]]
    want = 1.0 / (2 + 3 * np.exp(-3.0))
    assert abs(score[0, 0] - want) <= 1e-6 and abs(score[1, 1] - want) <= 1e-6 and score[0, 1] == 0


# ---- module ----------------------------------------------------------------------------------------------------------------
def build_model(name, cuda):
    m = build_detector(CC.models()[name]).eval()
    sd = CC.state(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.to(cuda)


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "crnn_tps.npz"))


def ragged(idx, score):
    return [r[r >= 0].tolist() for r in idx], [s[r >= 0].tolist() for r, s in zip(idx, score)]


def test_crnn_tps_module_against_the_reference(cuda, G):
    m = build_model("crnn_tps", cuda)
    assert isinstance(m, tps_pp_amd.CRNNNet)
    img = torch.from_numpy(CC.images()).to(cuda)
    with torch.no_grad():
        rect = m.preprocessor(img)
        feat = m.backbone(rect)
        logits = m.decoder(feat, None, None, None, train_mode=False)
    e_rect = np.abs(rect.cpu().numpy() - G["rect"]).max()
    e_feat, e_logits = np.abs(feat.cpu().numpy() - G["feat"]).max(), np.abs(logits.cpu().numpy() - G["logits"]).max()
    print(f"crnn_tps: max abs error rectified {e_rect:.3e}, feat {e_feat:.3e}, logits {e_logits:.3e} (bar 1e-4)")
    assert tuple(feat.shape) == (CC.N, 512, 1, 26) and tuple(logits.shape) == (CC.N, 26, 37)
    assert e_rect <= 1e-4                                           # the classic module's bar (tests/test_gpu_modules.py)
    assert e_feat <= 1e-4 and e_logits <= 1e-4
    conv = m.label_convertor
    for ratios, ki, ks in ((CC.VALID_RATIOS, "idx", "score"), (None, "idx_full", "score_full")):
        idx, score = conv.tensor2idx(logits, CC.img_metas(CC.N, ratios))
        wi, ws = ragged(G[ki], G[ks])
        assert idx == wi
        assert all(np.abs(np.array(a) - np.array(b)).max(initial=0) <= 1e-4 for a, b in zip(score, ws))
    idxk, scorek = conv.tensor2idx(logits, CC.img_metas(CC.N, CC.VALID_RATIOS), topk=CC.TOPK, return_topk=True)
    for n in range(CC.N):
        keep = G["idx_topk"][n, :, 0] >= 0
        assert idxk[n] == G["idx_topk"][n][keep].tolist()
        assert np.abs(np.array(scorek[n]).reshape(-1, CC.TOPK) - G["score_topk"][n][keep]).max(initial=0) <= 1e-4
    # forward(..., return_loss=False): the list of dicts, valid ratios from resize_shape as simple_test computes them
    metas = [dict(resize_shape=(32, int(round(r * CC.HW[1])), 1)) for r in CC.VALID_RATIOS]
    res = m(img, metas, return_loss=False)
    wi, ws = ragged(G["idx"], G["score"])
    assert isinstance(res, list) and [set(r) for r in res] == [{"text", "score"}] * CC.N
    assert [r["text"] for r in res] == conv.idx2str(wi)
    assert all(np.abs(np.array(r["score"]) - np.array(s)).max(initial=0) <= 1e-4 for r, s in zip(res, ws))


def test_crnn_module_without_a_preprocessor_at_width_32(cuda, G):
    m = build_model("crnn", cuda)
    img = torch.from_numpy(CC.images32()).to(cuda)
    with torch.no_grad():
        feat = m.backbone(img)
        logits = m.decoder(feat, None, None, None, train_mode=False)
    e_feat, e_logits = np.abs(feat.cpu().numpy() - G["feat32"]).max(), np.abs(logits.cpu().numpy() - G["logits32"]).max()
    print(f"crnn width 32: max abs error feat {e_feat:.3e}, logits {e_logits:.3e} (bar 1e-4)")
    assert tuple(logits.shape) == (CC.N32, 9, 37) and e_feat <= 1e-4 and e_logits <= 1e-4
    res = m.simple_test(img, [dict(resize_shape=(32, 32, 1)) for _ in range(CC.N32)])
    wi, ws = ragged(G["idx32"], G["score32"])
    assert [r["text"] for r in res] == m.label_convertor.idx2str(wi)
    assert all(np.abs(np.array(r["score"]) - np.array(s)).max(initial=0) <= 1e-4 for r, s in zip(res, ws))


def test_one_training_step_decreases_the_loss(cuda):
    """A smoke test of the wiring: `.train()` is the PyTorch composition behind the HIP warp forward and backward."""
    m = build_model("crnn_tps", cuda).train()
    img = torch.from_numpy(CC.images()).to(cuda)
    metas = [dict(resize_shape=(32, 100, 1), text=s) for s in CC.TEXTS]
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    loss0 = m(img, metas, return_loss=True)["loss_ctc"]
    assert loss0.grad_fn is not None
    opt.zero_grad()
    loss0.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    opt.step()
    loss1 = m(img, metas, return_loss=True)["loss_ctc"]
    print(f"loss_ctc {loss0.item():.4f} -> {loss1.item():.4f}")
    assert loss1.item() < loss0.item()
