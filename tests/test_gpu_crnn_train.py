"""-m gpu: the HIP training paths of the CRNN decoder and the CTC loss (include/tpspp_crnn_train.h, tps_pp_amd/crnn.py,
tps_pp_amd/losses.py).

Every entry point runs inside tests/guarded_alloc.py: inputs, outputs, saved tensors and workspaces lie between guard bands
and are poisoned, so nothing is written outside them and every element is written.  Comparisons against float64 use the
project's bar unchanged (`rel`, `within_bar` of tests/test_gpu_train_primitives.py): relative L2 error <= max(1e-5, 2 x the
error of PyTorch's fp32 composition of the same operation on the GPU against the same float64); every error is printed
with its bar.  The LSTM's fp32 composition is the cell written out with F.linear (`cell_full`) under autograd, its float64
reference `nn.LSTM(...).double()` on the CPU; the CTC loss's are `F.ctc_loss(log_softmax(.))` in fp32 on the GPU and in
float64 on the CPU."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import crnn_train_cases as TC
import guarded_alloc as GA
import tps_pp_amd
from test_gpu_train_primitives import rel, within_bar
from tps_pp_amd import build_detector, ops
from tps_pp_amd.losses import CTCLoss

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import crnn_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

H = ops.CRNN_HIDDEN
GROUPS = ops.CRNN_LSTM_GROUPS
LSTM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
              "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


# ---- LSTM ----------------------------------------------------------------------------------------------------------------
def cell_full(xg, w_hh):
    """`cell()` of tests/test_gpu_crnn.py restated without in-place writes, so that autograd runs through it, and returning
    what the training forward keeps: xg (T, N, 2, 4H), w_hh (2, 4H, H) -> (out (T, N, 2H), gates (T, N, 2, 4H) after their
    activations, cell states (T, N, 2, H))."""
    T, N = xg.shape[:2]
    hs, gs, cs = [[None] * T, [None] * T], [[None] * T, [None] * T], [[None] * T, [None] * T]
    for d in range(2):
        h, c = xg.new_zeros((N, H)), xg.new_zeros((N, H))
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            i, f, gg, o = (xg[t, :, d] + F.linear(h, w_hh[d])).chunk(4, dim=1)
            i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
            c = f * c + i * gg
            h = o * torch.tanh(c)
            hs[d][t], gs[d][t], cs[d][t] = h, torch.cat([i, f, gg, o], 1), c
    return (torch.stack([torch.cat([hs[0][t], hs[1][t]], 1) for t in range(T)]),
            torch.stack([torch.stack([gs[0][t], gs[1][t]], 1) for t in range(T)]),
            torch.stack([torch.stack([cs[0][t], cs[1][t]], 1) for t in range(T)]))


@pytest.fixture(scope="module")
def lstms():
    """{input width: (nn.LSTM fp32, its float64 copy)} with weights twice PyTorch's initial scale (`lstms()` of
    tests/test_gpu_crnn.py), so that the gates leave their linear range."""
    out = {}
    for K in (512, 256):
        torch.manual_seed(K)
        m = nn.LSTM(K, H, bidirectional=True)
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(2.0)
        m64 = nn.LSTM(K, H, bidirectional=True).double()
        m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
        out[K] = (m, m64)
    return out


def packed(p):
    """{name: tensor} of an nn.LSTM -> (w_ih (8H, K), b_ih + b_hh (8H), w_hh (2, 4H, H))."""
    return (torch.cat([p["weight_ih_l0"], p["weight_ih_l0_reverse"]]),
            torch.cat([p["bias_ih_l0"] + p["bias_hh_l0"], p["bias_ih_l0_reverse"] + p["bias_hh_l0_reverse"]]),
            torch.stack([p["weight_hh_l0"], p["weight_hh_l0_reverse"]]))


def lstm_train_case(cuda, lstms, K, T, N, group, bad, label):
    """Forward and backward of one layer through the entry points, under guards, against float64."""
    m, m64 = lstms[K]
    x, d_out = rnd((T, N, K), 1000 * T + N), rnd((T, N, 2 * H), 2000 * T + N)
    # float64 on the CPU
    m64.zero_grad()
    x64 = x.double().requires_grad_(True)
    out64 = m64(x64)[0]
    out64.backward(d_out.double())
    want = {n: getattr(m64, n).grad.clone() for n in LSTM_NAMES}
    with torch.no_grad():
        w64 = packed({n: getattr(m64, n) for n in LSTM_NAMES})
        ref = cell_full(F.linear(x.double(), w64[0], w64[1]).view(T, N, 2, 4 * H), w64[2])
        assert (ref[0] - out64).abs().max() < 1e-12               # the restated cell is nn.LSTM's
    # PyTorch's fp32 composition on the GPU
    p32 = {n: getattr(m, n).detach().to(cuda).requires_grad_(True) for n in LSTM_NAMES}
    x32 = x.to(cuda).requires_grad_(True)
    w32 = packed(p32)
    lib = cell_full(F.linear(x32, w32[0], w32[1]).view(T, N, 2, 4 * H), w32[2])
    lib[0].backward(d_out.to(cuda))
    # the kernels
    w_ih, b, w_hh = (t.detach() for t in packed({n: getattr(m, n) for n in LSTM_NAMES}))
    with GA.guarded(cuda) as g:
        xd, wd, dd = g.input(x), g.input(w_hh), g.input(d_out)
        wt = g.input(w_hh.transpose(1, 2).contiguous())
        desc = (T, N, N * K, K, 1)
        xg = ops.linear_fwd(xd, desc, w_ih.to(cuda), b.to(cuda)).view(T, N, 2, 4 * H)
        out, gates, cell = ops.crnn_lstm_train_fwd(xg, wd, group)
        plain = ops.crnn_lstm(xg, wd, group)
        d_xg, d_dir = ops.crnn_lstm_bwd(dd, gates, cell, wt, group, direction_major=True)
        dw_ih, db = ops.linear_bwd_weight(d_xg.view(T * N, 8 * H), xd, desc, 8 * H, K)
        dx = ops.linear_bwd_data(d_xg.view(T * N, 8 * H), w_ih.to(cuda)).view(T, N, K)
        dw_hh = ops.crnn_lstm_bwd_w_hh(d_dir, out)
        g.check([xg, out, gates, cell, plain, d_xg, d_dir, dw_ih, db, dx], require_guarded=True)
        g.check(GA.Unguarded(dw_hh, "stacked by torch.stack from two guarded tpspp_linear_bwd_weight results"))
    assert torch.equal(bits(out), bits(plain)), f"{label}: the training forward's out differs from tpspp_crnn_lstm_fwd's"
    assert torch.equal(bits(d_dir), bits(d_xg.permute(2, 0, 1, 3))), f"{label}: the direction-major copy differs"
    within_bar(f"{label} gates", gates, lib[1], ref[1], bad)
    within_bar(f"{label} cell", cell, lib[2], ref[2], bad)
    within_bar(f"{label} dx", dx, x32.grad, x64.grad, bad)
    for n in range(N):
        within_bar(f"{label} dx image {n}", dx[:, n], x32.grad[:, n], x64.grad[:, n], bad)
    got = {"weight_ih_l0": dw_ih[:4 * H], "weight_ih_l0_reverse": dw_ih[4 * H:], "weight_hh_l0": dw_hh[0],
           "weight_hh_l0_reverse": dw_hh[1], "bias_ih_l0": db[:4 * H], "bias_hh_l0": db[:4 * H],
           "bias_ih_l0_reverse": db[4 * H:], "bias_hh_l0_reverse": db[4 * H:]}
    for n in LSTM_NAMES:
        within_bar(f"{label} d {n}", got[n], p32[n].grad, want[n], bad)
    if T == 1:
        assert not bits(dw_hh).any(), "T = 1: no step has a previous h, d w_hh is +0"


@pytest.mark.parametrize("K", (512, 256))
@pytest.mark.parametrize("T", (1, 2, 9, 26, 33))
def test_lstm_training_against_float64_over_T(cuda, lstms, K, T):
    bad = {}
    lstm_train_case(cuda, lstms, K, T, 3, 0, bad, f"lstm train K={K} T={T} N=3")
    assert not bad, bad


@pytest.mark.parametrize("g", GROUPS)
def test_lstm_training_against_float64_over_group_edges(cuda, lstms, g):
    bad = {}
    for N in (1, g - 1, g + 1, 2 * g + 3):
        lstm_train_case(cuda, lstms, 256, 3, N, g, bad, f"lstm train K=256 T=3 N={N} g={g}")
    assert not bad, bad


@pytest.fixture(scope="module")
def xg_batch(lstms):
    """A batch that spans three blocks of the largest group: xg (3, 35, 2, 4H), w_hh, its transpose and d_out."""
    w_hh = torch.stack([lstms[256][0].weight_hh_l0, lstms[256][0].weight_hh_l0_reverse]).detach()
    N = 2 * max(GROUPS) + 3
    return rnd((3, N, 2, 4 * H), 77, 2.0), w_hh, w_hh.transpose(1, 2).contiguous(), rnd((3, N, 2 * H), 177)


def run_lstm(cuda, xg, w_hh, w_hh_t, d_out, group=0):
    with GA.guarded(cuda) as g:
        out, gates, cell = ops.crnn_lstm_train_fwd(g.input(xg), g.input(w_hh), group)
        d_xg, d_dir = ops.crnn_lstm_bwd(g.input(d_out), gates, cell, g.input(w_hh_t), group, direction_major=True)
        g.check([out, gates, cell, d_xg, d_dir], require_guarded=True)
    assert torch.equal(bits(d_dir), bits(d_xg.permute(2, 0, 1, 3)))
    return out.cpu(), d_xg.cpu()


def test_lstm_backward_zero_gradient_gives_zero_bit_for_bit(cuda, xg_batch):
    xg, w_hh, w_hh_t, d_out = xg_batch
    for g in (0,) + GROUPS:
        d_xg = run_lstm(cuda, xg, w_hh, w_hh_t, torch.zeros_like(d_out), g)[1]
        assert not bits(d_xg).any(), f"g={g}: {int((bits(d_xg) != 0).sum())} words are not +0.0"


def test_lstm_backward_image_is_independent_of_batch_position_and_group(cuda, xg_batch):
    xg, w_hh, w_hh_t, d_out = xg_batch
    N = xg.shape[1]

    def part(lo, hi, g):
        """d_xg of the images lo .. hi - 1 run as a batch of their own."""
        return run_lstm(cuda, xg[:, lo:hi].contiguous(), w_hh, w_hh_t, d_out[:, lo:hi].contiguous(), g)[1]

    alone = torch.cat([part(n, n + 1, 0) for n in range(N)], 1)
    assert bits(alone).any()
    for g in (0,) + GROUPS:
        d_xg = run_lstm(cuda, xg, w_hh, w_hh_t, d_out, g)[1]
        ne = (bits(d_xg) != bits(alone)).flatten(2).any(2).any(0)
        assert not ne.any(), f"g={g}: images {ne.nonzero().flatten().tolist()} differ from their N = 1 run"
    for n in (0, 17, N - 1):                                       # ... and alone under every group size, and mid-batch
        for g in GROUPS:
            assert torch.equal(bits(part(n, n + 1, g)), bits(alone[:, n:n + 1])), (n, g)
        lo = n if n + 2 <= N else n - 1
        assert torch.equal(bits(part(lo, lo + 2, 4)[:, n - lo]), bits(alone[:, n]))


def test_lstm_backward_directions_run_the_right_way(cuda, xg_batch):
    _, w_hh, w_hh_t, _ = xg_batch
    T, N, t0 = 5, 6, 2
    xg = rnd((T, N, 2, 4 * H), 78, 2.0)
    d_out = torch.zeros((T, N, 2 * H))
    d_out[t0] = rnd((N, 2 * H), 178)
    d_xg = bits(run_lstm(cuda, xg, w_hh, w_hh_t, d_out)[1])
    assert not d_xg[t0 + 1:, :, 0].any(), "direction 0: steps after t0 carry no gradient"
    assert not d_xg[:t0, :, 1].any(), "direction 1: steps before t0 carry no gradient"
    assert d_xg[:t0 + 1, :, 0].flatten(1).any(1).all() and d_xg[t0:, :, 1].flatten(1).any(1).all()


def test_lstm_backward_saturated_gates_stay_finite_and_within_the_bar(cuda, xg_batch):
    _, w_hh, w_hh_t, _ = xg_batch
    xg, d_out = rnd((4, 5, 2, 4 * H), 79, 2.0) * 50, rnd((4, 5, 2 * H), 179)
    assert (xg.abs() > 20).float().mean() > 0.7
    x64 = xg.double().requires_grad_(True)
    cell_full(x64, w_hh.double())[0].backward(d_out.double())
    x32 = xg.to(cuda).requires_grad_(True)
    cell_full(x32, w_hh.to(cuda))[0].backward(d_out.to(cuda))
    d_xg = run_lstm(cuda, xg, w_hh, w_hh_t, d_out)[1]
    assert torch.isfinite(d_xg).all()
    bad = {}
    within_bar("lstm backward saturated", d_xg, x32.grad, x64.grad, bad)
    assert not bad, bad


def test_bilstm_autograd_is_reproducible_and_equals_its_parts(cuda, lstms):
    T, N, K = 4, 5, 256
    m = copy.deepcopy(lstms[K][0]).to(cuda)
    x, d_out = rnd((T, N, K), 81).to(cuda), rnd((T, N, 2 * H), 82).to(cuda)
    runs = []
    for _ in range(2):
        m.zero_grad()
        xr = x.clone().requires_grad_(True)
        with GA.guarded(cuda) as g:
            out = ops.crnn_bilstm_autograd(xr, (T, N, N * K, K, 1), T, N, m)
            out.backward(d_out)
            grads = [xr.grad] + [getattr(m, n).grad for n in LSTM_NAMES]
            g.check([out, grads])
        runs.append([out.detach().clone()] + [t.clone() for t in grads])
    ok, why = GA.same_bits(runs[0], runs[1])
    assert ok, why
    w_ih, b, w_hh = (t.detach() for t in packed({n: getattr(m, n) for n in LSTM_NAMES}))
    xg = ops.linear_fwd(x, (T, N, N * K, K, 1), w_ih, b).view(T, N, 2, 4 * H)
    out, gates, cell = ops.crnn_lstm_train_fwd(xg, w_hh)
    d_xg, d_dir = ops.crnn_lstm_bwd(d_out, gates, cell, w_hh.transpose(1, 2).contiguous(), direction_major=True)
    assert torch.equal(bits(ops.crnn_lstm_bwd(d_out, gates, cell, w_hh.transpose(1, 2).contiguous())), bits(d_xg))
    dw_ih, db = ops.linear_bwd_weight(d_xg.view(T * N, 8 * H), x, (T, N, N * K, K, 1), 8 * H, K)
    dw_hh = ops.crnn_lstm_bwd_w_hh(d_dir, out)
    parts = [out, ops.linear_bwd_data(d_xg.view(T * N, 8 * H), w_ih).view(T, N, K), dw_ih[:4 * H], dw_hh[0], db[:4 * H],
             db[:4 * H], dw_ih[4 * H:], dw_hh[1], db[4 * H:], db[4 * H:]]
    ok, why = GA.same_bits(runs[0], parts)
    assert ok, why
    assert m.bias_ih_l0.grad.data_ptr() != m.bias_hh_l0.grad.data_ptr()        # equal values in tensors of their own


# ---- CTC loss ------------------------------------------------------------------------------------------------------------
RED = {"none": 0, "mean": 1, "sum": 2}


def run_ctc(cuda, case, reduction="none", zero_infinity=False, grad=None):
    """Forward and backward through the entry points under guards -> (loss (N), reduced | None, d_logits) on the host."""
    logits, padded, tl, il = case
    N = logits.shape[0]
    if grad is None:
        grad = torch.ones((N,)) if reduction == "none" else torch.ones((1,))
    with GA.guarded(cuda) as g:
        lg, tld, ild, gd = g.input(logits), g.input(tl), g.input(il), g.input(grad)
        tg = g.input(padded) if padded.numel() else padded.to(cuda)
        loss, lse, red, ws = ops.crnn_ctc_loss_fwd(lg, tg, tld, ild, TC.BLANK, zero_infinity, RED[reduction])
        d = ops.crnn_ctc_loss_bwd(gd, lg, tg, tld, ild, lse, ws, TC.BLANK, zero_infinity, RED[reduction])
        # (an infeasible image without zero_infinity: its rows of d are not pinned and may hold any NaN)
        g.check([loss, lse, ws] + ([] if red is None else [red]) + ([d] if torch.isfinite(loss).all() else []),
                require_guarded=True)
    return loss.cpu(), None if red is None else red.cpu(), d.cpu()


@pytest.mark.parametrize("name", sorted(TC.CTC_CASES))
def test_ctc_loss_against_float64(cuda, name):
    case = TC.ctc_case(name)
    logits, padded, tl, il = case
    N, T, C = logits.shape
    bad = {}
    past = torch.arange(T)[None, :] >= il[:, None]
    for reduction in ("none", "mean", "sum"):
        grad = rnd((N,), 5).abs() + 0.5 if reduction == "none" else torch.tensor([0.7])
        x64 = logits.double().requires_grad_(True)
        want = TC.ctc_torch(x64, padded, tl, il, reduction)
        want.backward(grad.double().view(want.shape))
        x32 = logits.to(cuda).requires_grad_(True)
        lib = TC.ctc_torch(x32, padded, tl, il, reduction)
        lib.backward(grad.to(cuda).view(lib.shape))
        loss, red, d = run_ctc(cuda, case, reduction, False, grad)
        if reduction == "none":
            within_bar(f"ctc {name} loss per image", loss, lib, want, bad)
        else:
            within_bar(f"ctc {name} loss {reduction}", red.view(()), lib, want, bad)
        within_bar(f"ctc {name} d_logits ({reduction})", d, x32.grad, x64.grad, bad)
        assert not bits(d)[past].any(), f"{name} ({reduction}): rows past the input length are not +0.0"
    assert not bad, bad


def test_ctc_loss_infeasible_image_inside_a_feasible_batch(cuda):
    base = TC.ctc_case("mixed")
    case = TC.ctc_case("mixed", extra=TC.INFEASIBLE)
    others = [0, 2, 3, 4]
    loss0, _, d0 = run_ctc(cuda, base)
    for zero_infinity in (True, False):
        loss, _, d = run_ctc(cuda, case, "none", zero_infinity)
        assert loss[1].item() == (0.0 if zero_infinity else float("inf"))
        assert torch.equal(bits(loss[others]), bits(loss0)) and torch.equal(bits(d[others]), bits(d0))
        if zero_infinity:
            assert not bits(d[1]).any(), "zero_infinity: the infeasible image's gradient block is +0.0"
    # the reductions see the replaced loss: PyTorch's rule, in float64
    logits, padded, tl, il = case
    bad = {}
    for reduction in ("mean", "sum"):
        want = TC.ctc_torch(logits.double(), padded, tl, il, reduction, True)
        lib = TC.ctc_torch(logits.to(cuda), padded, tl, il, reduction, True)
        within_bar(f"ctc zero_infinity {reduction}", run_ctc(cuda, case, reduction, True)[1].view(()), lib, want, bad)
    assert not bad, bad


def test_ctc_loss_image_is_independent_of_its_batch_and_reproducible(cuda):
    case = TC.ctc_case("mixed")
    logits, padded, tl, il = case
    loss, _, d = run_ctc(cuda, case)
    again = run_ctc(cuda, case)
    ok, why = GA.same_bits([loss, d], [again[0], again[2]])
    assert ok, why
    for n in range(logits.shape[0]):
        L = int(tl[n])
        alone = run_ctc(cuda, (logits[n:n + 1], padded[n:n + 1, :L].contiguous(), tl[n:n + 1], il[n:n + 1]))
        assert torch.equal(bits(alone[0]), bits(loss[n:n + 1])) and torch.equal(bits(alone[2]), bits(d[n:n + 1])), n
    for reduction in ("mean", "sum"):
        a, b = run_ctc(cuda, case, reduction), run_ctc(cuda, case, reduction)
        ok, why = GA.same_bits(list(a), list(b))
        assert ok, why


# ---- modules ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "crnn_tps.npz"))


def build_model(name, cuda):
    m = build_detector(CC.models()[name]).eval()
    sd = CC.state(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.to(cuda)


def test_ctc_loss_module_on_the_golden_logits(cuda, G):
    conv = tps_pp_amd.CTCConvertor(dict_type="DICT36", with_unknown=False, lower=True)
    td, metas = conv.str2tensor(CC.TEXTS), CC.img_metas(CC.N)
    logits = torch.from_numpy(G["logits"])
    x64 = logits.double().requires_grad_(True)
    want = CTCLoss()(x64, td, metas)["loss_ctc"]
    want.backward()
    x32 = logits.to(cuda).requires_grad_(True)
    lib = CTCLoss()(x32, td, metas)["loss_ctc"]
    lib.backward()
    xh = logits.to(cuda).requires_grad_(True)
    mod = CTCLoss().set_train_backend("hip")
    with GA.guarded(cuda) as g:
        got = mod(xh, td, metas)["loss_ctc"]
        got.backward()
        g.check([got, xh.grad])
    assert got.shape == want.shape == ()
    bad = {}
    within_bar("golden loss_ctc against float64", got, lib, want, bad)
    within_bar("golden d_logits against float64", xh.grad, x32.grad, x64.grad, bad)
    within_bar("golden loss_ctc against the reference", got, lib, torch.from_numpy(G["loss"]).reshape(()), bad)
    within_bar("golden d_logits against the reference", xh.grad, x32.grad, torch.from_numpy(G["loss_grad"]), bad)
    assert not bad, bad


def decoder_case(cuda, dec, feat, texts, metas, loss_kwargs, label, bad, cut=None):
    """Decoder + loss, "hip" for both, against the float64 CPU composition; lib32 is the "torch" backend on the GPU.
    cut: (lo, hi) -- the modules see feat[..., lo:hi], a non-contiguous view of the leaf."""
    conv = tps_pp_amd.CTCConvertor(dict_type="DICT36", with_unknown=False, lower=True)
    td = conv.str2tensor(texts)
    view = (lambda t: t) if cut is None else (lambda t: t[..., cut[0]:cut[1]])

    def run(d, leaf, loss):
        d.zero_grad()
        logits = d(view(leaf), None, None, None, train_mode=True)
        out = loss(logits, td, metas)["loss_ctc"]
        out.backward()
        return out.detach(), leaf.grad, {k: p.grad for k, p in d.named_parameters()}

    dec64 = copy.deepcopy(dec).cpu().double().train().set_train_backend("torch")
    want = run(dec64, feat.double().requires_grad_(True), CTCLoss(**loss_kwargs))
    dec32 = copy.deepcopy(dec).train().set_train_backend("torch")
    lib = run(dec32, feat.to(cuda).requires_grad_(True), CTCLoss(**loss_kwargs))
    dech = copy.deepcopy(dec).train().set_train_backend("hip")
    with GA.guarded(cuda) as g:
        got = run(dech, feat.to(cuda).requires_grad_(True), CTCLoss(**loss_kwargs).set_train_backend("hip"))
        g.check([got[0], got[1], list(got[2].values())])
    assert len(got[2]) == 20 and torch.isfinite(want[0])
    within_bar(f"{label} loss_ctc", got[0], lib[0], want[0], bad)
    within_bar(f"{label} d_feat", got[1], lib[1], want[1], bad)
    if cut is not None:
        outside = torch.ones(feat.shape[-1], dtype=torch.bool)
        outside[cut[0]:cut[1]] = False
        assert not got[1][..., outside.to(cuda)].any(), "columns outside the view receive no gradient"
    for k in want[2]:
        within_bar(f"{label} d {k}", got[2][k], lib[2][k], want[2][k], bad)


def test_decoder_and_loss_modules_against_float64(cuda, G):
    dec = build_model("crnn_tps", cuda).decoder
    feat = torch.from_numpy(G["feat"])
    bad = {}
    decoder_case(cuda, dec, feat, CC.TEXTS, CC.img_metas(CC.N), {}, "decoder+loss", bad)
    wide = torch.cat([rnd((CC.N, 512, 1, 2), 91), feat, rnd((CC.N, 512, 1, 3), 92)], 3)
    decoder_case(cuda, dec, wide, CC.TEXTS, CC.img_metas(CC.N), {}, "decoder+loss sliced map", bad, cut=(2, 28))
    # input lengths 26, 13, 8: "crnn2016" needs 9 positions, so the third image is infeasible and zero_infinity drops it
    decoder_case(cuda, dec, feat, CC.TEXTS, CC.img_metas(CC.N, CC.VALID_RATIOS), dict(flatten=False, zero_infinity=True),
                 "decoder+loss flatten=False", bad)
    decoder_case(cuda, dec, torch.from_numpy(G["feat32"]), ["ab", "c"], CC.img_metas(CC.N32), {}, "decoder+loss T=9", bad)
    assert not bad, bad


def test_decoder_paths_that_keep_pytorch(cuda, G):
    dec = build_model("crnn_tps", cuda).decoder.train().set_train_backend("hip")
    feat = torch.from_numpy(G["feat"]).to(cuda)
    got = dec(feat, None, None, None, train_mode=True)
    assert got.grad_fn is not None and "LinearNwc" in type(got.grad_fn).__name__
    dec.eval()
    with torch.no_grad():
        ev = dec(feat, None, None, None, train_mode=False)           # the eval fast path is untouched
    assert ev.grad_fn is None and (ev - got.detach()).abs().max() <= 1e-4
    cnn = tps_pp_amd.build_decoder(dict(type="CRNNDecoder", in_channels=512, num_classes=37, rnn_flag=False)).to(cuda)
    out = cnn.train().set_train_backend("hip")(feat, None, None, None, train_mode=True)
    assert "Nwc" not in type(out.grad_fn).__name__ and tuple(out.shape) == (CC.N, 26, 37)      # rnn_flag=False: PyTorch


def test_one_training_step_on_hip_decreases_the_loss(cuda):
    m = build_model("crnn_tps", cuda)
    img = torch.from_numpy(CC.images()).to(cuda)
    metas = [dict(resize_shape=(32, 100, 1), text=s) for s in CC.TEXTS]
    never = build_model("crnn_tps", cuda)
    with torch.no_grad():
        want = never(img, metas, return_loss=False)
        want_logits = never.decoder(never.backbone(never.preprocessor(img)), None, None, None, train_mode=False)
    m.train().set_train_backend("torch", decoder="hip", loss="hip")
    frozen = [b for b in m.modules() if isinstance(b, nn.BatchNorm2d)]
    for b in frozen:                                                # no running statistic moves in this first pass
        b.eval()
    loss = m(img, metas, return_loss=True)["loss_ctc"]
    assert "CtcLoss" in type(loss.grad_fn).__name__
    loss.backward()
    m.eval()
    with torch.no_grad():
        got = m(img, metas, return_loss=False)
        got_logits = m.decoder(m.backbone(m.preprocessor(img)), None, None, None, train_mode=False)
    assert got == want and torch.equal(bits(got_logits), bits(want_logits)), "the eval path changed after a HIP training pass"
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    loss0 = m(img, metas, return_loss=True)["loss_ctc"]
    opt.zero_grad()
    loss0.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    opt.step()
    loss1 = m(img, metas, return_loss=True)["loss_ctc"]
    print(f"loss_ctc {loss0.item():.4f} -> {loss1.item():.4f}")
    assert loss1.item() < loss0.item()
