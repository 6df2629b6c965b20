"""-m gpu: the NRTR decoder's training graph and its loss on HIP kernels (include/tpspp_train_dec.h) -- attention with a
per-key mask, a causal mask and separate row strides (tpspp_attn_train.hip), the target embedding and the sequence
cross-entropy (tpspp_dec_train.hip), the decoder layers composed around them (ops.decoder_layer_autograd) and the public
switches (NRTRDecoder.set_train_backend, _SequenceLoss.set_train_backend, EncodeDecodeRecognizer.set_train_backend).

Bar (tests/test_gpu_attn_train.py::within_bar, restated here): the relative L2 error of every result against a float64
composition on the CPU is <= max(1e-5, 2 x the error of PyTorch's fp32 composition on the GPU against the same float64).
At kernel level the float64 composition is the attention of `nrtr_head._mha_graph` with the (N, Lq, Lk) mask and the
materialised dropout mask; at module level `NRTRDecoder._forward_train_graph` and `losses.sequence_cross_entropy`.  The
embedding gradient is compared exactly, on integer-valued data.

The case tables at the top are plain data: tests/test_dec_train_host.py checks on the CPU that they hold what they claim."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import guarded_alloc as GA
from freeze_patterns import check_freeze_patterns
from tps_pp_amd import NRTRDecoder, TFDecoderLayer, TFEncoderLayer, losses, ops

pytestmark = pytest.mark.gpu


def rel(got, want):
    want = want.detach().cpu().double()
    n = want.norm()
    d = (got.detach().cpu().double() - want).norm()
    return (d / n).item() if n > 0 else d.item()


def within_bar(label, got, lib32, want, bad):
    """Collects (error, bar) of `got` in `bad` if it misses max(1e-5, 2 x the error of the fp32 composition `lib32`)."""
    assert got is not None, f"{label}: missing"
    assert torch.isfinite(got).all(), f"{label}: not finite"
    bar = max(1e-5, 2 * rel(lib32, want))
    e = rel(got, want)
    print(f"{label}: rel L2 {e:.3e}, bar {bar:.3e}")
    if e > bar:
        bad[label] = (e, bar)


# ---- case tables ---------------------------------------------------------------------------------------------------------
def _keys(T, masked):
    m = torch.ones(T, dtype=torch.bool)
    m[list(masked)] = False
    return m


def self_case(name, heads, T, masked_per_image, empty_rows=None):
    """Causal self-attention on T tokens; image b has the keys `masked_per_image[b]` masked.  empty_rows: {image: the
    queries that see no key at all} -- every other query of the case sees at least one."""
    return dict(name=name, heads=heads, Tq=T, Tk=T, causal=True, valid_len=None,
                key_mask=torch.stack([_keys(T, m) for m in masked_per_image]), empty_rows=empty_rows or {})


# per T: no mask, a pad suffix, pads in the middle (T = 1 leaves room for no mask)
SELF_CASES = [
    self_case("T1", 1, 1, [[], []]),
    self_case("T8", 2, 8, [[], range(5, 8), range(2, 4)]),
    self_case("T40", 1, 40, [[], range(17, 40), range(9, 21)]),
    self_case("T64", 2, 64, [[], range(63, 64), range(1, 63)]),
    self_case("T65", 1, 65, [[], range(64, 65), range(30, 64)]),
    # image 1: keys 64..127 masked, key 128 visible -- queries >= 128 see block 0, nothing in block 1, block 2 (the skipped
    # running-maximum update); queries 64..127 walk block 1 and see nothing in it
    self_case("T130", 2, 130, [[], range(64, 128), range(100, 130)]),
    # image 1: key 0 (and 1) masked: queries 0 and 1 see no key at all
    self_case("T40-key0", 2, 40, [[], [0, 1], range(30, 40)], {1: [0, 1]}),
    self_case("T130-key0", 1, 130, [range(0, 70), []], {0: list(range(70))}),
]


def cross_case(Tq, Tk):
    """Cross-attention: ragged valid_len with a length of 1 and a length inside the last block of 64 keys."""
    vl = [Tk, 1, max(1, Tk - 3)]
    return dict(name=f"{Tq}x{Tk}", heads=1 if Tk == 256 else 2, Tq=Tq, Tk=Tk, causal=False, valid_len=vl, key_mask=None,
                empty_rows={})


CROSS_CASES = [cross_case(*s) for s in ((1, 20), (8, 20), (3, 1), (40, 64), (40, 65), (65, 256))]
ATTN_CASES = {c["name"]: c for c in SELF_CASES + CROSS_CASES}


def visible(case):
    """(N, Tq, Tk) bool: which key each query of the case sees."""
    Tq, Tk = case["Tq"], case["Tk"]
    N = len(case["valid_len"]) if case["valid_len"] is not None else case["key_mask"].shape[0]
    vis = torch.ones((N, Tq, Tk), dtype=torch.bool)
    if case["valid_len"] is not None:
        vis &= (torch.arange(Tk)[None, :] < torch.tensor(case["valid_len"])[:, None])[:, None, :]
    if case["key_mask"] is not None:
        vis &= case["key_mask"][:, None, :]
    if case["causal"]:
        vis &= torch.tril(torch.ones((Tq, Tk), dtype=torch.bool))[None]
    return vis


def ce_case(name, K, L, shift, ignored, N=3, big=False):
    """Cross-entropy of (N, L, K) logits; `ignored`: {image: positions of the TARGETS (N, L) set to the ignore index}
    ("all" = every position).  Every case has a scored position except "all-ignored"."""
    return dict(name=name, K=K, L=L, shift=shift, N=N, ignored=ignored, big=big)


CE_IGNORE = 1000
CE_CASES = [
    ce_case("K1", 1, 2, False, {}),
    ce_case("K1-shift", 1, 2, True, {1: [1]}),
    ce_case("K5-L8", 5, 8, False, {0: [7], 2: [0, 3]}),
    ce_case("K5-L8-shift", 5, 8, True, {0: [7], 2: [1, 3]}),
    ce_case("K92-L40", 92, 40, False, {0: range(20, 40), 1: "all"}),
    ce_case("K92-L40-shift", 92, 40, True, {0: range(20, 40), 1: "all"}),             # image 1: all targets ignored
    ce_case("K1024-L2", 1024, 2, False, {2: [1]}),
    ce_case("K1024-L8-shift", 1024, 8, True, {1: range(4, 8)}),
    ce_case("K92-big", 92, 8, True, {0: [7]}, big=True),                                # logits of +-80
    ce_case("all-ignored", 5, 8, True, {0: "all", 1: "all"}, N=2),
]
CE_BY_NAME = {c["name"]: c for c in CE_CASES}


def ce_inputs(case):
    g = torch.Generator().manual_seed(7 + case["K"] * 100 + case["L"])
    N, L, K = case["N"], case["L"], case["K"]
    logits = torch.randn((N, L, K), generator=g) * 2
    if case["big"]:
        sel = torch.rand((N, L, K), generator=g)
        logits = torch.where(sel < 0.1, torch.full_like(logits, 80.0), torch.where(sel > 0.9, torch.full_like(logits, -80.0),
                                                                                  logits))
    targets = torch.randint(0, K, (N, L), generator=g)
    for b, pos in case["ignored"].items():
        targets[b, list(range(L)) if pos == "all" else list(pos)] = CE_IGNORE
    return logits, targets


def ce_scored(case):
    """Number of scored positions of the case."""
    _, t = ce_inputs(case)
    t = t[:, 1:] if case["shift"] else t
    return int((t != CE_IGNORE).sum())


# ---- attention: float64 reference and the HIP run ------------------------------------------------------------------------
def attention_ref(q, k, v, heads, vis, keep=None, p=0.0):
    """The attention of `_mha_graph` under the (N, Tq, Tk) mask `vis` -> (out (N, Tq, C), lse (N, heads, Tq)).  A query
    that sees no key is defined as include/tpspp_train_dec.h defines it: out 0, lse -inf, no gradient."""
    n, tq, c = q.shape
    tk = k.shape[1]
    vis = vis.to(q.device)
    empty = ~vis.any(-1)                                                   # (N, Tq)
    qh = q.reshape(n, tq, heads, 64).transpose(1, 2)
    kh = k.reshape(n, tk, heads, 64).transpose(1, 2)
    vh = v.reshape(n, tk, heads, 64).transpose(1, 2)
    att = torch.matmul(qh / (64 ** 0.5), kh.transpose(2, 3))
    att = att.masked_fill(~(vis | empty[:, :, None])[:, None], float("-inf"))
    lse = torch.logsumexp(att, dim=-1).masked_fill(empty[:, None, :], float("-inf"))
    att = F.softmax(att, dim=-1) * (~empty)[:, None, :, None].to(q.dtype)
    if keep is not None:
        att = att * keep.to(device=q.device, dtype=q.dtype) / (1.0 - p)
    return torch.matmul(att, vh).transpose(1, 2).reshape(n, tq, c), lse


def ref_run(ops_, gout, heads, vis, dtype, device, keep=None, p=0.0):
    xs = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in ops_]
    out, lse = attention_ref(*xs, heads, vis, keep, p)
    out.backward(gout.detach().to(device=device, dtype=dtype))
    return [out.detach(), lse.detach()] + [t.grad for t in xs]


def make_case(case, seed=0):
    g = torch.Generator().manual_seed(1000 * case["Tq"] + case["Tk"] + seed)
    N, C = visible(case).shape[0], 64 * case["heads"]
    q, gout = (torch.randn((N, case["Tq"], C), generator=g) for _ in range(2))
    k, v = (torch.randn((N, case["Tk"], C), generator=g) for _ in range(2))
    return q, k, v, gout


NAMES = ("out", "lse", "dq", "dk", "dv")


def hip_run_all(dev, case, q, k, v, gout, p=0.0, seed=0, offset=0, layout="dense", alloc=None):
    """-> ([out, lse, dq, dk, dv], the tensors the two calls allocated or wrote) of tpspp_attn_train_fwd_ex / _bwd_ex.
    layout: "dense"; "fused" -- q, k, v views of one (N, T, 3C) buffer, the gradients views of another; "cross" -- q a view
    with ld_q = C + 32, k / v the halves of a (N*Tk, 2C) buffer, dq written with ld_dq = C + 64 and dk / dv with
    ld_dkv = 2C.  alloc: a guarded_alloc.Guard whose inputs the operands become."""
    N, Tq, C = q.shape
    Tk, heads = k.shape[1], case["heads"]
    put = alloc.input if alloc is not None else (lambda t: t.to(dev))
    vl = None if case["valid_len"] is None else put(torch.tensor(case["valid_len"], dtype=torch.int32))
    km = None if case["key_mask"] is None else put(case["key_mask"].to(torch.uint8))
    if layout == "fused":
        buf = put(torch.cat([q, k, v], dim=2))
        qd, kd, vd, ld_q, ld_kv = buf, buf[..., C:], buf[..., 2 * C:], 3 * C, 3 * C
        grads = torch.empty((N, Tq, 3 * C), device=dev, dtype=torch.float32)
        dq, dk, dv, ld_dq, ld_dkv, produced = grads, grads[..., C:], grads[..., 2 * C:], 3 * C, 3 * C, [grads]
        views = [grads[..., :C], grads[..., C:2 * C], dv]
    elif layout == "cross":
        qb = put(torch.cat([q, torch.zeros((N, Tq, 32))], dim=2))
        kvb = put(torch.cat([k, v], dim=2))
        qd, kd, vd, ld_q, ld_kv = qb, kvb, kvb[..., C:], C + 32, 2 * C
        dqb = torch.empty((N, Tq, C + 64), device=dev, dtype=torch.float32)
        dkvb = torch.empty((N, Tk, 2 * C), device=dev, dtype=torch.float32)
        dqb[..., C:] = 0                                  # the 64 columns beside dq belong to the caller
        dq, dk, dv, ld_dq, ld_dkv, produced = dqb, dkvb, dkvb[..., C:], C + 64, 2 * C, [dqb, dkvb]
        views = [dqb[..., :C], dkvb[..., :C], dv]
    else:
        qd, kd, vd, ld_q, ld_kv = put(q), put(k), put(v), C, C
        dq = torch.empty((N, Tq, C), device=dev, dtype=torch.float32)
        dk, dv = (torch.empty((N, Tk, C), device=dev, dtype=torch.float32) for _ in range(2))
        ld_dq = ld_dkv = C
        produced = views = [dq, dk, dv]
    gd = put(gout)
    out, lse = ops.attn_train_fwd_ex(qd, ld_q, kd, vd, ld_kv, N, C, heads, Tq, Tk, vl, km, case["causal"], p, seed, offset)
    ops.attn_train_bwd_ex(gd, qd, ld_q, kd, vd, ld_kv, out, lse, N, C, heads, Tq, Tk, vl, km, case["causal"], p, seed, offset,
                          dq, ld_dq, dk, dv, ld_dkv)
    return [out.view(N, Tq, C), lse] + views, [out, lse] + produced


def hip_run(*a, **kw):
    return hip_run_all(*a, **kw)[0]


def check_against_float64(cuda, case, p=0.0, seed=0, offset=0, layout="dense"):
    q, k, v, gout = make_case(case)
    N, heads, vis = q.shape[0], case["heads"], visible(case)
    keep = ops.attn_dropout_mask(N, heads, case["Tq"], case["Tk"], p, seed, offset, cuda).cpu() if p > 0 else None
    got = hip_run(cuda, case, q, k, v, gout, p, seed, offset, layout)
    want = ref_run((q, k, v), gout, heads, vis, torch.float64, "cpu", keep, p)
    lib32 = ref_run((q, k, v), gout, heads, vis, torch.float32, cuda, keep, p)
    empty = ~vis.any(-1)                                                   # (N, Tq)
    finite = ~empty[:, None, :].expand_as(want[1])
    assert (got[1].cpu()[~finite] == float("-inf")).all(), "lse of a query that sees no key must be -inf"
    bad = {}
    for name, g, t, w in zip(NAMES, got, lib32, want):
        if name == "lse":
            g, t, w = (x.cpu()[finite] for x in (g, t, w))
        within_bar(f"{case['name']} {layout} p={p} {name}", g, t, w, bad)
    assert not bad, bad
    return got


# ---- 1. causal self-attention --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in SELF_CASES])
def test_causal_self_attention_against_float64(cuda, name):
    case = ATTN_CASES[name]
    dense = check_against_float64(cuda, case)
    fused = check_against_float64(cuda, case, layout="fused")
    ok, why = GA.same_bits(dense, fused)
    assert ok, f"views of one (N, T, 3C) buffer and dense operands must give the same bits: {why}"
    out, lse, dq, dk, dv = dense
    for b, rows in case["empty_rows"].items():
        assert (out[b, rows] == 0).all() and (dq[b, rows] == 0).all() and (lse[b, :, rows] == float("-inf")).all(), b
    # a masked key, and a key no query sees, has exact zero gradients
    unseen = ~visible(case).any(1)
    assert (dk.cpu()[unseen] == 0).all() and (dv.cpu()[unseen] == 0).all()


def test_empty_rows_add_nothing_to_dk_and_dv(cuda):
    """The rows of an image that see no key contribute nothing: changing their q and d_out changes no other result."""
    case = ATTN_CASES["T40-key0"]
    q, k, v, gout = make_case(case)
    first = hip_run(cuda, case, q, k, v, gout)
    q2, g2 = q.clone(), gout.clone()
    for b, rows in case["empty_rows"].items():
        q2[b, rows] = 5.0 - q[b, rows]
        g2[b, rows] = 100.0 + gout[b, rows]
    ok, why = GA.same_bits(first, hip_run(cuda, case, q2, k, v, g2))
    assert ok, why


# ---- 2. cross-attention --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in CROSS_CASES])
def test_cross_attention_against_float64(cuda, name):
    case = ATTN_CASES[name]
    dense = check_against_float64(cuda, case)
    cross = check_against_float64(cuda, case, layout="cross")
    ok, why = GA.same_bits(dense, cross)
    assert ok, f"strided and dense operands must give the same bits: {why}"


def test_autograd_wrapper_takes_the_strided_operands_without_copies(cuda):
    case = ATTN_CASES["40x65"]
    q, k, v, gout = make_case(case)
    C = q.shape[2]
    want = hip_run(cuda, case, q, k, v, gout, 0.1, 5, 3)
    qb = q.to(cuda).requires_grad_(True)
    kvb = torch.cat([k, v], dim=2).to(cuda).requires_grad_(True)
    vl = torch.tensor(case["valid_len"], dtype=torch.int32, device=cuda)
    assert ops._attn_operands("t", qb, kvb[..., :C], kvb[..., C:])[3:] == (C, 2 * C)
    out = ops.attn_train_autograd_ex(qb, kvb[..., :C], kvb[..., C:], vl, None, False, 0.1, 5, 3)
    out.backward(gout.to(cuda))
    ok, why = GA.same_bits([want[0], want[2], want[3], want[4]], [out.detach(), qb.grad, kvb.grad[..., :C], kvb.grad[..., C:]])
    assert ok, why


# ---- 3. masked keys ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T40", "T130", "40x65"])
def test_masked_keys_get_exact_zeros_and_are_never_used(cuda, name):
    case = ATTN_CASES[name]
    q, k, v, gout = make_case(case)
    unseen = ~visible(case).any(1)                                         # (N, Tk)
    assert unseen.any()
    for p in (0.0, 0.5):
        out, lse, dq, dk, dv = hip_run(cuda, case, q, k, v, gout, p, 3, 0)
        assert (dk.cpu()[unseen] == 0).all() and (dv.cpu()[unseen] == 0).all(), p
        assert dv.cpu()[~unseen].abs().max() > 0
        k2, v2 = k.clone(), v.clone()
        k2[unseen] = 7.0 - 3.0 * k[unseen]
        v2[unseen] = 1e3 + v[unseen]
        ok, why = GA.same_bits([out, lse, dq, dk, dv], hip_run(cuda, case, q, k2, v2, gout, p, 3, 0))
        assert ok, why


# ---- 4. dropout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["T65", "T130", "40x65"])
def test_dropout_matches_the_materialised_mask(cuda, name, p):
    check_against_float64(cuda, ATTN_CASES[name], p=p, seed=1234567890123, offset=3)


def test_zero_rate_is_the_no_dropout_arithmetic_bit_for_bit(cuda):
    for name in ("T65", "40x65"):
        case = ATTN_CASES[name]
        ts = make_case(case)
        plain = hip_run(cuda, case, *ts)
        ok, why = GA.same_bits(plain, hip_run(cuda, case, *ts, 0.0, 987654321, 11))
        assert ok, why
        assert not GA.same_bits(plain[0], hip_run(cuda, case, *ts, 0.5, 987654321, 11)[0])[0]


# ---- 5. the encoder's entry points are the same kernels -------------------------------------------------------------------
@pytest.mark.parametrize("name,p", [("8x20", 0.0), ("40x65", 0.5)])
def test_without_the_new_masks_the_bits_are_those_of_attn_train_fwd_and_bwd(cuda, name, p):
    case = dict(ATTN_CASES[name], Tq=ATTN_CASES[name]["Tk"])               # the old entry points' tests use Tq == Tk
    q, k, v, gout = make_case(case)
    N, T, C = q.shape
    new = hip_run(cuda, case, q, k, v, gout, p, 11, 2)
    qd, kd, vd, gd = (t.to(cuda) for t in (q, k, v, gout))
    vl = torch.tensor(case["valid_len"], dtype=torch.int32, device=cuda)
    out, lse = ops.attn_train_fwd(qd, kd, vd, C, N, C, case["heads"], T, T, vl, p, 11, 2)
    dq, dk, dv = (torch.empty_like(qd) for _ in range(3))
    ops.attn_train_bwd(gd, qd, kd, vd, C, out, lse, N, C, case["heads"], T, T, vl, p, 11, 2, dq, dk, dv, C)
    ok, why = GA.same_bits(new, [out.view(N, T, C), lse, dq, dk, dv])
    assert ok, why


# ---- 6. embedding --------------------------------------------------------------------------------------------------------
EMBED_CASES = [(1, 5, 64), (7, 93, 128), (320, 5, 128), (2051, 93, 64)]


def embed_inputs(M, classes, C, kind="random"):
    g = torch.Generator().manual_seed(M + classes)
    pad = classes - 1
    tok = torch.randint(0, classes, (M,), generator=g)
    if classes > 3:
        tok[tok == 1] = 2                                                  # class 1 is never used
    if kind == "one":
        tok[:] = 2
    elif kind == "pad":
        tok[:] = pad
    dx = torch.randint(-4, 5, (M, C), generator=g).float()
    weight = torch.randn((classes, C), generator=g)
    return tok, dx, weight, pad


@pytest.mark.parametrize("M,classes,C", EMBED_CASES, ids=[f"M{c[0]}" for c in EMBED_CASES])
@pytest.mark.parametrize("kind", ["random", "one", "pad"])
def test_embedding_forward_and_gradient_are_exact(cuda, M, classes, C, kind):
    tok, dx, weight, pad = embed_inputs(M, classes, C, kind)
    L = 7 if M % 7 == 0 else 1
    N = M // L
    pos = torch.randn((1, L + 3, C), generator=torch.Generator().manual_seed(1))
    w = weight.to(cuda).requires_grad_(True)
    out = ops.embed_pos_autograd(tok.view(N, L), w, pos.to(cuda), pad)
    want = weight[tok].view(N, L, C).to(cuda) + pos.to(cuda)[0, :L]
    ok, why = GA.same_bits(out.detach(), want)
    assert ok, why
    out.backward(dx.view(N, L, C).to(cuda))
    ref = torch.zeros((classes, C), dtype=torch.float64).index_add_(0, tok, dx.double())
    ref[pad] = 0
    assert torch.equal(w.grad.cpu().double(), ref), "integer-valued sums are exact in any order"
    assert (w.grad[pad] == 0).all()
    if classes > 3:
        assert (w.grad[1] == 0).all(), "a class no token names"
    assert kind == "pad" or w.grad.abs().max() > 0


def test_embedding_ignores_tokens_out_of_range_on_the_device_and_refuses_them_on_the_host(cuda):
    tok, dx, weight, pad = embed_inputs(320, 5, 64)
    bad = tok.clone()
    bad[[3, 100]] = torch.tensor([5, -1])
    with pytest.raises(ValueError, match=r"tokens must lie in \[0, 5\)"):
        ops.embed_pos_autograd(bad.view(1, -1), weight.to(cuda), torch.zeros(320, 64, device=cuda), pad)
    dw = ops.embed_bwd(dx.to(cuda), bad.to(cuda).int(), 5, pad)
    keep = torch.ones(320, dtype=torch.bool)
    keep[[3, 100]] = False
    ref = torch.zeros((5, 64), dtype=torch.float64).index_add_(0, tok[keep], dx[keep].double())
    ref[pad] = 0
    assert torch.equal(dw.cpu().double(), ref)
    out = ops.embed_pos_fwd(bad.to(cuda).int().view(1, -1), weight.to(cuda), torch.ones(320, 64, device=cuda))
    assert (out[0, [3, 100]] == 1).all()


# ---- 7. cross-entropy ----------------------------------------------------------------------------------------------------
def ce_run(case, reduction, flatten, dtype, device, hip=False, view=False):
    logits, targets = ce_inputs(case)
    x = logits.to(device=device, dtype=dtype).requires_grad_(True)
    if hip and view:              # the caller shifts: the strided view logits[:, :-1] against targets[:, 1:], shift off
        loss = ops.seq_cross_entropy_autograd(x[:, :-1], targets[:, 1:], CE_IGNORE, reduction, False, flatten)
    elif hip:
        loss = ops.seq_cross_entropy_autograd(x, targets, CE_IGNORE, reduction, case["shift"], flatten)
    else:
        loss = losses.sequence_cross_entropy(x, targets, CE_IGNORE, reduction, case["shift"], flatten)
    g = torch.randn(loss.shape, generator=torch.Generator().manual_seed(3)).to(device=device, dtype=dtype)
    loss.backward(g)
    return loss.detach(), x.grad


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("name", [c["name"] for c in CE_CASES if c["name"] != "all-ignored"])
def test_cross_entropy_against_float64(cuda, name, reduction):
    case = CE_BY_NAME[name]
    for flatten in ((True, False) if reduction == "none" else (True,)):
        want = ce_run(case, reduction, flatten, torch.float64, "cpu")
        lib32 = ce_run(case, reduction, flatten, torch.float32, cuda)
        runs = [("", ce_run(case, reduction, flatten, torch.float32, cuda, hip=True))]
        if case["shift"]:
            runs.append((" view", ce_run(case, reduction, flatten, torch.float32, cuda, hip=True, view=True)))
        bad = {}
        for tag, got in runs:
            assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (got[0].shape, want[0].shape)
            within_bar(f"{name} {reduction}{tag} loss", got[0], lib32[0], want[0], bad)
            within_bar(f"{name} {reduction}{tag} d_logits", got[1], lib32[1], want[1], bad)
            assert (got[1][want[1].to(cuda) == 0] == 0).all() or case["K"] == 1, "ignored positions: exact zeros"
        assert not bad, bad
        if case["shift"]:
            ok, why = GA.same_bits(runs[0][1], runs[1][1])
            assert ok, f"the view logits[:, :-1] and shift = 1 are the same computation: {why}"


def test_cross_entropy_ignored_positions_and_the_dropped_one_get_exact_zero_gradients(cuda):
    case = CE_BY_NAME["K92-L40-shift"]
    _, targets = ce_inputs(case)
    for reduction in ("none", "mean", "sum"):
        _, d = ce_run(case, reduction, True, torch.float32, cuda, hip=True)
        ignored = torch.ones((case["N"], case["L"]), dtype=torch.bool)
        ignored[:, :-1] = targets[:, 1:] == CE_IGNORE
        assert (d.cpu()[ignored] == 0).all() and (d[1] == 0).all() and (d.cpu()[~ignored].abs().amax(-1) > 0).all()


def test_mean_over_no_scored_position_is_nan_as_in_pytorch(cuda):
    case = CE_BY_NAME["all-ignored"]
    want, _ = ce_run(case, "mean", True, torch.float32, cuda)
    got, d = ce_run(case, "mean", True, torch.float32, cuda, hip=True)
    assert torch.isnan(want) and torch.isnan(got) and (d == 0).all()
    got, d = ce_run(case, "sum", True, torch.float32, cuda, hip=True)
    assert got.item() == 0 and (d == 0).all()


# ---- 8. determinism ------------------------------------------------------------------------------------------------------
def all_six(cuda):
    res = []
    for name, p in (("T130", 0.1), ("65x256", 0.5)):
        case = ATTN_CASES[name]
        res += hip_run(cuda, case, *make_case(case), p, 77, 2)
    tok, dx, weight, pad = embed_inputs(2051, 93, 64)
    res.append(ops.embed_pos_fwd(tok.to(cuda).int().view(7, 293), weight.to(cuda), torch.ones(293, 64, device=cuda)))
    res.append(ops.embed_bwd(dx.to(cuda), tok.to(cuda).int(), 93, pad))
    for red in ("mean", "none"):
        res += list(ce_run(CE_BY_NAME["K92-L40-shift"], red, True, torch.float32, cuda, hip=True))
    return res


def test_bitwise_reproducible_across_calls_and_streams(cuda):
    first, second = all_six(cuda), all_six(cuda)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        third = all_six(cuda)
    side.synchronize()
    for other in (second, third):
        ok, why = GA.same_bits(first, other)
        assert ok, why


# ---- 9. guard bands and poison -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", [("T65", "fused"), ("T130", "dense"), ("T40-key0", "dense"), ("40x65", "cross"),
                                         ("65x256", "cross"), ("3x1", "dense")])
def test_guard_bands_and_poison_attention(cuda, name, layout):
    case = ATTN_CASES[name]
    ts = make_case(case)
    with GA.guarded(cuda) as g:
        for p in (0.0, 0.5):
            res, produced = hip_run_all(cuda, case, *ts, p, 9, 1, layout, alloc=g)
            g.check(produced, require_guarded=True)
            assert all(torch.isfinite(t).all() for t in res[:1] + res[2:])
        assert not g.fallthrough, g.fallthrough


def test_guard_bands_and_poison_embedding_and_cross_entropy(cuda):
    with GA.guarded(cuda) as g:
        for M, classes, C in EMBED_CASES:
            tok, dx, weight, pad = embed_inputs(M, classes, C)
            tk = g.input(tok.int().view(1, M))
            out = ops.embed_pos_fwd(tk, g.input(weight), g.input(torch.ones(M, C)))
            dw = ops.embed_bwd(g.input(dx), tk, classes, pad)
            g.check([out, dw], require_guarded=True)
        for case in CE_CASES:
            logits, targets = ce_inputs(case)
            x, t = g.input(logits), g.input(targets.int())
            for red in (0, 1, 2):
                loss, lse, r, c = ops.seq_ce_fwd(x, t, case["shift"], CE_IGNORE, red)
                gr = g.input(torch.ones(loss.shape if red == 0 else (1,)))
                d = ops.seq_ce_bwd(gr, x, t, lse, c, case["shift"], CE_IGNORE, red)
                g.check([loss, lse, d] + ([r, c] if red else []), require_guarded=True)
        assert not g.fallthrough, g.fallthrough


# ---- 10. decoder module --------------------------------------------------------------------------------------------------
def small_decoder(dropout=0.0):
    cfg = cases.HD_SMALL
    m = NRTRDecoder(d_embedding=cfg["d_model"], num_classes=cases.NUM_CLASSES, start_idx=cases.START_IDX,
                    padding_idx=cases.PAD_IDX, max_seq_len=cases.HD_MAXLEN, dropout=dropout, **cfg)
    sd = cases.synth_state(m.state_dict(), 10, cases.head_state_rule, cases.HD_KEEP)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


def wide_decoder(dropout=0.0):
    torch.manual_seed(6)
    return NRTRDecoder(n_layers=1, d_model=512, d_inner=256, dropout=dropout, num_classes=cases.NUM_CLASSES,
                       start_idx=cases.START_IDX, padding_idx=cases.PAD_IDX, max_seq_len=40)


DECODERS = {"small": small_decoder, "wide": wide_decoder}


def targets_of(N, L, lengths, seed=2):
    """(N, L) padded targets: <SOS>, `lengths[b]` characters, <EOS>, then padding."""
    g = torch.Generator().manual_seed(seed)
    t = torch.full((N, L), cases.PAD_IDX, dtype=torch.long)
    for b, n in enumerate(lengths):
        row = [cases.START_IDX] + torch.randint(0, 90, (n,), generator=g).tolist() + [cases.END_IDX]
        t[b, :min(L, len(row))] = torch.tensor(row[:L])
    return t


def decoder_inputs(name):
    g = torch.Generator().manual_seed(22)
    if name == "small":
        N, T, C, L = cases.HD_N, cases.HD_HW[0] * cases.HD_HW[1], cases.HD_SMALL["d_model"], cases.HD_MAXLEN
        ratios, lengths = cases.HD_RATIOS, [6, 3, 0]                       # pad suffixes of 0, 3 and 6 positions
    else:
        N, T, C, L = 2, 64, 512, 40
        ratios, lengths = [1.0, 0.4], [38, 11]
    out_enc = torch.randn((N, T, C), generator=g)
    gout = torch.randn((N, L, cases.NUM_CLASSES - 1), generator=g)
    return out_enc, targets_of(N, L, lengths), gout, [dict(valid_ratio=r) for r in ratios]


def decoder_grads(m, out_enc, targets, gout, metas, dtype, device, backend="torch"):
    m = copy.deepcopy(m).to(device).to(dtype).train().set_train_backend(backend)
    x = out_enc.detach().to(device=device, dtype=dtype).requires_grad_(True)
    if backend == "hip":
        out = m(None, x, {"padded_targets": targets}, metas, train_mode=True)
    else:
        out = m._forward_train_graph(x, targets.to(device), metas)
    out.backward(gout.to(device=device, dtype=dtype))
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["out_enc"] = x.grad
    grads["logits"] = out.detach()
    return grads


@pytest.mark.parametrize("name", ["small", "wide"])
def test_decoder_gradients_against_float64(cuda, name):
    m = DECODERS[name]()
    out_enc, targets, gout, metas = decoder_inputs(name)
    got = decoder_grads(m, out_enc, targets, gout, metas, torch.float32, cuda, "hip")
    want = decoder_grads(m, out_enc, targets, gout, metas, torch.float64, "cpu")
    lib32 = decoder_grads(m, out_enc, targets, gout, metas, torch.float32, cuda)
    assert set(got) == set(want) and got["logits"].shape == gout.shape
    bad = {}
    for k in want:
        assert want[k] is not None and want[k].norm() > 0, k
        within_bar(f"{name} {k}", got[k], lib32[k], want[k], bad)
    assert not bad, bad
    assert (got["trg_word_emb.weight"][cases.PAD_IDX] == 0).all()


def decoder_loss(m, loss, out_enc, targets, metas):
    return loss(m(None, out_enc, {"padded_targets": targets}, metas, train_mode=True), {"padded_targets": targets})["loss_ce"]


@pytest.mark.parametrize("name", ["small", "wide"])
def test_sgd_steps_track_the_torch_backend(cuda, name):
    out_enc, targets, _, metas = decoder_inputs(name)
    out_enc = out_enc.to(cuda)
    seqs = {}
    for mode in ("torch", "hip"):
        m = DECODERS[name]().to(cuda).train().set_train_backend(mode)
        loss = losses.TFLoss(ignore_index=cases.PAD_IDX, reduction="mean").set_train_backend(mode)
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        seq = []
        for _ in range(3):
            opt.zero_grad()
            val = decoder_loss(m, loss, out_enc, targets, metas)
            val.backward()
            opt.step()
            seq.append(val.item())
        seqs[mode] = seq
    t, h = np.array(seqs["torch"]), np.array(seqs["hip"])
    assert np.all(np.abs(h - t) <= 1e-3 * np.abs(t)), seqs
    assert t[-1] != t[0]


def test_dropout_follows_torch_manual_seed(cuda):
    m = small_decoder(dropout=0.1).to(cuda).train().set_train_backend("hip")
    out_enc, targets, _, metas = decoder_inputs("small")
    out_enc = out_enc.to(cuda)
    outs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        outs.append(m(None, out_enc, {"padded_targets": targets}, metas, train_mode=True).detach())
    assert GA.same_bits(outs[0], outs[1])[0] and not GA.same_bits(outs[0], outs[2])[0]


def test_no_library_layer_runs_in_a_hip_training_step(cuda, monkeypatch):
    m = small_decoder(dropout=0.1).to(cuda).train().set_train_backend("hip")
    loss = losses.TFLoss(ignore_index=cases.PAD_IDX, reduction="mean").set_train_backend("hip")
    out_enc, targets, _, metas = decoder_inputs("small")
    x = out_enc.to(cuda).requires_grad_(True)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the HIP training path")
        return f

    for name in ("linear", "layer_norm", "softmax", "gelu", "embedding", "cross_entropy"):
        monkeypatch.setattr(F, name, refuse(f"F.{name}"))
    for name in ("matmul", "bmm"):
        monkeypatch.setattr(torch, name, refuse(f"torch.{name}"))
    val = decoder_loss(m, loss, x, targets, metas)
    val.backward()
    assert torch.isfinite(val) and x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
    with pytest.raises(AssertionError, match="called on the HIP training path"):
        decoder_loss(m.set_train_backend("torch"), loss, x, targets, metas)


def test_eval_paths_do_not_depend_on_the_train_backend(cuda):
    m = small_decoder().to(cuda).eval()
    out_enc, targets, _, metas = decoder_inputs("small")
    out_enc = out_enc.to(cuda)
    res = {}
    with torch.no_grad():
        for mode in ("torch", "hip"):
            m.set_train_backend(mode)
            res[mode] = [m(None, out_enc, None, metas, train_mode=False),
                         m(None, out_enc, {"padded_targets": targets}, metas, train_mode=True)]
    ok, why = GA.same_bits(res["torch"], res["hip"])
    assert ok, why


# ---- 10b. frozen layers --------------------------------------------------------------------------------------------------
def frozen_blocks(cuda):
    """{name: (Function, call, inputs, {name: Parameter}, the last Linear, further patterns)} on d_model 128 (2 heads),
    N = 3, T = 20 encoder tokens, L = 9 target positions, attention dropout 0.1: the attention block of an encoder layer
    (with q / k / v / fc biases) under valid_len with one short row, and the three blocks of a decoder layer (its
    self-attention under a pad mask with one padded tail)."""
    torch.manual_seed(8)
    enc, dec = TFEncoderLayer(128, 64, 2, qkv_bias=True).to(cuda), TFDecoderLayer(128, 64, 2).to(cuda)
    g = torch.Generator().manual_seed(9)
    xt, xl = torch.randn((3, 20, 128), generator=g).to(cuda), torch.randn((3, 9, 128), generator=g).to(cuda)
    out_enc = torch.randn((3, 20, 128), generator=g).to(cuda)
    vl = torch.tensor([20, 7, 20], dtype=torch.int32, device=cuda)
    pad = torch.ones((3, 9), dtype=torch.bool, device=cuda)
    pad[1, 5:] = False

    def named(attn, norm, first="attn"):
        return {**dict(attn.named_parameters(prefix=first)), **dict(norm.named_parameters(prefix="norm"))}

    return {
        "self-valid_len": (ops._AttnBlockFunction, lambda x: ops.attn_block_autograd(x, enc.attn, enc.norm1, vl, 0.1, 3, 1),
                           [xt], named(enc.attn, enc.norm1), "attn.fc.", None),
        "self-causal": (ops._AttnBlockFunction,
                        lambda x: ops.attn_block_autograd(x, dec.self_attn, dec.norm1, None, 0.1, 3, 2, key_mask=pad,
                                                          causal=True),
                        [xl], named(dec.self_attn, dec.norm1), "attn.fc.", None),
        "cross": (ops._CrossAttnBlockFunction,
                  lambda x, e: ops.cross_attn_block_autograd(x, e, dec.enc_attn, dec.norm2, vl, 0.1, 3, 3),
                  [xl, out_enc], named(dec.enc_attn, dec.norm2), "attn.fc.",
                  {"out_enc frozen": {"input0"} | set(named(dec.enc_attn, dec.norm2)),
                   "only out_enc trainable": {"input1"}}),
        "ffn": (ops._FfnBlockFunction, lambda x: ops.ffn_block_autograd(x, dec.mlp, dec.norm3), [xl],
                named(dec.mlp, dec.norm3, "mlp"), "mlp.w_2.", None),
    }


@pytest.mark.parametrize("name", ["self-valid_len", "self-causal", "cross", "ffn"])
def test_freeze_patterns_return_none_and_keep_the_bits(cuda, name, monkeypatch):
    fn_cls, call, inputs, params, last, more = frozen_blocks(cuda)[name]
    check_freeze_patterns(monkeypatch, fn_cls, call, inputs, params, last, more)


# ---- 11. recogniser ------------------------------------------------------------------------------------------------------
def test_nrtr_forward_train_with_every_stage_on_hip(cuda):
    import tps_pp_amd as P
    torch.manual_seed(0)
    m = P.build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                         strides=[2, 1, 2, 1, 2]),
                              tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                              decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                              label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
                              max_seq_len=8))
    m = m.to(cuda).train().set_train_backend("hip_all", backbone="hip", encoder="hip", decoder="hip", loss="hip")
    assert (m.decoder.train_backend, m.loss.train_backend) == ("hip", "hip") and m.decoder.dropout_p == 0.1
    img = torch.randn((2, 3, 32, 128), device=cuda)
    metas = [dict(resize_shape=(32, 128, 3), text="ab"), dict(resize_shape=(32, 100, 3), text="tps")]
    opt = torch.optim.SGD(m.parameters(), lr=0.02)
    seq = []
    for step in range(3):
        opt.zero_grad()
        val = sum(v.mean() for v in m.forward_train(img, metas).values())
        assert torch.isfinite(val)
        val.backward()
        if step == 0:
            for k, p in m.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all(), k
        opt.step()
        seq.append(val.item())
    print("losses", seq)
    assert seq[2] < seq[0], seq
