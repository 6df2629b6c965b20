"""-m gpu: the NRTR encoder's training graph on HIP kernels -- the masked attention with dropout forward and backward
(tpspp_attn_train.hip, include/tpspp_train_attn.h), the encoder layers composed around it (ops.encoder_layer_autograd)
and the public switches (NRTREncoder.set_train_backend, EncodeDecodeRecognizer.set_train_backend(..., encoder=)).

Bar (the project's own, tests/test_gpu_regressor_train.py::check_block): the relative L2 error of every result against a
float64 composition on the CPU is <= max(1e-5, 2 x the error of PyTorch's fp32 composition on the GPU against the same
float64).  At kernel level the float64 composition is the attention of `nrtr_head._mha_graph` (its matmul / masked_fill /
softmax / matmul lines, with the materialised dropout mask in place of F.dropout); at encoder level it is the module's own
`_forward_graph`."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import guarded_alloc as GA
from tps_pp_amd import NRTREncoder, ops

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


# ---- the attention of _mha_graph on projected q / k / v, any dtype and device -------------------------------------------
def attention_ref(q, k, v, heads, valid_len=None, keep=None, p=0.0):
    """-> (out (N, Tq, C), lse (N, heads, Tq)).  keep: the materialised (N, heads, Tq, Tk) dropout mask, or None."""
    n, tq, c = q.shape
    tk = k.shape[1]
    qh = q.reshape(n, tq, heads, 64).transpose(1, 2)
    kh = k.reshape(n, tk, heads, 64).transpose(1, 2)
    vh = v.reshape(n, tk, heads, 64).transpose(1, 2)
    att = torch.matmul(qh / (64 ** 0.5), kh.transpose(2, 3))
    if valid_len is not None:
        vl = torch.as_tensor(valid_len, device=q.device)
        mask = torch.arange(tk, device=q.device)[None, :] < vl[:, None]
        att = att.masked_fill(~mask[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(att, dim=-1)
    att = F.softmax(att, dim=-1)
    if keep is not None:
        att = att * keep.to(device=q.device, dtype=q.dtype) / (1.0 - p)
    return torch.matmul(att, vh).transpose(1, 2).reshape(n, tq, c), lse


def ref_run(q, k, v, gout, heads, valid_len, dtype, device, keep=None, p=0.0):
    xs = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in (q, k, v)]
    out, lse = attention_ref(*xs, heads, valid_len, keep, p)
    out.backward(gout.detach().to(device=device, dtype=dtype))
    return [out.detach(), lse.detach()] + [t.grad for t in xs]


def make_case(N, heads, T, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * N + heads + seed)
    C = 64 * heads
    return [torch.randn((N, T, C), generator=g) for _ in range(4)]          # q, k, v, gout


def hip_run(cuda, q, k, v, gout, valid_len, p=0.0, seed=0, offset=0, fused=False):
    """-> [out, lse, dq, dk, dv] of the HIP kernels; `fused`: q / k / v as views of one (N, T, 3C) buffer."""
    N, T, C = q.shape
    vl = None if valid_len is None else torch.tensor(valid_len, dtype=torch.int32, device=cuda)
    if fused:
        buf = torch.cat([q, k, v], dim=2).to(cuda).requires_grad_(True)
        xs = [buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]]
    else:
        xs = [t.to(cuda).requires_grad_(True) for t in (q, k, v)]
    out = ops.attn_train_autograd(*xs, vl, p, seed, offset)
    out.backward(gout.to(cuda))
    # the log-sum-exp is the forward's second output: the raw entry point returns it
    qd, kd, vd = (t.detach().contiguous() for t in xs)
    out2, lse = ops.attn_train_fwd(qd, kd, vd, C, N, C, C // 64, T, k.shape[1], vl, p, seed, offset)
    assert GA.same_bits(out2.view(N, T, C), out)[0], "views of a fused buffer and dense operands must give the same bits"
    grads = [buf.grad[..., :C], buf.grad[..., C:2 * C], buf.grad[..., 2 * C:]] if fused else [t.grad for t in xs]
    return [out.detach(), lse] + grads


NAMES = ("out", "lse", "dq", "dk", "dv")
SHAPES = [(3, 2, 20, [20, 12, 7]), (2, 1, 1, [1, 1]), (3, 2, 64, [64, 1, 33]), (2, 2, 65, None), (1, 1, 255, [200]),
          (1, 1, 256, None)]


def check_against_float64(cuda, label, N, heads, T, valid_len, p=0.0, seed=0, offset=0, fused=False):
    q, k, v, gout = make_case(N, heads, T)
    keep = ops.attn_dropout_mask(N, heads, T, T, p, seed, offset, cuda).cpu() if p > 0 else None
    got = hip_run(cuda, q, k, v, gout, valid_len, p, seed, offset, fused)
    want = ref_run(q, k, v, gout, heads, valid_len, torch.float64, "cpu", keep, p)
    lib32 = ref_run(q, k, v, gout, heads, valid_len, torch.float32, cuda, keep, p)
    bad = {}
    for name, g, t, w in zip(NAMES, got, lib32, want):
        within_bar(f"{label} {name}", g, t, w, bad)
    assert not bad, bad
    return got


# ---- 1. forward and the three gradients against float64 ------------------------------------------------------------------
@pytest.mark.parametrize("N,heads,T,valid_len", SHAPES, ids=[f"T{s[2]}" for s in SHAPES])
def test_forward_and_gradients_against_float64(cuda, N, heads, T, valid_len):
    check_against_float64(cuda, f"T={T}", N, heads, T, valid_len)


def test_views_of_one_fused_projection_buffer(cuda):
    N, heads, T = cases.HD_N, cases.HD_SMALL["n_head"], cases.HD_HW[0] * cases.HD_HW[1]
    check_against_float64(cuda, "fused", N, heads, T, [20, 12, 7], fused=True)
    check_against_float64(cuda, "fused p=0.1", N, heads, T, [20, 12, 7], p=0.1, seed=5, offset=1, fused=True)


def test_encoder_signature_is_the_general_path_and_reads_strided_operands_in_place(cuda):
    """`attn_train_autograd` is `attn_train_autograd_ex` without the two masks: q as a view of a wider buffer next to k, v
    as the halves of a fused (N, T, 2C) one are read where they lie, and output and gradients have the bits of the dense
    operands and of the raw `tpspp_attn_train_fwd` / `_bwd` entry points.  T = 65 crosses one 64-key block."""
    N, heads, T, p, seed, offset = 2, 2, 65, 0.5, 20240229, 3
    C = 64 * heads
    q, k, v, gout = (t.to(cuda) for t in make_case(N, heads, T, seed=7))
    vl = torch.tensor([65, 40], dtype=torch.int32, device=cuda)
    out, lse = ops.attn_train_fwd(q, k, v, C, N, C, heads, T, T, vl, p, seed, offset)
    raw = [out.view(N, T, C)] + [torch.empty_like(q) for _ in range(3)]
    ops.attn_train_bwd(gout, q, k, v, C, out, lse, N, C, heads, T, T, vl, p, seed, offset, *raw[1:], C)

    xs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = ops.attn_train_autograd(*xs, vl, p, seed, offset)
    out.backward(gout)
    ok, why = GA.same_bits(raw, [out.detach()] + [t.grad for t in xs])
    assert ok, f"dense: {why}"

    qb = torch.full((N, T, C + 32), float("nan"), device=cuda)             # the spare columns are never read
    qb[..., :C] = q
    qb.requires_grad_(True)
    kvb = torch.cat([k, v], dim=2).requires_grad_(True)
    views = (qb[..., :C], kvb[..., :C], kvb[..., C:])
    taken = ops._attn_operands("t", *views)
    assert taken[3:] == (C + 32, 2 * C) and [t.data_ptr() for t in taken[:3]] == [t.data_ptr() for t in views]
    out = ops.attn_train_autograd(*views, vl, p, seed, offset)
    out.backward(gout)
    assert kvb.grad.shape == kvb.shape and qb.grad.shape == qb.shape
    ok, why = GA.same_bits(raw, [out.detach(), qb.grad[..., :C], kvb.grad[..., :C], kvb.grad[..., C:]])
    assert ok, f"strided: {why}"
    assert (qb.grad[..., C:] == 0).all()


# ---- 2. masked keys ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,heads,T,valid_len", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=["T20", "T64", "T255"])
def test_masked_keys_get_exact_zeros_and_are_never_read(cuda, N, heads, T, valid_len):
    q, k, v, gout = make_case(N, heads, T)
    for p in (0.0, 0.5):
        out, lse, dq, dk, dv = hip_run(cuda, q, k, v, gout, valid_len, p, 3, 0)
        for b, n in enumerate(valid_len):
            assert (dk[b, n:] == 0).all() and (dv[b, n:] == 0).all(), (p, b)
            # (a single valid key has P = 1 whatever k is: its dk is zero by the mathematics, only dv is not)
            assert dv[b, :n].abs().max() > 0 and (n == 1 or dk[b, :n].abs().max() > 0), (p, b)
        k2, v2 = k.clone(), v.clone()
        for b, n in enumerate(valid_len):
            k2[b, n:] = 7.0 - 3.0 * k[b, n:]
            v2[b, n:] = 1e3 + v[b, n:]
        again = hip_run(cuda, q, k2, v2, gout, valid_len, p, 3, 0)
        ok, why = GA.same_bits([out, lse, dq], again[:3])
        assert ok, why
        for b, n in enumerate(valid_len):
            assert GA.same_bits([dk[b, :n], dv[b, :n]], [again[3][b, :n], again[4][b, :n]])[0]


# ---- 3. dropout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N,heads,T,valid_len", [SHAPES[0], SHAPES[3]], ids=["T20", "T65"])
def test_dropout_matches_the_materialised_mask(cuda, N, heads, T, valid_len, p):
    check_against_float64(cuda, f"T={T} p={p}", N, heads, T, valid_len, p=p, seed=1234567890123, offset=3)


def test_dropout_mask_is_a_function_of_seed_and_offset_at_the_right_rate(cuda):
    N, heads, T = 8, 2, 80
    n = N * heads * T * T
    assert n >= 10 ** 5
    for p in (0.1, 0.5):
        m = ops.attn_dropout_mask(N, heads, T, T, p, 42, 7, cuda)
        assert m.dtype == torch.uint8 and m.shape == (N, heads, T, T) and int(m.max()) == 1 and int(m.min()) == 0
        assert torch.equal(m, ops.attn_dropout_mask(N, heads, T, T, p, 42, 7, cuda))
        for seed, offset in ((43, 7), (42, 8), (42 + (1 << 32), 7), (42, 7 + (1 << 32))):
            other = ops.attn_dropout_mask(N, heads, T, T, p, seed, offset, cuda)
            frac = (other != m).float().mean().item()
            assert abs(frac - 2 * p * (1 - p)) < 0.02, (seed, offset, frac)      # independent masks differ at rate 2p(1-p)
        kept = m.float().mean().item()
        assert abs(kept - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (p, kept)
        # the decision of an element does not depend on the sizes around it
        sub = ops.attn_dropout_mask(3, 1, 20, 33, p, 42, 7, cuda)
        assert torch.equal(sub, m[:3, :1, :20, :33])
        # no stripes: every row, column, head and image is kept at the rate
        for dims, cnt in (((0, 1, 2), N * heads * T), ((0, 1, 3), N * heads * T), ((1, 2, 3), heads * T * T)):
            r = m.float().mean(dim=dims)
            assert (r - (1 - p)).abs().max().item() <= 6 * math.sqrt(p * (1 - p) / cnt), dims
    assert int(ops.attn_dropout_mask(2, 2, 20, 20, 0.0, 42, 7, cuda).min()) == 1


def test_zero_rate_is_the_no_dropout_arithmetic_bit_for_bit(cuda):
    for N, heads, T, valid_len in (SHAPES[0], SHAPES[3]):
        q, k, v, gout = make_case(N, heads, T)
        plain = hip_run(cuda, q, k, v, gout, valid_len)
        zero = hip_run(cuda, q, k, v, gout, valid_len, 0.0, 987654321, 11)
        ok, why = GA.same_bits(plain, zero)
        assert ok, why
        some = hip_run(cuda, q, k, v, gout, valid_len, 0.5, 987654321, 11)
        assert not GA.same_bits(plain[0], some[0])[0]


# ---- 4. determinism ------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_across_calls_and_streams(cuda):
    for (N, heads, T, valid_len), p in ((SHAPES[0], 0.1), (SHAPES[3], 0.0), (SHAPES[3], 0.5), (SHAPES[4], 0.1)):
        q, k, v, gout = make_case(N, heads, T)
        first = hip_run(cuda, q, k, v, gout, valid_len, p, 77, 2)
        second = hip_run(cuda, q, k, v, gout, valid_len, p, 77, 2)
        side = torch.cuda.Stream(cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            third = hip_run(cuda, q, k, v, gout, valid_len, p, 77, 2)
        side.synchronize()
        for other in (second, third):
            ok, why = GA.same_bits(first, other)
            assert ok, (T, p, why)


# ---- 5. encoder level ----------------------------------------------------------------------------------------------------
def small_encoder(dropout=0.0):
    m = NRTREncoder(dropout=dropout, **cases.HD_SMALL)
    sd = cases.synth_state(m.state_dict(), 9, cases.head_state_rule, cases.HD_KEEP)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


def wide_encoder(dropout=0.0):
    torch.manual_seed(5)
    return NRTREncoder(n_layers=1, d_model=512, d_inner=256, dropout=dropout)


def encoder_inputs(name):
    g = torch.Generator().manual_seed(21)
    if name == "small":
        N, (H, W), C = cases.HD_N, cases.HD_HW, cases.HD_SMALL["d_model"]
        ratios = cases.HD_RATIOS
    else:
        N, (H, W), C = 2, (4, 16), 512
        ratios = [1.0, 0.4]
    feat = torch.randn((N, C, H, W), generator=g)
    gout = torch.randn((N, H * W, C), generator=g)
    return feat, gout, [dict(valid_ratio=r) for r in ratios]


ENCODERS = {"small": small_encoder, "wide": wide_encoder}


def encoder_grads(m, feat, gout, metas, dtype, device, backend="torch"):
    m = copy.deepcopy(m).to(device).to(dtype).train().set_train_backend(backend)
    x = feat.detach().to(device=device, dtype=dtype).requires_grad_(True)
    out = m(x, metas) if backend == "hip" else m._forward_graph(x, metas)
    out.backward(gout.to(device=device, dtype=dtype))
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["feat"] = x.grad
    grads["out"] = out.detach()
    return grads


@pytest.mark.parametrize("name", ["small", "wide"])
def test_encoder_gradients_against_float64(cuda, name):
    m = ENCODERS[name]()
    feat, gout, metas = encoder_inputs(name)
    got = encoder_grads(m, feat, gout, metas, torch.float32, cuda, "hip")
    want = encoder_grads(m, feat, gout, metas, torch.float64, "cpu")
    lib32 = encoder_grads(m, feat, gout, metas, torch.float32, cuda)
    assert set(got) == set(want) and got["out"].shape == (feat.shape[0], feat.shape[2] * feat.shape[3], feat.shape[1])
    bad = {}
    for k in want:
        assert want[k] is not None and want[k].norm() > 0, k
        within_bar(f"{name} {k}", got[k], lib32[k], want[k], bad)
    assert not bad, bad


@pytest.mark.parametrize("name", ["small", "wide"])
def test_sgd_steps_track_the_torch_backend(cuda, name):
    feat, _, metas = encoder_inputs(name)
    feat = feat.to(cuda)
    losses = {}
    for mode in ("torch", "hip"):
        m = ENCODERS[name]().to(cuda).train().set_train_backend(mode)
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        seq = []
        for _ in range(3):
            opt.zero_grad()
            loss = (m(feat, metas) - 0.5).square().mean()
            loss.backward()
            opt.step()
            seq.append(loss.item())
        losses[mode] = seq
    t, h = np.array(losses["torch"]), np.array(losses["hip"])
    assert np.all(np.abs(h - t) <= 1e-3 * np.abs(t)), losses
    assert t[-1] != t[0]


def test_a_mask_length_of_zero_is_refused_on_the_host(cuda):
    m = small_encoder().to(cuda).train().set_train_backend("hip")
    feat, _, _ = encoder_inputs("small")
    with pytest.raises(ValueError, match="mask length 0"):
        m(feat.to(cuda), [dict(valid_ratio=1.0), dict(valid_ratio=0.0), dict(valid_ratio=0.5)])


def test_dropout_follows_torch_manual_seed(cuda):
    m = small_encoder(dropout=0.1).to(cuda).train().set_train_backend("hip")
    feat, _, metas = encoder_inputs("small")
    feat = feat.to(cuda)
    outs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        outs.append(m(feat, metas).detach())
    assert GA.same_bits(outs[0], outs[1])[0] and not GA.same_bits(outs[0], outs[2])[0]


# ---- 6. no library layer -------------------------------------------------------------------------------------------------
def test_no_library_layer_runs_in_a_hip_training_step(cuda, monkeypatch):
    m = small_encoder(dropout=0.1).to(cuda).train().set_train_backend("hip")
    feat, gout, metas = encoder_inputs("small")
    x = feat.to(cuda).requires_grad_(True)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the HIP training path")
        return f

    for name in ("linear", "layer_norm", "softmax", "gelu"):
        monkeypatch.setattr(F, name, refuse(f"F.{name}"))
    for name in ("matmul", "bmm"):
        monkeypatch.setattr(torch, name, refuse(f"torch.{name}"))
    out = m(x, metas)
    out.backward(gout.to(cuda))
    assert torch.isfinite(out).all() and x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
    with pytest.raises(AssertionError, match="called on the HIP training path"):
        m.set_train_backend("torch")(x, metas)


# ---- 7. eval mode --------------------------------------------------------------------------------------------------------
def test_eval_mode_does_not_depend_on_the_train_backend(cuda):
    m = small_encoder().to(cuda).eval()
    feat, _, metas = encoder_inputs("small")
    feat = feat.to(cuda)
    with torch.no_grad():
        a = m.set_train_backend("torch")(feat, metas)
        b = m.set_train_backend("hip")(feat, metas)
    ok, why = GA.same_bits(a, b)
    assert ok, why


# ---- 8. recogniser -------------------------------------------------------------------------------------------------------
def test_nrtr_forward_train_with_the_encoder_on_hip(cuda):
    import tps_pp_amd as P
    torch.manual_seed(0)
    m = P.build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                         strides=[2, 1, 2, 1, 2]),
                              tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                              decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                              label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
                              max_seq_len=8))
    m = m.to(cuda).train().set_train_backend("hip_all", backbone="hip", encoder="hip")
    assert (m.tpsnet.train_backend, m.backbone.train_backend, m.encoder.train_backend) == ("hip_all", "hip", "hip")
    assert m.encoder.dropout_p == 0.1
    img = torch.randn((2, 3, 32, 128), device=cuda)
    metas = [dict(resize_shape=(32, 128, 3), text="ab"), dict(resize_shape=(32, 100, 3), text="tps")]
    losses = m.forward_train(img, metas)
    sum(v.mean() for v in losses.values()).backward()
    for k, p in m.encoder.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
    for k, p in m.backbone.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


# ---- 9. guard bands and poison -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,heads,T,valid_len", [SHAPES[0], SHAPES[3]], ids=["T20", "T65"])
@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused"])
def test_guard_bands_and_poison(cuda, N, heads, T, valid_len, fused):
    q, k, v, gout = make_case(N, heads, T)
    C = 64 * heads
    with GA.guarded(cuda) as g:
        if fused:
            buf = g.input(torch.cat([q, k, v], dim=2))
            qd, kd, vd, ld = buf, buf[..., C:], buf[..., 2 * C:], 3 * C
        else:
            qd, kd, vd, ld = g.input(q), g.input(k), g.input(v), C
        gd = g.input(gout)
        vl = None if valid_len is None else g.input(torch.tensor(valid_len, dtype=torch.int32))
        served = 0
        for p in (0.0, 0.5):
            out, lse = ops.attn_train_fwd(qd, kd, vd, ld, N, C, heads, T, T, vl, p, 9, 1)
            if fused:
                grads = torch.empty((N, T, 3 * C), device=cuda, dtype=torch.float32)
                dq, dk, dv, ldg = grads, grads[..., C:], grads[..., 2 * C:], 3 * C
                produced = [grads]
            else:
                dq, dk, dv = (torch.empty((N, T, C), device=cuda, dtype=torch.float32) for _ in range(3))
                ldg, produced = C, [dq, dk, dv]
            ops.attn_train_bwd(gd, qd, kd, vd, ld, out, lse, N, C, heads, T, T, vl, p, 9, 1, dq, dk, dv, ldg)
            mask = ops.attn_dropout_mask(N, heads, T, T, p, 9, 1, cuda)
            served = g.check([out, lse] + produced, require_guarded=True)
            assert int(mask.max()) <= 1, "mask bytes never written (poison 0xFF)"
            assert torch.isfinite(out).all() and all(torch.isfinite(t).all() for t in produced)
        assert served == 2 * (3 + len(produced)) and not g.fallthrough, g.fallthrough
