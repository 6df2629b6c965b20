"""-m gpu: the five shared training entry points of tpspp_regressor_bwd.hip, called directly through their wrappers
(ops.mm, ops.linear_fwd, ops.linear_bwd_data, ops.linear_bwd_weight, ops.act_bwd, ops.plane_ln_fwd, ops.plane_ln_bwd) at
the smallest shapes that reach each staging path, tile tail and split boundary.

Two kinds of comparison:

A. EXACT.  Everything that is a sum of products runs on small integers stored as fp32 (A, B, x, dy in [-4, 4], bias and
   R in [-64, 64], alpha in {1, 0.5, -2}): every product and every partial sum, in any order, is an integer (or a half
   integer) far below 2^24, hence exactly representable, so the kernel must equal the float64 product formed on the CPU
   bit for bit whatever the order of the four MFMA chains or of the slab sums (tests/test_train_primitives_host.py
   checks the magnitudes of the inputs actually used).  Operands are placed in NaN-filled buffers through their strides
   (a read of an element that is not addressed poisons the result); C is written into a buffer prefilled with a sentinel
   bit pattern, margins included, and the whole buffer is compared, so an element between the addressed ones that
   changes is seen.  The float64 reference applies the epilogue's operations in the kernel's order (alpha * sum, + bias,
   ReLU, R + .), so signed zeros agree as well; a sum that is zero is +0.0, as every chain starts from +0.0 and rounds to
   nearest (the references add 0.0 to their sums, which turns a -0.0 from a single product 0 * -3 into that).

B. AGAINST FLOAT64 WITH THE PROJECT'S BAR (tests/test_gpu_regressor_train.py::check_block,
   tests/test_gpu_attn_train.py::within_bar, restated here unchanged): the relative L2 error against a float64
   composition on the CPU is <= max(1e-5, 2 x the error of PyTorch's fp32 composition of the same operation on the GPU
   against the same float64).  Every measured error is printed with its bar.

The case tables and the reference builders are module-level and need no GPU: the host file imports them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as GA
from tps_pp_amd import ops

pytestmark = pytest.mark.gpu

TILE = 64                  # mm_kernel / lin_wgrad_kernel: outputs per workgroup, each way
WAVE_TILE = 32             # ... per wavefront
SENTINEL = 0x7FA5A5A5      # a NaN no kernel produces: what C buffers hold before a launch
MARGIN = 64                # sentinel elements before and after the addressed span of C


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


# ---- strided host buffers -----------------------------------------------------------------------------------------------
def strided(buf, shape, strides):
    """View of the flat array `buf` with `strides` in elements."""
    return np.lib.stride_tricks.as_strided(buf, tuple(shape), tuple(int(s) * buf.itemsize for s in strides))


def span(shape, strides):
    """Elements from the first to one past the last addressed element (0 for an empty view)."""
    if any(n == 0 for n in shape):
        return 0
    return sum((n - 1) * abs(int(s)) for n, s in zip(shape, strides)) + 1


def offsets(shape, strides):
    """Element offset of every index of a view, as an int64 array of `shape`."""
    off = np.zeros(tuple(shape), np.int64)
    for ax, (n, s) in enumerate(zip(shape, strides)):
        ix = np.arange(n, dtype=np.int64) * int(s)
        off += ix.reshape([-1 if a == ax else 1 for a in range(len(shape))])
    return off


def place(logical, strides):
    """A NaN-filled flat fp32 buffer holding `logical` at `strides` (elements)."""
    buf = np.full((span(logical.shape, strides),), np.nan, np.float32)
    if buf.size:
        strided(buf, logical.shape, strides)[...] = logical
    return buf


def ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def tile_of(i, j):
    return (f"workgroup tile ({i // TILE}, {j // TILE}), wavefront tile ({i % TILE // WAVE_TILE}, "
            f"{j % TILE // WAVE_TILE}), in-tile ({i % TILE}, {j % TILE})")


def assert_same_bits(label, got, want, names=("i", "j")):
    """Bit equality of two equally shaped fp32 arrays; names the first differing index and its tile."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, f"{label}: shape {got.shape} against {want.shape}"
    diff = bits(got) != bits(want)
    if not diff.any():
        return
    idx = tuple(int(v) for v in np.argwhere(diff)[0])
    where = ", ".join(f"{n} = {v}" for n, v in zip(names, idx[-len(names):]))
    lead = f"{idx[:-len(names)]} " if len(idx) > len(names) else ""
    ij = idx[-2:] if len(idx) >= 2 else (0, idx[0])
    raise AssertionError(f"{label}: {int(diff.sum())} of {diff.size} elements differ, the first at {lead}{where}: got "
                         f"{got[idx]!r}, want {want[idx]!r}; {tile_of(*ij)}")


# ---- tpspp_mm_f32: the exact cases ------------------------------------------------------------------------------------------
LAYOUTS = ("k", "row", "gap")                    # k fastest, row fastest, neither unit
ALPHAS = (1.0, 0.5, -2.0)
MM_SHAPES = ((1, 1, 1, 1), (1, 1, 65, 2), (1, 65, 1, 3), (1, 33, 31, 15), (1, 64, 64, 16), (1, 65, 65, 17),
             (1, 130, 33, 33), (3, 33, 65, 31), (2, 64, 64, 1))
MM_KTOTAL = (48, 40, 33, 20)                     # batch 3, K 16: last entry full, 8, 1, and K_b = -12 (an empty sum)


def operand_strides(layout, rows, K):
    """(row stride, k stride) of a (rows, K) operand."""
    if layout == "k":
        return K, 1
    if layout == "row":
        return 1, rows
    return 2 * K + 3, 2


def c_gap_strides(M, N):
    return M * (2 * N + 1) + 5, 2 * N + 1, 2


def _mm_exact_cases():
    out, idx = [], 0
    for s, (b, M, N, K) in enumerate(MM_SHAPES):
        for ia, la in enumerate(LAYOUTS):
            for ib, lb in enumerate(LAYOUTS):
                out.append(dict(id=f"b{b}-m{M}-n{N}-k{K}-A{la}-B{lb}", batch=b, M=M, N=N, K=K, la=la, lb=lb,
                                bias=bool(idx & 1), R=bool(idx & 2), b_shared=bool(idx & 4),
                                alpha=ALPHAS[(s + ia + ib) % 3], epi=(idx // 3) % 2, k_total=0, c_layout="gap", seed=idx))
                idx += 1
    return out


def _mm_ktotal_cases():
    out = []
    for n, kt in enumerate(MM_KTOTAL):
        for m, (la, lb) in enumerate((("k", "k"), ("row", "gap"), ("gap", "row"), ("k", "row"))):
            idx = 4 * n + m                      # m: all four of bias / R present or absent, per k_total
            out.append(dict(id=f"ktotal{kt}-A{la}-B{lb}", batch=3, M=33, N=65, K=16, la=la, lb=lb, bias=bool(idx & 1),
                            R=bool(idx & 2), b_shared=False, alpha=ALPHAS[idx % 3], epi=(idx // 2) % 2, k_total=kt,
                            c_layout="gap", seed=500 + idx))
    return out


MM_EXACT = _mm_exact_cases()
MM_KTOTAL_CASES = _mm_ktotal_cases()
MM_NCHW_CASE = dict(id="b3-m33-n65-k31-C-nchw", batch=3, M=33, N=65, K=31, la="k", lb="k", bias=True, R=True,
                    b_shared=True, alpha=0.5, epi=1, k_total=0, c_layout="nchw", seed=900)
MM_GUARD_CASE = dict(id="b3-m33-n65-k31-guarded", batch=3, M=33, N=65, K=31, la="gap", lb="row", bias=True, R=True,
                     b_shared=False, alpha=-2.0, epi=1, k_total=0, c_layout="dense", seed=901)


def mm_kb(c, q):
    """K_b of batch entry q (include/tpspp.h), floored at 0: an empty sum."""
    if c["k_total"] <= 0:
        return c["K"]
    return max(0, min(c["K"], c["k_total"] - q * c["K"]))


def mm_build(c):
    """Host side of one exact case: the logical integer matrices, the NaN-filled operand buffers with their strides, and
    C's geometry.  With k_total the batch entries of A and B are consecutive K-wide column blocks of one (rows, batch * K)
    matrix (batch stride K * k stride), NaN from column k_total on: nothing past the reduction may be read."""
    rng = np.random.default_rng(1000 + c["seed"])
    b, M, N, K, kt = c["batch"], c["M"], c["N"], c["K"], c["k_total"]
    h = {}
    if kt:
        A2, B2 = ints(rng, (M, b * K), 4), ints(rng, (N, b * K), 4)
        A2[:, kt:] = np.nan
        B2[:, kt:] = np.nan
        sai, sak = operand_strides(c["la"], M, b * K)
        sbj, sbk = operand_strides(c["lb"], N, b * K)
        h["A"], h["B"] = place(A2, (sai, sak)), place(B2, (sbj, sbk))
        h["a_strides"], h["b_strides"] = (K * sak, sai, sak), (K * sbk, sbj, sbk)
        h["A_log"] = np.stack([A2[:, q * K:(q + 1) * K] for q in range(b)])
        h["B_log"] = np.stack([B2[:, q * K:(q + 1) * K] for q in range(b)])
    else:
        nb_b = 1 if c["b_shared"] else b
        h["A_log"], B_own = ints(rng, (b, M, K), 4), ints(rng, (nb_b, N, K), 4)
        sai, sak = operand_strides(c["la"], M, K)
        sbj, sbk = operand_strides(c["lb"], N, K)
        sab = span((M, K), (sai, sak)) + 3
        sbb = span((N, K), (sbj, sbk)) + 1
        h["A"] = place(h["A_log"], (sab, sai, sak))
        h["B"] = place(B_own, (sbb, sbj, sbk))
        h["a_strides"], h["b_strides"] = (sab, sai, sak), (0 if c["b_shared"] else sbb, sbj, sbk)
        h["B_log"] = np.broadcast_to(B_own, (b, N, K)) if c["b_shared"] else B_own
    h["bias"] = ints(rng, (N,), 64) if c["bias"] else None
    if c["c_layout"] == "gap":
        h["c_strides"] = c_gap_strides(M, N)
    elif c["c_layout"] == "nchw":                # C is an (batch, N, M) map, its tokens (b c hw -> b hw c)
        h["c_strides"] = ops._nchw_tokens(torch.empty(b, N, M))[2:]
    else:
        h["c_strides"] = (M * N, N, 1)
    h["c_span"] = span((b, M, N), h["c_strides"])
    h["R_log"] = ints(rng, (b, M, N), 64) if c["R"] else None
    h["R"] = None
    if c["R"]:
        h["R"] = np.full((h["c_span"] + 2 * MARGIN,), np.nan, np.float32)
        strided(h["R"][MARGIN:], (b, M, N), h["c_strides"])[...] = h["R_log"]
    return h


def epilogue64(acc, alpha, bias, epi, R):
    """The kernel's epilogue in float64, operation by operation (exact on the integer cases, signed zeros included)."""
    v = np.float64(alpha) * acc
    if bias is not None:
        v = v + bias.astype(np.float64)
    if epi == 1:
        v = np.where(v > 0.0, v, 0.0)
    if R is not None:
        v = R.astype(np.float64) + v
    return v


def mm_reference(c, h):
    """-> (sums (batch, M, N) float64, C (batch, M, N) fp32), read through the strides from the operand buffers."""
    b, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    A = strided(h["A"], (b, M, K), h["a_strides"]).astype(np.float64)
    B = strided(h["B"], (b, N, K), h["b_strides"]).astype(np.float64)
    acc = np.zeros((b, M, N), np.float64)
    for q in range(b):
        kb = mm_kb(c, q)
        acc[q] = A[q, :, :kb] @ B[q, :, :kb].T + 0.0
    R = strided(h["R"][MARGIN:], (b, M, N), h["c_strides"]) if c["R"] else None
    return acc, epilogue64(acc, c["alpha"], h["bias"], c["epi"], R).astype(np.float32)


def mm_expected_buffer(c, h, want):
    """The whole C buffer after the launch, as int32: the sentinel everywhere but at the addressed elements."""
    buf = np.full((h["c_span"] + 2 * MARGIN,), SENTINEL, np.int32)
    if want.size:
        strided(buf[MARGIN:], want.shape, h["c_strides"])[...] = bits(want)
    return buf


def mm_explain(c, h, got, want_buf):
    """None if the buffers agree, else a message naming the first wrong (b, i, j) and its tile, or the stray offset."""
    bad = np.flatnonzero(got != want_buf)
    if not bad.size:
        return None
    first = int(bad[0]) - MARGIN
    shape = (c["batch"], c["M"], c["N"])
    hit = np.argwhere(offsets(shape, h["c_strides"]) == first) if all(shape) else np.zeros((0, 3), np.int64)
    g, w = got[bad[0]:bad[0] + 1].view(np.float32)[0], want_buf[bad[0]:bad[0] + 1].view(np.float32)[0]
    if not len(hit):
        return (f"{c['id']}: {bad.size} elements wrong; the first is offset {first} from C, which (b, i, j) never "
                f"addresses, and it no longer holds the sentinel: {g!r} (0x{int(got[bad[0]]) & 0xFFFFFFFF:08X})")
    q, i, j = (int(v) for v in hit[0])
    return (f"{c['id']}: {bad.size} elements wrong; the first is (b, i, j) = ({q}, {i}, {j}): got {g!r}, want {w!r}; "
            f"{tile_of(i, j)}; K_b = {mm_kb(c, q)}, strides A {h['a_strides']} B {h['b_strides']} C {h['c_strides']}")


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_mm_exact(dev, c):
    h = mm_build(c)
    _, want = mm_reference(c, h)
    want_buf = mm_expected_buffer(c, h, want)
    Cb = _dev(np.full_like(want_buf, SENTINEL), dev).view(torch.float32)
    Rb = _dev(h["R"], dev)
    ops.mm(_dev(h["A"], dev), h["a_strides"], _dev(h["B"], dev), h["b_strides"], Cb[MARGIN:], h["c_strides"], c["batch"],
           c["M"], c["N"], c["K"], bias=_dev(h["bias"], dev), R=None if Rb is None else Rb[MARGIN:], epi=c["epi"],
           alpha=c["alpha"], k_total=c["k_total"])
    msg = mm_explain(c, h, Cb.view(torch.int32).cpu().numpy(), want_buf)
    assert msg is None, msg


@pytest.mark.parametrize("c", MM_EXACT, ids=[c["id"] for c in MM_EXACT])
def test_mm_exact(cuda, c):
    """Tails in M, N and K (odd K, K % 16 != 0, K = 1), all nine staging-path pairs, batch > 1 with a shared or an own B,
    bias / R present or absent, C through strides that leave gaps: bit-equal, and nothing else in C's buffer changes."""
    run_mm_exact(cuda, c)


@pytest.mark.parametrize("c", MM_KTOTAL_CASES, ids=[c["id"] for c in MM_KTOTAL_CASES])
def test_mm_k_total_exact(cuda, c):
    """One reduction split over the batch: K_b = min(K, k_total - b*K), the last entry full, 8, 1 and empty (K_b <= 0:
    C = epi(bias) (+ R)).  Columns of A and B from k_total on are NaN."""
    run_mm_exact(cuda, c)


def test_mm_exact_nchw_token_output(cuda):
    """C and R in the token layout of an NCHW map (ops._nchw_tokens): every element of the map is written."""
    run_mm_exact(cuda, MM_NCHW_CASE)


@pytest.mark.parametrize("empty", ["batch", "M", "N"])
def test_mm_empty_products_write_nothing(cuda, empty):
    c = dict(MM_EXACT[7 * 9], id=f"empty-{empty}")
    h = mm_build(c)
    sizes = dict(batch=c["batch"], M=c["M"], N=c["N"])
    sizes[empty] = 0
    Cb = _dev(np.full((h["c_span"] + 2 * MARGIN,), SENTINEL, np.int32), cuda).view(torch.float32)
    ops.mm(_dev(h["A"], cuda), h["a_strides"], _dev(h["B"], cuda), h["b_strides"], Cb[MARGIN:], h["c_strides"],
           sizes["batch"], sizes["M"], sizes["N"], c["K"], bias=_dev(h["bias"], cuda))
    torch.cuda.synchronize()
    assert bool((Cb.view(torch.int32) == SENTINEL).all()), f"{empty} = 0 wrote to C"


# ---- tpspp_mm_f32: the epilogues that round (comparison B) ---------------------------------------------------------------
MM_ROUNDED = [dict(id=f"b{b}-m{M}-n{N}-k{K}-epi{epi}-{'R' if R else 'noR'}", batch=b, M=M, N=N, K=K, epi=epi, R=R,
                   alpha=0.125)
              for (b, M, N, K) in ((3, 33, 65, 31), (1, 65, 65, 17)) for epi in (2, 3) for R in (False, True)]
MM_SATURATED = dict(id="b1-m65-n65-k17-tanh-alpha64", batch=1, M=65, N=65, K=17, epi=3, R=False, alpha=64.0)


@functools.lru_cache(maxsize=None)
def _mm_rounded_inputs(b, M, N, K):
    g = torch.Generator().manual_seed(7 * b + 11 * M + 13 * N + 17 * K)
    return tuple(torch.randn(s, generator=g) for s in ((b, M, K), (b, N, K), (N,), (b, M, N)))


def mm_rounded_compose(c, A, B, bias, R):
    """epi(alpha * A B^T + bias) (+ R) with torch operators, in the dtype and on the device of the operands."""
    z = c["alpha"] * torch.matmul(A, B.transpose(1, 2)) + bias
    z = F.gelu(z) if c["epi"] == 2 else torch.tanh(z)
    return z + R if c["R"] else z


def run_mm_rounded(dev, c):
    A, B, bias, R = _mm_rounded_inputs(c["batch"], c["M"], c["N"], c["K"])
    b, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    want = mm_rounded_compose(c, A.double(), B.double(), bias.double(), R.double())
    Ad, Bd, bd, Rd = (t.to(dev) for t in (A, B, bias, R))
    lib32 = mm_rounded_compose(c, Ad, Bd, bd, Rd)
    C = torch.empty((b, M, N), device=dev)
    ops.mm(Ad, (M * K, K, 1), Bd, (N * K, K, 1), C, (M * N, N, 1), b, M, N, K, bias=bd, R=Rd if c["R"] else None,
           epi=c["epi"], alpha=c["alpha"])
    return C, lib32, want


@pytest.mark.parametrize("c", MM_ROUNDED, ids=[c["id"] for c in MM_ROUNDED])
def test_mm_gelu_tanh_epilogues(cuda, c):
    C, lib32, want = run_mm_rounded(cuda, c)
    bad = {}
    within_bar(f"mm {c['id']}", C, lib32, want, bad)
    assert not bad, bad


def test_mm_tanh_saturates_finite(cuda):
    """alpha = 64: almost every pre-activation is far in tanh's tails.  Finite everywhere, never beyond +-1, and exactly
    +-1 wherever |z| > 20 (1 - tanh(20) = 8e-18, far below half an ulp of 1), besides the bar."""
    c = MM_SATURATED
    C, lib32, want = run_mm_rounded(cuda, c)
    A, B, bias, _ = _mm_rounded_inputs(c["batch"], c["M"], c["N"], c["K"])
    z = c["alpha"] * torch.matmul(A.double(), B.double().transpose(1, 2)) + bias.double()
    got = C.cpu()
    assert torch.isfinite(got).all()
    assert float(got.abs().max()) <= 1.0
    far = z.abs() > 20
    assert int(far.sum()) > far.numel() // 2
    assert torch.equal(got[far], torch.sign(z[far]).float()), "tanh epilogue not exactly +-1 in its tails"
    bad = {}
    within_bar(f"mm {c['id']}", C, lib32, want, bad)
    assert not bad, bad


# ---- ops.linear_fwd / ops.linear_bwd_data on an NCHW map ------------------------------------------------------------------
LINEAR_NCHW = dict(N=3, C=17, H=5, W=7, O=65)


@functools.lru_cache(maxsize=None)
def linear_nchw_case():
    """Integer x (N, C, H, W), weight (O, C), bias (O), dy (N*H*W, O), and the exact y and dx."""
    d = LINEAR_NCHW
    rng = np.random.default_rng(77)
    x = ints(rng, (d["N"], d["C"], d["H"], d["W"]), 4)
    w, bias = ints(rng, (d["O"], d["C"]), 4), ints(rng, (d["O"],), 64)
    dy = ints(rng, (d["N"] * d["H"] * d["W"], d["O"]), 4)
    tok = x.reshape(d["N"], d["C"], -1).transpose(0, 2, 1).reshape(-1, d["C"]).astype(np.float64)
    y = tok @ w.astype(np.float64).T + bias
    dtok = dy.astype(np.float64) @ w.astype(np.float64) + 0.0                 # (N*HW, C)
    dx = dtok.reshape(d["N"], -1, d["C"]).transpose(0, 2, 1).reshape(x.shape)
    return dict(x=x, w=w, bias=bias, dy=dy, y=y.astype(np.float32), dx=dx.astype(np.float32))


def test_linear_fwd_bwd_data_nchw_exact(cuda):
    k = linear_nchw_case()
    x, w = _dev(k["x"], cuda), _dev(k["w"], cuda)
    desc = ops._nchw_tokens(x)
    y = ops.linear_fwd(x, desc, w, _dev(k["bias"], cuda))
    assert_same_bits("linear_fwd on NCHW tokens", y.cpu().numpy(), k["y"], names=("row", "o"))
    dx = torch.full_like(x, float("nan")).view(torch.int32).fill_(-1).view(torch.float32)      # poison 0xFFFFFFFF
    ops.linear_bwd_data(_dev(k["dy"], cuda), w, dx, desc)
    assert GA.poison_count(dx) == 0, "linear_bwd_data left elements of the NCHW map unwritten"
    got = dx.cpu().numpy()
    hw = LINEAR_NCHW["H"] * LINEAR_NCHW["W"]
    assert_same_bits("linear_bwd_data into an NCHW map (i = channel, j = pixel; the kernel's tile is (pixel, channel))",
                     got.reshape(-1, LINEAR_NCHW["C"], hw), k["dx"].reshape(-1, LINEAR_NCHW["C"], hw), names=("c", "p"))


# ---- tpspp_linear_bwd_weight ------------------------------------------------------------------------------------------------
# S / L: the documented fixed split of each case (tests/test_train_primitives_host.py holds them to the workspace query)
WG_EXACT = [
    dict(id="m1-o1-k1", M=1, O=1, K=1, layout="dense", lim=4, S=1, L=256),
    dict(id="m255-o65-k17", M=255, O=65, K=17, layout="dense", lim=4, S=1, L=256),
    dict(id="m256-o64-k64", M=256, O=64, K=64, layout="dense", lim=4, S=1, L=256),
    dict(id="m257-o65-k17", M=257, O=65, K=17, layout="dense", lim=4, S=2, L=256),          # last slice: one row
    dict(id="m513-o1-k130", M=513, O=1, K=130, layout="dense", lim=4, S=3, L=256),
    dict(id="m131089-o3-k5", M=131073 + 16, O=3, K=5, layout="dense", lim=3, S=482, L=272),  # M > 512 * 256
    dict(id="nchw-n3-hw100-c17-o33", M=300, O=33, K=17, layout="nchw", nb=3, lim=4, S=2, L=256),  # boundary inside image 2
    dict(id="m257-o65-k17-padded", M=257, O=65, K=17, layout="padded", lim=4, S=2, L=256),  # neither stride is 1
]
WG_MODES = ("both", "weight", "bias")
WG_ROUNDED = [c for c in WG_EXACT if c["id"] in ("m257-o65-k17", "nchw-n3-hw100-c17-o33")]
WG_SPLIT = [c for c in WG_EXACT if c["S"] > 1]


def wg_desc(c):
    """The token descriptor (nb, Mi, sb, si, sk) of x (ops.py)."""
    M, K = c["M"], c["K"]
    if c["layout"] == "dense":
        return ops._dense(M, K)
    if c["layout"] == "padded":
        return (1, M, 0, 2 * K + 3, 2)
    hw = M // c["nb"]
    return (c["nb"], hw, K * hw, 1, hw)


def wg_place(c, x_log):
    """x (M, K) in a NaN-filled buffer at the case's layout."""
    nb, Mi, sb, si, sk = wg_desc(c)
    return place(x_log.reshape(nb, Mi, c["K"]), (sb, si, sk))


def wg_read(c, buf):
    nb, Mi, sb, si, sk = wg_desc(c)
    return strided(buf, (nb, Mi, c["K"]), (sb, si, sk)).reshape(c["M"], c["K"])


@functools.lru_cache(maxsize=None)
def wg_exact_case(cid):
    c = next(k for k in WG_EXACT if k["id"] == cid)
    rng = np.random.default_rng(2000 + WG_EXACT.index(c))
    dy, x_log = ints(rng, (c["M"], c["O"]), c["lim"]), ints(rng, (c["M"], c["K"]), c["lim"])
    xbuf = wg_place(c, x_log)
    dw = dy.astype(np.float64).T @ wg_read(c, xbuf).astype(np.float64) + 0.0
    db = dy.astype(np.float64).sum(0) + 0.0
    return dict(dy=dy, x_log=x_log, x=xbuf, dw=dw.astype(np.float32), db=db.astype(np.float32))


def run_wg(dev, c, dy, xbuf, mode, x_gelu=False):
    return ops.linear_bwd_weight(_dev(dy, dev) if isinstance(dy, np.ndarray) else dy,
                                 _dev(xbuf, dev) if isinstance(xbuf, np.ndarray) else xbuf, wg_desc(c), c["O"], c["K"],
                                 want_weight=mode != "bias", want_bias=mode != "weight", x_gelu=x_gelu)


@pytest.mark.parametrize("mode", WG_MODES)
@pytest.mark.parametrize("c", WG_EXACT, ids=[c["id"] for c in WG_EXACT])
def test_linear_bwd_weight_exact(cuda, c, mode):
    k = wg_exact_case(c["id"])
    dw, db = run_wg(cuda, c, k["dy"], k["x"], mode)
    assert (dw is None) == (mode == "bias") and (db is None) == (mode == "weight")
    if dw is not None:
        assert_same_bits(f"dweight {c['id']} ({mode}, S = {c['S']}, L = {c['L']})", dw.cpu().numpy(), k["dw"],
                         names=("o", "k"))
    if db is not None:
        assert_same_bits(f"dbias {c['id']} ({mode}, S = {c['S']}, L = {c['L']})", db.cpu().numpy(), k["db"], names=("o",))


@functools.lru_cache(maxsize=None)
def wg_rounded_case(cid):
    c = next(k for k in WG_EXACT if k["id"] == cid)
    g = torch.Generator().manual_seed(3000 + WG_EXACT.index(c))
    dy, x_log = torch.randn((c["M"], c["O"]), generator=g), torch.randn((c["M"], c["K"]), generator=g)
    xbuf = wg_place(c, x_log.numpy())
    return dict(dy=dy, x_log=x_log, x=xbuf, dw=dy.double().t() @ F.gelu(x_log.double()), db=dy.double().sum(0))


@pytest.mark.parametrize("c", WG_ROUNDED, ids=[c["id"] for c in WG_ROUNDED])
def test_linear_bwd_weight_gelu_input(cuda, c):
    """x_act = 2: dW = dy^T gelu(x), the GELU applied while x is staged."""
    k = wg_rounded_case(c["id"])
    dyd, xd = k["dy"].to(cuda), k["x_log"].to(cuda)
    dw, db = run_wg(cuda, c, dyd, k["x"], "both", x_gelu=True)
    bad = {}
    within_bar(f"linear_bwd_weight gelu {c['id']} dweight", dw, dyd.t() @ F.gelu(xd), k["dw"], bad)
    within_bar(f"linear_bwd_weight gelu {c['id']} dbias", db, dyd.sum(0), k["db"], bad)
    assert not bad, bad


@pytest.mark.parametrize("x_gelu", [False, True])
@pytest.mark.parametrize("c", WG_SPLIT, ids=[c["id"] for c in WG_SPLIT])
def test_linear_bwd_weight_same_bits_on_another_stream(cuda, c, x_gelu):
    """Fixed split-K: two calls on rounding inputs, the second on another stream, agree bit for bit at every S > 1."""
    g = torch.Generator().manual_seed(4000 + WG_EXACT.index(c))
    dy = torch.randn((c["M"], c["O"]), generator=g).to(cuda)
    x = _dev(wg_place(c, torch.randn((c["M"], c["K"]), generator=g).numpy()), cuda)
    first = run_wg(cuda, c, dy, x, "both", x_gelu)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        second = run_wg(cuda, c, dy, x, "both", x_gelu)
    side.synchronize()
    torch.cuda.synchronize()
    ok, why = GA.same_bits(first, second)
    assert ok, f"{c['id']}: {why}"
    assert all(torch.isfinite(t).all() for t in first)


# ---- tpspp_plane_ln_fwd / _bwd ---------------------------------------------------------------------------------------------
# S / L: the fixed split of the parameter gradient (split_rows(rows, 16))
LN_CASES = [
    dict(id="r1-p1", rows=1, P=1, S=1, L=16),
    dict(id="r1-p255", rows=1, P=255, S=1, L=16),            # fewer elements than threads in block_sum
    dict(id="r3-p256", rows=3, P=256, S=1, L=16),
    dict(id="r17-p257", rows=17, P=257, S=2, L=16),
    dict(id="r33-p1024", rows=33, P=1024, S=3, L=16),
    dict(id="r8193-p8", rows=8193, P=8, S=257, L=32),
]
LN_EPS = (1e-5, 1e-6)
LN_KINDS = ("randn", "const", "offset")
LN_VARIANT_CASES = [c for c in LN_CASES if c["id"] in ("r3-p256", "r17-p257")]
LN_CONST = 2.5             # dyadic: a plane of it sums and divides exactly, so mean == x and every deviation is 0


@functools.lru_cache(maxsize=None)
def ln_case(cid, eps, kind="randn"):
    """fp32 inputs and the float64 results of F.layer_norm and its autograd on the CPU (computed once, shared)."""
    c = next(k for k in LN_CASES if k["id"] == cid)
    rows, P = c["rows"], c["P"]
    g = torch.Generator().manual_seed(5000 + LN_CASES.index(c) + 100 * LN_KINDS.index(kind))
    x = torch.randn((rows, P), generator=g)
    const_row = rows // 2
    if kind == "const":
        x[const_row] = LN_CONST
    elif kind == "offset":
        x = 100.0 + 0.01 * x
    w, b = 1.0 + 0.5 * torch.randn((P,), generator=g), torch.randn((P,), generator=g)
    dy, dx0 = torch.randn((rows, P), generator=g), torch.randn((rows, P), generator=g)
    dy_int = torch.randint(-4, 5, (rows, P), generator=g).float()
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    y64 = F.layer_norm(x64, (P,), w64, b64, eps)
    gx, gw, gb = torch.autograd.grad(y64, (x64, w64, b64), dy.double())
    mean64 = x.double().mean(1)
    rstd64 = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + eps)
    return dict(x=x, w=w, b=b, dy=dy, dx0=dx0, dy_int=dy_int, const_row=const_row, y=y64.detach(), mean=mean64,
                rstd=rstd64, dx=gx, dx_acc=dx0.double() + gx, dw=gw, db=gb, db_int=dy_int.double().sum(0) + 0.0)


def ln_lib32(k, eps, dev):
    """PyTorch's fp32 LayerNorm on the GPU: y, mean, rstd, and the gradients for dy."""
    x, w, b = (k[n].to(dev).requires_grad_() for n in ("x", "w", "b"))
    y, mean, rstd = torch.native_layer_norm(x, (x.shape[1],), w, b, eps)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), k["dy"].to(dev))
    return dict(y=y.detach(), mean=mean.reshape(-1), rstd=rstd.reshape(-1), dx=gx, dx_acc=k["dx0"].to(dev) + gx, dw=gw,
                db=gb)


def run_ln(dev, cid, eps, kind="randn"):
    """Every result of the forward and the backward of one case under the bar; -> the case, the saved statistics."""
    k = ln_case(cid, eps, kind)
    lib = ln_lib32(k, eps, dev)
    x, w, b, dy = (k[n].to(dev) for n in ("x", "w", "b", "dy"))
    label = f"plane_ln {cid} eps {eps:g} {kind}"
    bad = {}
    y, mean, rstd = ops.plane_ln_fwd(x, w, b, eps)
    for name, got in (("y", y), ("mean", mean), ("rstd", rstd)):
        within_bar(f"{label} {name}", got, lib[name], k[name], bad)
    dx = torch.full_like(x, float("nan"))
    dw, db = ops.plane_ln_bwd(dy, x, w, mean, rstd, dx=dx, accumulate=False, want_params=True)
    within_bar(f"{label} dx", dx, lib["dx"], k["dx"], bad)
    within_bar(f"{label} dweight", dw, lib["dw"], k["dw"], bad)
    within_bar(f"{label} dbias (rounding dy)", db, lib["db"], k["db"], bad)
    if x.shape[1] == 1:
        # P = 1: x - mean is exactly 0, so xhat, dx and dweight are exactly 0 and y == bias.  (float64 autograd leaves a
        # residue of 1e-13 in its dx here, so the relative error printed above is 1 for an exact result and says nothing.)
        assert not dx.any() and not dw.any() and torch.equal(y, b.expand_as(y)) and torch.equal(mean, x.reshape(-1))
    dxa = k["dx0"].to(dev)
    none =ops.plane_ln_bwd(dy, x, w, mean, rstd, dx=dxa, accumulate=True, want_params=False)
    assert none == (None, None)
    within_bar(f"{label} dx accumulate=1", dxa, lib["dx_acc"], k["dx_acc"], bad)
    _, dbi = ops.plane_ln_bwd(k["dy_int"].to(dev), x, w, mean, rstd, dx=None, want_params=True)
    assert_same_bits(f"{label} dbias of integer dy (S = {next(c for c in LN_CASES if c['id'] == cid)['S']})",
                     dbi.cpu().numpy(), k["db_int"].float().numpy(), names=("p",))
    assert not bad, bad
    return k, (x, w, b, dy, y, mean, rstd, dx, dw, db)


@pytest.mark.parametrize("eps", LN_EPS)
@pytest.mark.parametrize("c", LN_CASES, ids=[c["id"] for c in LN_CASES])
def test_plane_ln_fwd_bwd(cuda, c, eps):
    run_ln(cuda, c["id"], eps)


@pytest.mark.parametrize("c", LN_VARIANT_CASES, ids=[c["id"] for c in LN_VARIANT_CASES])
def test_plane_ln_bwd_output_subsets(cuda, c):
    """want_params=False with dx, and dx=None with parameters: each the same bits as the call that forms everything."""
    _, (x, w, b, dy, y, mean, rstd, dx, dw, db) = run_ln(cuda, c["id"], 1e-5)
    dx_only = torch.full_like(x, float("nan"))
    assert ops.plane_ln_bwd(dy, x, w, mean, rstd, dx=dx_only, want_params=False) == (None, None)
    ok, why = GA.same_bits(dx_only, dx)
    assert ok, f"dx alone: {why}"
    dw2, db2 = ops.plane_ln_bwd(dy, x, w, mean, rstd, dx=None, want_params=True)
    ok, why = GA.same_bits((dw2, db2), (dw, db))
    assert ok, f"parameters alone: {why}"


@pytest.mark.parametrize("eps", LN_EPS)
@pytest.mark.parametrize("c", LN_VARIANT_CASES, ids=[c["id"] for c in LN_VARIANT_CASES])
def test_plane_ln_constant_plane(cuda, c, eps):
    """One plane constant: variance 0, y == bias exactly there, rstd = 1 / sqrt(eps), everything finite and in the bar."""
    k, (x, w, b, dy, y, mean, rstd, dx, dw, db) = run_ln(cuda, c["id"], eps, "const")
    r = k["const_row"]
    assert torch.equal(mean[r].cpu(), torch.tensor(LN_CONST))
    assert torch.equal(y[r].cpu(), k["b"]), "y != bias on the constant plane"
    assert all(torch.isfinite(t).all() for t in (y, mean, rstd, dx, dw, db))


@pytest.mark.parametrize("c", [c for c in LN_CASES if c["id"] in ("r17-p257", "r33-p1024")], ids=lambda c: c["id"])
def test_plane_ln_cancellation(cuda, c):
    """x = 100 + 0.01 * randn: the variance is 1e-8 of the mean square."""
    run_ln(cuda, c["id"], 1e-5, "offset")


# ---- tpspp_act_bwd ------------------------------------------------------------------------------------------------------------
ACT_N = (1, 255, 256, 257, 100003)
ACT_TANH_SCALE = 0.125
TINY = float(np.float32(2.0 ** -149))            # the smallest positive subnormal
RELU_SPECIALS = (0.0, -0.0, TINY, -1.0, -TINY, 3.0)
TANH_SPECIALS = (1.0, -1.0, 0.0)
GELU_SPECIALS = (12.0, -12.0, 40.0, -40.0, 0.0)
ACT_SPECIAL_EVERY = 7


def with_specials(t, specials):
    """`t` with specials[m] at index ACT_SPECIAL_EVERY * m (cyclically): index 0 always holds specials[0]."""
    t = np.array(t, np.float32)
    at = np.arange(0, t.size, ACT_SPECIAL_EVERY)
    t[at] = np.asarray(specials, np.float32)[(at // ACT_SPECIAL_EVERY) % len(specials)]
    return t


@functools.lru_cache(maxsize=None)
def act_case(op, n):
    """g, t (fp32 numpy) and the float64 result of `tpspp_act_bwd` op (0 ReLU: exact; 1 GELU; 2 tanh)."""
    rng = np.random.default_rng(6000 + 10 * n + op)
    if op == ops.ACT_RELU:
        g, t = ints(rng, (n,), 4), with_specials(ints(rng, (n,), 4), RELU_SPECIALS)
        return dict(g=g, t=t, want=np.where(t > 0, g, np.float32(0.0)).astype(np.float64))
    g = rng.standard_normal(n).astype(np.float32)
    if op == ops.ACT_GELU:
        t = with_specials(3.0 * rng.standard_normal(n), GELU_SPECIALS)
        x64 = torch.from_numpy(t).double().requires_grad_()
        (want,) = torch.autograd.grad(F.gelu(x64), x64, torch.from_numpy(g).double())
        return dict(g=g, t=t, want=want.numpy())
    u = 8.0 * rng.standard_normal(n)
    t = with_specials(np.tanh(ACT_TANH_SCALE * u), TANH_SPECIALS)
    t64 = t.astype(np.float64)
    return dict(g=g, t=t, want=g.astype(np.float64) * (1.0 - t64 * t64) * ACT_TANH_SCALE)


def act_lib32(op, g, t):
    """PyTorch's fp32 composition of the same backward on the GPU."""
    if op == ops.ACT_GELU:
        x = t.clone().requires_grad_()
        return torch.autograd.grad(F.gelu(x), x, g)[0]
    return g * (1.0 - t * t) * ACT_TANH_SCALE


@pytest.mark.parametrize("alias", [False, True], ids=["out", "in-place"])
@pytest.mark.parametrize("op", [ops.ACT_RELU, ops.ACT_GELU, ops.ACT_TANH], ids=["relu", "gelu", "tanh"])
@pytest.mark.parametrize("n", ACT_N)
def test_act_bwd(cuda, n, op, alias):
    k = act_case(op, n)
    g, t = _dev(k["g"], cuda), _dev(k["t"], cuda)
    scale = ACT_TANH_SCALE if op == ops.ACT_TANH else 1.0
    if alias:
        buf = g.clone()
        out = ops.act_bwd(op, buf, t, scale, out=buf)
        assert out.data_ptr() == buf.data_ptr()
    else:
        out = ops.act_bwd(op, g, t, scale)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    if op == ops.ACT_RELU:                       # 0.0, -0.0 and negatives pass nothing; the smallest subnormal passes g
        assert_same_bits(f"act_bwd relu n {n}", got, k["want"].astype(np.float32), names=("e",))
        return
    if op == ops.ACT_TANH:
        ones = np.abs(k["t"]) == 1.0
        assert ones.any() and not got[ones].any(), "tanh backward at t = +-1 is not exactly 0"
    bad = {}
    within_bar(f"act_bwd op {op} n {n} {'in place' if alias else 'out'}", out, act_lib32(op, g, t),
               torch.from_numpy(k["want"]), bad)
    assert not bad, bad


# ---- the ragged cases inside guard bands ----------------------------------------------------------------------------------------
def test_guarded_mm(cuda):
    c = MM_GUARD_CASE
    h = mm_build(c)
    _, want = mm_reference(c, h)
    with GA.guarded(cuda) as g:
        A, B = g.input(torch.from_numpy(h["A"])), g.input(torch.from_numpy(h["B"]))
        bias, R = g.input(torch.from_numpy(h["bias"])), g.input(torch.from_numpy(h["R"][MARGIN:MARGIN + h["c_span"]]))
        C = torch.empty((c["batch"], c["M"], c["N"]), device=cuda, dtype=torch.float32)
        ops.mm(A, h["a_strides"], B, h["b_strides"], C, h["c_strides"], c["batch"], c["M"], c["N"], c["K"], bias=bias, R=R,
               epi=c["epi"], alpha=c["alpha"])
        assert g.check(C, require_guarded=True) == 1 and not g.fallthrough
    assert_same_bits(f"mm {c['id']}", C.cpu().numpy(), want)


def test_guarded_linear_bwd_weight(cuda):
    c = next(k for k in WG_EXACT if k["id"] == "m257-o65-k17")
    k = wg_exact_case(c["id"])
    with GA.guarded(cuda) as g:
        dy, x = g.input(torch.from_numpy(k["dy"])), g.input(torch.from_numpy(k["x"]))
        dw, db = ops.linear_bwd_weight(dy, x, wg_desc(c), c["O"], c["K"])
        assert g.check((dw, db), require_guarded=True) == 3 and not g.fallthrough     # dW, db and the workspace
    assert_same_bits("guarded dweight", dw.cpu().numpy(), k["dw"], names=("o", "k"))
    assert_same_bits("guarded dbias", db.cpu().numpy(), k["db"], names=("o",))


def test_guarded_plane_ln(cuda):
    k = ln_case("r17-p257", 1e-5)
    with GA.guarded(cuda) as g:
        x, w, b, dy = (g.input(k[n]) for n in ("x", "w", "b", "dy_int"))
        y, mean, rstd = ops.plane_ln_fwd(x, w, b, 1e-5)
        dx = torch.empty_like(x)
        dw, db = ops.plane_ln_bwd(dy, x, w, mean, rstd, dx=dx, want_params=True)
        assert g.check((y, mean, rstd, dx, dw, db), require_guarded=True) == 7 and not g.fallthrough
    assert_same_bits("guarded plane_ln dbias of integer dy", db.cpu().numpy(), k["db_int"].float().numpy(), names=("p",))
    bad = {}
    within_bar("guarded plane_ln y", y, ln_lib32(k, 1e-5, cuda)["y"], k["y"], bad)
    assert not bad, bad


@pytest.mark.parametrize("alias", [False, True], ids=["out", "in-place"])
def test_guarded_act_bwd(cuda, alias):
    k = act_case(ops.ACT_RELU, 257)
    with GA.guarded(cuda) as g:
        gr, t = g.input(torch.from_numpy(k["g"])), g.input(torch.from_numpy(k["t"]))
        out = ops.act_bwd(ops.ACT_RELU, gr, t, out=gr if alias else None)
        assert g.check(out, require_guarded=True) == (0 if alias else 1) and not g.fallthrough
    assert_same_bits("guarded act_bwd relu n 257", out.cpu().numpy(), k["want"].astype(np.float32), names=("e",))
