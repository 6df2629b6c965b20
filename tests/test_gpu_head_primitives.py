"""-m gpu: the inference primitives of the recogniser head, called directly through their wrappers (ops.transpose2d,
ops.layernorm_cm, ops.fold_layernorm / ops.linear_ln, ops.attn_enc) at the smallest shapes that reach every instantiation,
tile tail and path switch of their launchers (tests/test_head_primitives_host.py recomputes the launchers' selection from
the case tables and asserts that every variant occurs).

Two kinds of comparison, the project's own (tests/test_gpu_train_primitives.py):

A. EXACT.
   * attn_enc, one-hot: the keys of an (image, head) are +-1 codes (T, 64), query i is 48 x the code of key pi(i) (pi a
     random map into the valid keys of the image), V holds integers in [-4, 4].  The kernel scales q by 1/8, so every score
     is an integer: 384 at the matching key, at most 6 g elsewhere, g the largest off-diagonal entry of codes codes^T.  With
     g <= 38 the gap is >= 156 and expf(-156) is exactly 0 in fp32: the probabilities are exactly one-hot and the output is
     V[pi(i)], under np.array_equal.  A kernel that does not subtract the row maximum overflows (exp(384)).
   * attn_enc, uniform: q = 0, so every valid key weighs 1 / n.  One launch of N = T images with valid_len[b] = b + 1 puts
     the mask at every boundary; the output is the mean of the first n columns of V (an exact integer sum, 1 / n and the
     product round once each) to within 2 ulp.
   * transpose2d: bit equality.  layernorm_cm at C = 1: exactly beta.
   In every masked attention case the columns of k and v at or beyond valid_len[b] hold NaN (include/tpspp.h: never used),
   one image has valid_len = T + 5 (means T), and the outputs of the masked QUERIES (finite q) are compared as well.

B. AGAINST FLOAT64 WITH THE PROJECT'S BAR: the relative L2 error against a float64 composition on the CPU is
   <= max(1e-5, 2 x the error of PyTorch's fp32 composition of the same operation on the GPU against the same float64).
   Every measured error is printed with its bar.
   linear_ln's folded formula, var = E[x^2] - mean^2 and Wg^T x - mean colsum in fp32, loses accuracy on the raw values as
   |mean| / std of a column grows: at column offsets r = 16 and 64 it is outside the project's bar, so there the bar is
   2 x the error of an fp32 NumPy restatement of the folded formula (`linear_ln_restated`, on the CPU) against the same
   float64; the factor 2 is the usual margin for a different summation order.  The kernel's, the restatement's and
   PyTorch's errors are all printed.  The restatement also misses the project's bar at K = 2, where two nearly equal
   values cancel in the variance.  The kernel shifts every column by the median of three of its values (rows 0, K / 2 and
   K - 1) before it sums, so it is ALSO held to the project's bar at r = 16 and 64, and with one outlying feature (+64,
   +1000) in any one of the three sampled rows.  With outliers in two sampled rows on the same side the shift is itself an
   outlier and the shifted column has |mean| / std near sqrt(K): there the bar is 2 x the restatement applied to the
   column minus that median, the same construction as above.

The case tables and the reference builders are module-level and need no GPU: the host file imports them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as GA
from test_gpu_attn_train import attention_ref
from test_gpu_train_primitives import assert_same_bits, ints, rel, within_bar
from tps_pp_amd import _lib, ops

pytestmark = pytest.mark.gpu

DK = 64                    # head width
U = 2.0 ** -24             # unit roundoff of fp32


def collect(label, e, bar, bad, extra=""):
    print(f"{label}: rel L2 {e:.3e}, bar {bar:.3e}{extra}")
    if not e <= bar:
        bad[label] = (e, bar)


# ---- the launchers' selection, restated (tps_pp_amd/csrc/tpspp_head.hip, tpspp_conv.hip) -----------------------------------
def attn_path(T):
    """The kernel tpspp_attn_enc_fwd launches: attn_enc_mfma_kernel<NJ> for T <= 128, else the LDS kernel."""
    return "lds" if T > 128 else f"nj{(T + 31) // 32}"


def attn_wavefronts(N, H, T):
    """Wavefronts of the matrix-core kernel (four to a workgroup)."""
    return N * H * ((T + 31) // 32)


def layernorm_vpt(C):
    """Values per thread of the layernorm_cm_kernel instantiation launched for C features."""
    return 8 if C <= 128 else 32 if C <= 512 else 64


def linear_ln_paths(K, M, Cout):
    """-> (wavefronts that split K, the set of {"fast", "slow"} branches some wavefront of some workgroup takes).
    A wavefront takes the unrolled branch iff its k-slice holds exactly 32 values and its workgroup's tile is full.  The
    token-major launch swaps the grid's axes and the operands: the tile count and both conditions are the same."""
    gx, gy = -(-M // 32), -(-Cout // 32)
    nw = 4 if K < 256 else 8 if gx * gy > 512 else 16
    kw = -(-K // (2 * nw)) * 2
    full_tile, tail_tile = M >= 32 and Cout >= 32, bool(M % 32 or Cout % 32)
    taken = set()
    for wv in range(nw):
        k_lo = wv * kw
        k_hi = min(K, k_lo + kw)
        nit = (k_hi - k_lo + 1) >> 1
        if nit <= 0:
            continue
        unrolled = nit == 16 and k_lo + 32 <= K
        if unrolled and full_tile:
            taken.add("fast")
        if not unrolled or tail_tile:
            taken.add("slow")
    return nw, taken


# ---- layouts -----------------------------------------------------------------------------------------------------------------
def to_cm(x):
    """(N, T, C) -> the head's channel-major (C, N * T); NumPy or torch."""
    n, t, c = x.shape
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x.transpose(2, 0, 1).reshape(c, n * t))
    return x.permute(2, 0, 1).reshape(c, n * t).contiguous()


def from_cm(x, N, T):
    """(C, N * T) -> (N, T, C)."""
    c = x.shape[0]
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x.reshape(c, N, T).transpose(1, 2, 0))
    return x.reshape(c, N, T).permute(1, 2, 0).contiguous()


def pack_qkv(q, k, v):
    """Three (N, T, C) -> qkv (3C, N * T): rows [0, C) = q, [C, 2C) = k, [2C, 3C) = v."""
    if isinstance(q, np.ndarray):
        return np.concatenate([to_cm(q), to_cm(k), to_cm(v)], 0)
    return torch.cat([to_cm(q), to_cm(k), to_cm(v)], 0)


def ragged(T):
    """valid_len of a masked case: one image beyond T (means T), one inside, one of a single key."""
    return [T + 5, max(1, (2 * T) // 3), 1]


def poisoned(x, valid_len):
    """Copy of (N, T, C) with the tokens at or beyond valid_len[b] set to NaN."""
    out = x.copy() if isinstance(x, np.ndarray) else x.clone()
    for b, n in enumerate(valid_len):
        out[b, n:] = float("nan")
    return out


def attn_ref_cm(qkv, N, T, valid_len=None):
    """attention_ref of tests/test_gpu_attn_train.py in this entry point's layout: qkv (3C, N * T) -> (C, N * T), in the
    dtype and on the device of qkv."""
    C = qkv.shape[0] // 3
    q, k, v = (from_cm(qkv[i * C:(i + 1) * C], N, T) for i in range(3))
    vl = None if valid_len is None else [min(int(n), T) for n in valid_len]
    return to_cm(attention_ref(q, k, v, C // DK, vl)[0])


# ---- attn_enc: the exact cases ---------------------------------------------------------------------------------------------
ATTN_T = (1, 32, 33, 64, 65, 96, 97, 128, 129, 256)
# (T, N, heads): C = 64 and C = 128 alternate, so each of NJ = 1..4 and the LDS kernel sees both; N * heads * ceil(T / 32)
# is no multiple of 4 at T = 1, 33, 65 and 96 (a last workgroup with fewer than four live wavefronts: NJ = 1, 2, 3 -- with
# NJ = 4 the count is always a multiple of 4)
ONEHOT_CASES = tuple(dict(id=f"t{T}-n3-h{1 + i % 2}", T=T, N=3, H=1 + i % 2) for i, T in enumerate(ATTN_T))
UNIFORM_CASES = (dict(id="t33-h1", T=33, H=1), dict(id="t96-h2", T=96, H=2), dict(id="t129-h1", T=129, H=1))
GRAM_LIMIT = 38
MATCH = 384                # the matching score: 6 * 64


@functools.lru_cache(maxsize=None)
def onehot_case(cid, masked):
    c = next(k for k in ONEHOT_CASES if k["id"] == cid)
    T, N, H = c["T"], c["N"], c["H"]
    rng = np.random.default_rng(7000 + 2 * T + int(masked))
    vl = ragged(T) if masked else None
    nv = [min(n, T) for n in vl] if masked else [T] * N
    codes = rng.choice(np.float32([-1.0, 1.0]), size=(N, T, H, DK))       # a different draw per image and head
    pi = np.stack([rng.integers(0, nv[b], size=(T, H)) for b in range(N)])
    v = ints(rng, (N, T, H, DK), 4)
    bi, hi = np.arange(N)[:, None, None], np.arange(H)[None, None, :]
    q = np.float32(48.0) * codes[bi, pi, hi]
    want = v[bi, pi, hi].reshape(N, T, H * DK)
    g = max(int((codes[b, :nv[b], h] @ codes[b, :nv[b], h].T - DK * np.eye(nv[b])).max())
            for b in range(N) for h in range(H)) if T > 1 else 0
    k3, v3, q3 = (a.reshape(N, T, H * DK) for a in (codes, v, q))
    clean = pack_qkv(q3, k3, v3)
    qkv = pack_qkv(q3, poisoned(k3, nv), poisoned(v3, nv)) if masked else clean
    return dict(T=T, N=N, H=H, valid_len=vl, nvalid=nv, qkv=qkv, clean=clean, want=to_cm(want), gram=g, pi=pi)


@functools.lru_cache(maxsize=None)
def uniform_case(cid):
    c = next(k for k in UNIFORM_CASES if k["id"] == cid)
    T, H = c["T"], c["H"]
    N = T
    rng = np.random.default_rng(7500 + T)
    vl = list(range(1, T + 1))
    vl[-1] = T + 5
    nv = [min(n, T) for n in vl]
    k = rng.choice(np.float32([-1.0, 1.0]), size=(N, T, H * DK))
    v = ints(rng, (N, T, H * DK), 4)
    q = np.zeros((N, T, H * DK), np.float32)
    mean = np.stack([v[b, :nv[b]].astype(np.float64).sum(0) / nv[b] for b in range(N)])       # (N, C)
    want = np.broadcast_to(mean[:, None, :], (N, T, H * DK))
    return dict(T=T, N=N, H=H, valid_len=vl, nvalid=nv, qkv=pack_qkv(q, poisoned(k, nv), poisoned(v, nv)),
                clean=pack_qkv(q, k, v), want=to_cm(np.ascontiguousarray(want)))


def explain_attn(label, got, want, N, T, nvalid, tol=None):
    """None if (C, N * T) `got` equals `want` (within `tol`, an array, if given), else a message naming the first wrong
    (image, head, query, feature), the query's key tile and whether the query itself is masked."""
    if tol is None:
        wrong = ~(got == want)
    else:
        wrong = ~(np.abs(got.astype(np.float64) - want) <= tol)
    if not wrong.any():
        return None
    r, m = (int(x) for x in np.argwhere(wrong)[0])
    b, i = divmod(m, T)
    return (f"{label}: {int(wrong.sum())} of {wrong.size} outputs differ, the first at image {b} (valid_len {nvalid[b]}), "
            f"head {r // DK}, query {i} ({'masked' if i >= nvalid[b] else 'valid'}, query block {i // 32}), feature "
            f"{r % DK}: got {got[r, m]!r}, want {want[r, m]!r}; path {attn_path(T)}")


# ---- attn_enc: comparison B ------------------------------------------------------------------------------------------------
ATTN_B_T = (20, 65, 96, 128, 129, 255)
ATTN_B_SCALES = (1.0, 4.0)
ATTN_B_N, ATTN_B_H = 3, 2


@functools.lru_cache(maxsize=None)
def attn_b_case(T, scale, masked):
    g = torch.Generator().manual_seed(8000 + 4 * T + int(scale) + 2 * int(masked))
    N, C = ATTN_B_N, DK * ATTN_B_H
    q, k, v = (scale * torch.randn((N, T, C), generator=g) for _ in range(3))
    vl = ragged(T) if masked else None
    nv = [min(n, T) for n in vl] if masked else [T] * N
    clean = pack_qkv(q, k, v)
    qkv = pack_qkv(q, poisoned(k, nv), poisoned(v, nv)) if masked else clean
    return dict(T=T, N=N, valid_len=vl, nvalid=nv, qkv=qkv, clean=clean, want=attn_ref_cm(clean.double(), N, T, vl))


# ---- layernorm_cm ---------------------------------------------------------------------------------------------------------
LNCM_SHAPES = ((1, 5), (2, 16), (100, 1), (128, 17), (129, 33), (512, 16), (513, 15), (1000, 40), (1024, 3))
LNCM_OFFSETS = (0.0, 16.0, 100.0)
LNCM_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def lncm_case(C, M, r):
    g = torch.Generator().manual_seed(9000 + 7 * C + M + int(r))
    x = torch.randn((C, M), generator=g) + r
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    y = F.layer_norm(x.double().t(), (C,), ga.double(), be.double(), LNCM_EPS).t().contiguous()
    return dict(x=x, gamma=ga, beta=be, y=y)


# ---- transpose2d ----------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = ((1, 1), (1, 70), (33, 31), (32, 32), (65, 97))
TRANSPOSE_SPECIALS = (-0.0, float("inf"), float("-inf"), 1e-45, -3.0e38)


def transpose_case(rows, cols):
    rng = np.random.default_rng(9500 + 101 * rows + cols)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    flat = x.reshape(-1)
    at = rng.permutation(flat.size)[:len(TRANSPOSE_SPECIALS)]
    flat[at] = np.float32(TRANSPOSE_SPECIALS[:at.size])
    return x


# ---- linear_ln ------------------------------------------------------------------------------------------------------------
# (K, M, Cout), with what the channel-major launch reaches (the token-major launch swaps the roles of M and Cout in the grid
# and reaches the same wavefront count and branches: tests/test_head_primitives_host.py)
LINEAR_LN_SHAPES = (
    (128, 64, 64),         # 4 wavefronts, fast path
    (127, 33, 40),         # 4: three wavefronts fast, the last slow; odd K; both tile tails
    (1, 3, 5),             # 4: tiny K
    (2, 32, 32),
    (255, 40, 96),         # 4: two trips of the slow loop
    (512, 64, 64),         # 16 wavefronts, fast path
    (256, 33, 92),         # 16: slow path
    (513, 40, 64),
    (256, 545, 929),       # 8 wavefronts (more than 512 tiles): fast path away from the tails
    (512, 545, 929),       # 8: slow path
    (256, 512, 1024),      # exactly 512 tiles: still 16 wavefronts
)
LINEAR_LN_BAR_OFFSETS = (0.0, 1.0, 4.0)         # the project's bar
LINEAR_LN_FAR_OFFSETS = (16.0, 64.0)            # 2 x the restatement's error, and the project's bar as well
LINEAR_LN_OUTLIER_SHAPES = ((512, 64, 64), (128, 64, 64), (513, 40, 64))      # unrolled (16 and 4 wavefronts), guarded
LINEAR_LN_OUTLIER_AMOUNTS = (64.0, 1000.0)
LINEAR_LN_CONSTS = (0.5, 8.0)
LINEAR_LN_EPS = 1e-5


def gelu32(z):
    """GELU (erf form) of an fp32 NumPy array, in fp32."""
    t = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
    return (0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))).numpy()


def linear_ln_restated(x, folded, eps):
    """The folded formula of include/tpspp.h on the raw values, in fp32 NumPy -> (M, Cout) before the epilogue: fp32 sums of
    x and x^2 per column (NumPy's blocked summation along the contiguous axis: a split sum like the kernel's), max(E[x^2] -
    mean^2, 0), rstd (Wg^T x - mean colsum) + bias_eff."""
    wg, colsum, bias_eff = (np.asarray(t, np.float32) for t in folded)
    xt = np.ascontiguousarray(np.asarray(x, np.float32).T)              # (M, K)
    K = np.float32(xt.shape[1])
    s1 = xt.sum(1, dtype=np.float32)
    s2 = (xt * xt).sum(1, dtype=np.float32)
    mean = s1 / K
    var = np.maximum(s2 / K - mean * mean, np.float32(0.0))
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    acc = xt @ wg                                                        # (M, Cout) fp32
    return rstd[:, None] * (acc - mean[:, None] * colsum[None, :]) + bias_eff[None, :]


def sampled_rows(K):
    """The three rows whose median shifts a column in the kernel."""
    return (0, K // 2, K - 1)


def outlier_cases(K):
    """(label, rows, project bar?) x amounts: one outlying feature in each sampled row alone and in a row that is not
    sampled (the project's bar), and in two sampled rows at once (the bar of the shifted restatement)."""
    lo, mid, hi = sampled_rows(K)
    kinds = (("row 0", (lo,), True), ("row K/2", (mid,), True), ("row K-1", (hi,), True), ("row 1", (1,), True),
             ("rows 0 and K-1", (lo, hi), False))
    return [(f"{name} + {a:g}", (rows, a), strict) for name, rows, strict in kinds for a in LINEAR_LN_OUTLIER_AMOUNTS]


def med3_shifted(x):
    """x (K, M) fp32 minus the median of rows 0, K / 2 and K - 1 of each column, in fp32: what the kernel sums."""
    x = np.asarray(x, np.float32)
    return x - np.median(x[list(sampled_rows(x.shape[0]))], axis=0)[None, :]


@functools.lru_cache(maxsize=8)
def linear_ln_case(K, M, Co, r, const=None, outlier=None):
    """One set of operands and the float64 results of both layouts.  `const`: the last column of x holds that constant;
    `outlier` = (rows, amount): that amount is added to those features of every column."""
    g = torch.Generator().manual_seed(10000 + K + 3 * M + 5 * Co + int(r))
    x = torch.randn((K, M), generator=g) + r
    if const is not None:
        x[:, M - 1] = const
    if outlier is not None:
        x[list(outlier[0])] += outlier[1]
    ga, be = torch.randn(K, generator=g), torch.randn(K, generator=g)
    w, b = torch.randn((Co, K), generator=g) / K ** 0.5, torch.randn(Co, generator=g)
    res = torch.randn((Co, M), generator=g)
    folded = ops.fold_layernorm(ga, be, w.t().contiguous(), b)           # CPU fp32: what kernel and restatement both take
    z = F.layer_norm(x.double().t(), (K,), ga.double(), be.double(), LINEAR_LN_EPS) @ w.double().t() + b.double()
    z32 = linear_ln_restated(x.numpy(), [t.numpy() for t in folded], LINEAR_LN_EPS)
    k = dict(x=x, gamma=ga, beta=be, w=w, b=b, res=res, folded=folded,
             tm=z.contiguous(), cm=(F.gelu(z).t() + res.double()).contiguous(),
             tm_restated=torch.from_numpy(z32), cm_restated=torch.from_numpy(gelu32(z32).T + res.numpy()))
    if outlier is not None:                      # the same formula on the column as the kernel shifts it
        s32 = linear_ln_restated(med3_shifted(x.numpy()), [t.numpy() for t in folded], LINEAR_LN_EPS)
        k.update(tm_shifted=torch.from_numpy(s32), cm_shifted=torch.from_numpy(gelu32(s32).T + res.numpy()))
    return k


def linear_ln_lib32(k, token_major, dev):
    """PyTorch's fp32 composition of the same operation on `dev`."""
    x, ga, be, w, b, res = (k[n].to(dev) for n in ("x", "gamma", "beta", "w", "b", "res"))
    z = F.layer_norm(x.t(), (x.shape[0],), ga, be, LINEAR_LN_EPS) @ w.t() + b
    return z if token_major else F.gelu(z).t() + res


def linear_ln_run(k, token_major, dev, act=2, residual=True):
    folded = [t.to(dev) for t in k["folded"]]
    if token_major:
        return ops.linear_ln(k["x"].to(dev), folded, LINEAR_LN_EPS, token_major=True)
    return ops.linear_ln(k["x"].to(dev), folded, LINEAR_LN_EPS, act=act, residual=k["res"].to(dev) if residual else None)


def const_column_bound(k, c, eps=LINEAR_LN_EPS):
    """Per output feature: rstd 2 gamma_(K+2) |c| sum_k |w_gamma[k, o]|, rstd = 1 / sqrt(eps): the forward bound of the two
    K-term sums (w_gamma^T x and mean colsum) that cancel on a constant column."""
    K = k["x"].shape[0]
    n = K + 2
    gamma_n = n * U / (1.0 - n * U)
    return (2.0 * gamma_n * abs(c) / eps ** 0.5) * k["folded"][0].double().abs().sum(0)


# =============================================================================================================================
# attn_enc
# =============================================================================================================================
def _run_attn(k, dev, qkv=None):
    vl = None if k["valid_len"] is None else torch.tensor(k["valid_len"], dtype=torch.int32, device=dev)
    qkv = k["qkv"] if qkv is None else qkv
    qkv = torch.from_numpy(qkv) if isinstance(qkv, np.ndarray) else qkv
    return ops.attn_enc(qkv.to(dev), k["N"], k["T"], vl)


# (case id, masked): at T = 1 ragged() masks nothing and poisons nothing -- that case holds valid_len > T alone
ONEHOT_PARAMS = [pytest.param(c["id"], m, id=f"{c['id']}-{('masked-poisoned' if c['T'] > 1 else 'valid-len-above-t') if m else 'full'}")
                 for c in ONEHOT_CASES for m in (False, True)]


@pytest.mark.parametrize("cid,masked", ONEHOT_PARAMS)
def test_attn_onehot_is_exact(cuda, cid, masked):
    k = onehot_case(cid, masked)
    assert k["gram"] <= GRAM_LIMIT
    got = _run_attn(k, cuda).cpu().numpy()
    msg = explain_attn(f"one-hot {cid}", got, k["want"], k["N"], k["T"], k["nvalid"])
    assert msg is None, msg


@pytest.mark.parametrize("cid", [c["id"] for c in UNIFORM_CASES])
def test_attn_uniform_mean_at_every_mask_boundary(cuda, cid):
    k = uniform_case(cid)
    got = _run_attn(k, cuda).cpu().numpy()
    tol = 2.0 * np.spacing(np.abs(k["want"]).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - k["want"]) / (tol / 2.0)
    print(f"uniform {cid}: largest error {np.nanmax(err):.3f} ulp, bar 2 ulp")
    msg = explain_attn(f"uniform {cid}", got, k["want"], k["N"], k["T"], k["nvalid"], tol)
    assert msg is None, msg


@pytest.mark.parametrize("masked", [False, True], ids=["full", "ragged-poisoned"])
@pytest.mark.parametrize("scale", ATTN_B_SCALES)
@pytest.mark.parametrize("T", ATTN_B_T)
def test_attn_against_float64(cuda, T, scale, masked):
    k = attn_b_case(T, scale, masked)
    got = _run_attn(k, cuda)
    lib32 = attn_ref_cm(k["clean"].to(cuda), k["N"], T, k["valid_len"])
    bad = {}
    within_bar(f"attn_enc T {T} scale {scale:g} {'ragged' if masked else 'full'} ({attn_path(T)})", got, lib32, k["want"],
               bad)
    assert not bad, bad


# =============================================================================================================================
# layernorm_cm, transpose2d
# =============================================================================================================================
@pytest.mark.parametrize("C,M", LNCM_SHAPES)
def test_layernorm_cm_against_float64(cuda, C, M):
    bad = {}
    for r in LNCM_OFFSETS:
        k = lncm_case(C, M, r)
        x, ga, be = (k[n].to(cuda) for n in ("x", "gamma", "beta"))
        got = ops.layernorm_cm(x, ga, be, LNCM_EPS)
        lib32 = F.layer_norm(x.t(), (C,), ga, be, LNCM_EPS).t()
        within_bar(f"layernorm_cm C {C} M {M} offset {r:g} (VPT {layernorm_vpt(C)})", got, lib32, k["y"], bad)
        if C == 1:
            assert_same_bits(f"layernorm_cm C 1 offset {r:g}: beta", got.cpu().numpy(),
                             k["beta"][:, None].expand(1, M).contiguous().numpy(), names=("c", "m"))
    assert not bad, bad


def test_layernorm_cm_refuses_more_than_1024_features(cuda):
    x = torch.zeros((1025, 3), device=cuda)
    ga = torch.ones(1025, device=cuda)
    with pytest.raises(_lib.TpsppError, match="at most 1024 features"):
        ops.layernorm_cm(x, ga, ga, LNCM_EPS)


@pytest.mark.parametrize("rows,cols", TRANSPOSE_SHAPES)
def test_transpose2d_is_a_copy(cuda, rows, cols):
    x = transpose_case(rows, cols)
    got = ops.transpose2d(torch.from_numpy(x).to(cuda)).cpu().numpy()
    assert_same_bits(f"transpose2d ({rows}, {cols})", got, np.ascontiguousarray(x.T), names=("c", "r"))


# =============================================================================================================================
# linear_ln
# =============================================================================================================================
LAYOUT_IDS = {False: "channel-major", True: "token-major"}


@pytest.mark.parametrize("token_major", [False, True], ids=list(LAYOUT_IDS.values()))
@pytest.mark.parametrize("K,M,Co", LINEAR_LN_SHAPES)
def test_linear_ln_against_float64(cuda, K, M, Co, token_major):
    nw, taken = linear_ln_paths(K, M, Co)
    name = "tm" if token_major else "cm"
    bad = {}
    for r in LINEAR_LN_BAR_OFFSETS + LINEAR_LN_FAR_OFFSETS:
        k = linear_ln_case(K, M, Co, r)
        want = k[name]
        got = linear_ln_run(k, token_major, cuda)
        lib32 = linear_ln_lib32(k, token_major, cuda)
        label = (f"linear_ln K {K} M {M} Cout {Co} {LAYOUT_IDS[token_major]} offset {r:g} ({nw} wavefronts, "
                 f"{'+'.join(sorted(taken))})")
        assert torch.isfinite(got).all(), f"{label}: not finite"
        e_restated, e_lib = rel(k[name + "_restated"], want), rel(lib32, want)
        extra = f"; restated {e_restated:.3e}, PyTorch fp32 {e_lib:.3e}"
        collect(label, rel(got, want), max(1e-5, 2 * e_lib), bad, extra)
        if r in LINEAR_LN_FAR_OFFSETS:
            collect(label + " against the restatement", rel(got, want), 2 * e_restated, bad)
    assert not bad, bad


@pytest.mark.parametrize("token_major", [False, True], ids=list(LAYOUT_IDS.values()))
@pytest.mark.parametrize("K,M,Co", LINEAR_LN_OUTLIER_SHAPES)
def test_linear_ln_outlying_features(cuda, K, M, Co, token_major):
    """One feature far from the rest of its column, in each row the kernel's shift samples: the project's bar.  Two sampled
    rows at once: the shift is an outlier, and the bar is 2 x the restatement on the column as shifted."""
    name = "tm" if token_major else "cm"
    bad = {}
    for what, outlier, strict in outlier_cases(K):
        k = linear_ln_case(K, M, Co, 0.0, None, outlier)
        want = k[name]
        got = linear_ln_run(k, token_major, cuda)
        label = f"linear_ln K {K} M {M} Cout {Co} {LAYOUT_IDS[token_major]} outlier {what}"
        assert torch.isfinite(got).all(), f"{label}: not finite"
        e_raw, e_shifted = rel(k[name + "_restated"], want), rel(k[name + "_shifted"], want)
        e_lib = rel(linear_ln_lib32(k, token_major, cuda), want)
        extra = f"; restated on raw values {e_raw:.3e}, as shifted {e_shifted:.3e}, PyTorch fp32 {e_lib:.3e}"
        collect(label, rel(got, want), max(1e-5, 2 * e_lib) if strict else 2 * e_shifted, bad, extra)
    assert not bad, bad


@pytest.mark.parametrize("token_major", [False, True], ids=list(LAYOUT_IDS.values()))
@pytest.mark.parametrize("K,M,Co", LINEAR_LN_SHAPES)
def test_linear_ln_constant_column(cuda, K, M, Co, token_major):
    """A column of x that is a constant c has variance 0: rstd = 1 / sqrt(eps) multiplies whatever the two K-term sums that
    cancel leave behind.  Before the activation (act 0, no residual) the column must be bias_eff to within the forward bound
    of those sums on the raw values (the kernel, which sums the column minus its first value, leaves nothing)."""
    for c in LINEAR_LN_CONSTS:
        k = linear_ln_case(K, M, Co, 0.0, c)
        got = linear_ln_run(k, token_major, cuda, act=0, residual=False).cpu().double()
        col = got[M - 1] if token_major else got[:, M - 1]
        assert torch.isfinite(col).all(), f"constant {c}: the column is not finite"
        err, bound = (col - k["folded"][2].double()).abs(), const_column_bound(k, c)
        worst = int((err / bound).argmax())
        print(f"linear_ln K {K} M {M} Cout {Co} {LAYOUT_IDS[token_major]} constant {c:g}: largest |out - bias_eff| / bound "
              f"{float(err[worst] / bound[worst]):.3e} (|out - bias_eff| {float(err[worst]):.3e}, bound "
              f"{float(bound[worst]):.3e})")
        assert bool((err <= bound).all()), (f"constant {c}: output feature {worst}: |out - bias_eff| "
                                            f"{float(err[worst]):.3e} above the bound {float(bound[worst]):.3e}")


def test_linear_ln_refusals(cuda):
    k = linear_ln_case(2, 32, 32, 0.0)
    x, res = k["x"].to(cuda), k["res"].to(cuda)
    folded = [t.to(cuda) for t in k["folded"]]
    with pytest.raises(_lib.TpsppError, match="token-major form takes no activation"):
        ops.linear_ln(x, folded, LINEAR_LN_EPS, act=2, token_major=True)
    with pytest.raises(_lib.TpsppError, match="token-major form takes no activation"):
        ops.linear_ln(x, folded, LINEAR_LN_EPS, residual=res.t().contiguous(), token_major=True)
    with pytest.raises(_lib.TpsppError, match="bad sizes / activation"):
        ops.linear_ln(x, folded, LINEAR_LN_EPS, act=3)


# =============================================================================================================================
# guard bands: one case per entry point at its tail-heaviest shape
# =============================================================================================================================
def test_guarded_transpose2d(cuda):
    x = transpose_case(65, 97)
    with GA.guarded(cuda) as g:
        out = ops.transpose2d(g.input(torch.from_numpy(x)))
        assert g.check(out, require_guarded=True) == 1 and not g.fallthrough
    assert_same_bits("guarded transpose2d (65, 97)", out.cpu().numpy(), np.ascontiguousarray(x.T), names=("c", "r"))


def test_guarded_layernorm_cm(cuda):
    C, M = 129, 33
    k = lncm_case(C, M, 0.0)
    with GA.guarded(cuda) as g:
        x, ga, be = (g.input(k[n]) for n in ("x", "gamma", "beta"))
        y = ops.layernorm_cm(x, ga, be, LNCM_EPS)
        assert g.check(y, require_guarded=True) == 1 and not g.fallthrough
    bad = {}
    within_bar("guarded layernorm_cm C 129 M 33", y, F.layer_norm(x.t(), (C,), ga, be, LNCM_EPS).t(), k["y"], bad)
    assert not bad, bad


@pytest.mark.parametrize("token_major", [False, True], ids=list(LAYOUT_IDS.values()))
def test_guarded_linear_ln(cuda, token_major):
    k = linear_ln_case(127, 33, 40, 0.0)
    with GA.guarded(cuda) as g:
        x, res = g.input(k["x"]), g.input(k["res"])
        folded = [g.input(t) for t in k["folded"]]
        if token_major:
            out = ops.linear_ln(x, folded, LINEAR_LN_EPS, token_major=True)
        else:
            out = ops.linear_ln(x, folded, LINEAR_LN_EPS, act=2, residual=res)
        assert g.check(out, require_guarded=True) == 1 and not g.fallthrough
    bad = {}
    within_bar(f"guarded linear_ln (127, 33, 40) {LAYOUT_IDS[token_major]}", out, linear_ln_lib32(k, token_major, cuda),
               k["tm" if token_major else "cm"], bad)
    assert not bad, bad


@pytest.mark.parametrize("cid", ["t33-n3-h1", "t129-n3-h1"])
def test_guarded_attn_enc(cuda, cid):
    k = onehot_case(cid, True)
    with GA.guarded(cuda) as g:
        qkv = g.input(torch.from_numpy(k["qkv"]))
        vl = g.input(torch.tensor(k["valid_len"], dtype=torch.int32))
        out = ops.attn_enc(qkv, k["N"], k["T"], vl)
        assert g.check(out, require_guarded=True) == 1 and not g.fallthrough
    msg = explain_attn(f"guarded one-hot {cid}", out.cpu().numpy(), k["want"], k["N"], k["T"], k["nvalid"])
    assert msg is None, msg
