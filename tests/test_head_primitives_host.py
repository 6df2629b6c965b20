"""CPU checks that tests/test_gpu_head_primitives.py is itself sound: the Gram condition and the magnitudes that make its
exact cases exact (an fp32 NumPy emulation of the attention reproduces them bit for bit), every float64 builder against
PyTorch's float64 composition, the need for the second linear_ln bar, the argument refusals that return before a launch,
and that its case tables reach every kernel instantiation and branch the launchers can select.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tps_pp_amd import _lib, build
import test_gpu_head_primitives as HP

EXACT = float(2 ** 24)
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def _is_int(a):
    a = np.asarray(a, np.float64)
    return bool(np.isfinite(a).all() and (a == np.round(a)).all())


def attn_emulated32(qkv, N, T, valid_len):
    """The attention in fp32 NumPy, operation by operation as both kernels perform it (q / 8, scores, row maximum over the
    valid keys, expf, sum, weighted values over the valid keys only, times 1 / sum).  qkv (3C, N * T) -> (C, N * T)."""
    C = qkv.shape[0] // 3
    q, k, v = (HP.from_cm(qkv[i * C:(i + 1) * C], N, T) for i in range(3))
    out = np.zeros((N, T, C), np.float32)
    for b in range(N):
        n = T if valid_len is None else min(valid_len[b], T)
        for h in range(C // HP.DK):
            f = slice(HP.DK * h, HP.DK * (h + 1))
            s = (q[b, :, f] * np.float32(0.125)) @ k[b, :n, f].T
            p = np.exp(s - s.max(1, keepdims=True), dtype=np.float32)
            out[b, :, f] = (p @ v[b, :n, f]) * (np.float32(1.0) / p.sum(1, dtype=np.float32, keepdims=True))
    return HP.to_cm(out)


def attention64(qkv, N, T, valid_len):
    """PyTorch's float64 composition written directly on the (3C, N * T) layout (no attention_ref, no to_cm / from_cm)."""
    C = qkv.shape[0] // 3
    H = C // HP.DK
    q, k, v = (qkv[i * C:(i + 1) * C].double().view(H, HP.DK, N, T) for i in range(3))
    a = torch.einsum("hdbi,hdbj->bhij", q, k) / 8.0
    if valid_len is not None:
        vl = torch.tensor([min(n, T) for n in valid_len])
        a = a.masked_fill(~(torch.arange(T)[None, :] < vl[:, None])[:, None, None, :], float("-inf"))
    return torch.einsum("bhij,hdbj->hdbi", F.softmax(a, -1), v).reshape(C, N * T)


# ---- the exact attention cases ------------------------------------------------------------------------------------------------
def test_exp_magnitudes():
    gap = (HP.DK - HP.GRAM_LIMIT) * 6
    assert gap == 156 and HP.MATCH == 6 * HP.DK == 384
    assert np.exp(np.float32(-gap)) == 0 and np.exp(np.float32(0.0)) == 1           # exactly one-hot
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(HP.MATCH)))                                # no row maximum: overflow
    assert np.float32(48.0) * np.float32(0.125) == 6 and HP.MATCH < EXACT


@pytest.mark.parametrize("cid,masked", HP.ONEHOT_PARAMS)
def test_onehot_case_is_sound(cid, masked):
    k = HP.onehot_case(cid, masked)
    T, N, H = k["T"], k["N"], k["H"]
    C = H * HP.DK
    assert k["gram"] <= HP.GRAM_LIMIT, "the Gram condition fails for this seed"
    q, kk, v = (HP.from_cm(k["clean"][i * C:(i + 1) * C], N, T) for i in range(3))
    assert set(np.unique(kk)) <= {-1.0, 1.0} and set(np.unique(q)) <= {-48.0, 48.0}
    assert _is_int(v) and np.abs(v).max() <= 4
    assert (k["pi"] < np.asarray(k["nvalid"])[:, None, None]).all() and k["pi"].min() >= 0
    # the scores the kernel forms: integers, 384 at pi(i), lower by at least 156 at every other valid key
    for b in range(N):
        n = k["nvalid"][b]
        for h in range(H):
            f = slice(HP.DK * h, HP.DK * (h + 1))
            s = (q[b, :, f].astype(np.float64) / 8.0) @ kk[b, :n, f].astype(np.float64).T          # (T, n)
            assert _is_int(s) and np.array_equal(s.argmax(1), k["pi"][b, :, h])
            top = s[np.arange(T), k["pi"][b, :, h]]
            assert (top == HP.MATCH).all()
            s[np.arange(T), k["pi"][b, :, h]] = -np.inf
            assert n == 1 or s.max() <= HP.MATCH - 156
    # the poison: NaN exactly in the k and v columns at or beyond valid_len, q finite everywhere
    qkv = k["qkv"]
    assert np.isfinite(qkv[:C]).all()
    if masked:
        assert k["valid_len"][0] == T + 5 and k["nvalid"] == [T, max(1, 2 * T // 3), 1]
        assert bool(np.isnan(qkv).any()) == (T > 1)               # T = 1 masks nothing: its id says so
        nan_kv = np.isnan(HP.from_cm(qkv[C:2 * C], N, T)).all(2) & np.isnan(HP.from_cm(qkv[2 * C:], N, T)).all(2)
        fin_kv = np.isfinite(HP.from_cm(qkv[C:2 * C], N, T)).all(2) & np.isfinite(HP.from_cm(qkv[2 * C:], N, T)).all(2)
        beyond = np.arange(T)[None, :] >= np.asarray(k["nvalid"])[:, None]
        assert np.array_equal(nan_kv, beyond) and np.array_equal(fin_kv, ~beyond)
        assert np.array_equal(qkv[~np.isnan(qkv)], k["clean"][~np.isnan(qkv)])
    else:
        assert k["valid_len"] is None and np.array_equal(qkv, k["clean"])
    # an fp32 emulation is exact, and the float64 builder agrees
    assert np.array_equal(attn_emulated32(k["clean"], N, T, k["valid_len"]), k["want"])
    ref = HP.attn_ref_cm(torch.from_numpy(k["clean"]).double(), N, T, k["valid_len"])
    assert torch.allclose(ref, torch.from_numpy(k["want"]).double(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("cid", [c["id"] for c in HP.UNIFORM_CASES])
def test_uniform_case_is_sound(cid):
    k = HP.uniform_case(cid)
    T, N, H = k["T"], k["N"], k["H"]
    C = H * HP.DK
    assert N == T and k["nvalid"] == list(range(1, T + 1)) and k["valid_len"][-1] == T + 5
    assert not k["clean"][:C].any() and np.isfinite(k["qkv"][:C]).all()
    v = HP.from_cm(k["clean"][2 * C:], N, T)
    assert _is_int(v) and np.abs(v).max() <= 4 and 4 * T < EXACT
    beyond = np.arange(T)[None, :] >= np.asarray(k["nvalid"])[:, None]
    for third in (1, 2):
        assert np.array_equal(np.isnan(HP.from_cm(k["qkv"][third * C:(third + 1) * C], N, T)).all(2), beyond)
        assert np.array_equal(np.isnan(HP.from_cm(k["qkv"][third * C:(third + 1) * C], N, T)).any(2), beyond)
    ref = HP.attn_ref_cm(torch.from_numpy(k["clean"]).double(), N, T, k["valid_len"])
    assert torch.allclose(ref, torch.from_numpy(k["want"]), rtol=1e-13, atol=1e-13)
    # the emulation (1 / n and the product round once each) stays within the test's 2 ulp
    got = attn_emulated32(k["clean"], N, T, k["valid_len"]).astype(np.float64)
    ulp = np.spacing(np.abs(k["want"]).astype(np.float32)).astype(np.float64)
    print(f"uniform {cid}: the fp32 emulation is within {(np.abs(got - k['want']) / ulp).max():.3f} ulp")
    assert (np.abs(got - k["want"]) <= 2.0 * ulp).all()


def test_attn_builder_is_pytorchs_float64_composition():
    for T, scale, masked in ((20, 1.0, True), (65, 4.0, False), (129, 4.0, True)):
        k = HP.attn_b_case(T, scale, masked)
        want = attention64(k["clean"], k["N"], T, k["valid_len"])
        assert torch.allclose(k["want"], want, rtol=1e-12, atol=1e-12)
        assert k["want"].dtype == torch.float64 and torch.isfinite(k["want"]).all()
        if masked:
            assert k["valid_len"] == HP.ragged(T) and 1 in k["valid_len"] and T + 5 in k["valid_len"]
            assert int(torch.isnan(k["qkv"]).sum()) == 2 * k["clean"].shape[0] // 3 * sum(T - n for n in k["nvalid"])
            assert torch.isfinite(k["qkv"][:k["qkv"].shape[0] // 3]).all()
    assert HP.ATTN_B_T == (20, 65, 96, 128, 129, 255) and HP.ATTN_B_SCALES == (1.0, 4.0)


def test_attn_report_names_the_query():
    k = HP.onehot_case("t33-n3-h1", True)
    got = k["want"].copy()
    assert HP.explain_attn("x", got, k["want"], 3, 33, k["nvalid"]) is None
    got[5, 2 * 33 + 32] = np.nan
    msg = HP.explain_attn("x", got, k["want"], 3, 33, k["nvalid"])
    assert "image 2 (valid_len 1)" in msg and "query 32 (masked, query block 1)" in msg and "feature 5" in msg and "nj2" in msg


# ---- layernorm_cm, transpose2d ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", HP.LNCM_SHAPES)
def test_layernorm_builder_is_the_formula(C, M):
    for r in HP.LNCM_OFFSETS:
        k = HP.lncm_case(C, M, r)
        x = k["x"].double()
        mean, var = x.mean(0), x.var(0, unbiased=False)
        y = (x - mean) / torch.sqrt(var + HP.LNCM_EPS) * k["gamma"].double()[:, None] + k["beta"].double()[:, None]
        assert torch.allclose(k["y"], y, rtol=1e-11, atol=1e-11)
        assert abs(float(k["x"].mean()) - r) < 4.0 / (C * M) ** 0.5 + 1e-3
        if C == 1:
            assert torch.equal(k["y"], k["beta"].double()[:, None].expand(1, M))


def test_transpose_cases_hold_their_specials():
    assert HP.TRANSPOSE_SHAPES == ((1, 1), (1, 70), (33, 31), (32, 32), (65, 97))
    x = HP.transpose_case(65, 97)
    assert np.isinf(x).sum() == 2 and (np.signbit(x) & (x == 0)).any() and (x == np.float32(1e-45)).any()


# ---- linear_ln --------------------------------------------------------------------------------------------------------------
# (the three shapes with more than 100000 outputs are left out to keep this file quick: the builder does not depend on size)
@pytest.mark.parametrize("K,M,Co", [s for s in HP.LINEAR_LN_SHAPES if s[1] * s[2] < 100000])
def test_linear_ln_builder_and_restatement(K, M, Co):
    k = HP.linear_ln_case(K, M, Co, 1.0)
    x, ga, be, w, b = (k[n].double() for n in ("x", "gamma", "beta", "w", "b"))
    mean, var = x.mean(0), x.var(0, unbiased=False)
    ln = ((x - mean) / torch.sqrt(var + HP.LINEAR_LN_EPS) * ga[:, None] + be[:, None]).t()             # (M, K)
    z = F.linear(ln, w, b)
    assert torch.allclose(k["tm"], z, rtol=1e-11, atol=1e-11)
    assert torch.allclose(k["cm"], (0.5 * z * (1.0 + torch.erf(z / 2 ** 0.5))).t() + k["res"].double(), rtol=1e-11, atol=1e-11)
    # the folded operands are the identity the header states, and the restatement computes it
    wg, colsum, bias_eff = (t.double() for t in k["folded"])
    assert torch.allclose(wg, ga[:, None] * w.t(), rtol=1e-6, atol=1e-7) and torch.allclose(colsum, wg.sum(0), atol=1e-4)
    assert torch.allclose(bias_eff, be @ w.t() + b, atol=1e-4)
    if K == 2:             # two nearly equal values cancel in E[x^2] - mean^2: the raw formula misses the project's bar
        assert 1e-5 < HP.rel(k["tm_restated"], k["tm"]) < 1e-2
    else:
        assert HP.rel(k["tm_restated"], k["tm"]) < 1e-5 and HP.rel(k["cm_restated"], k["cm"]) < 1e-5


def test_restated_error_far_from_zero_mean_is_above_pytorchs():
    """The second bar is needed: at |mean| / std = 64 (and 16) the folded formula itself, in fp32, is less accurate than
    PyTorch's fp32 LayerNorm -> Linear, and above the project's 1e-5 floor at 64; at offsets up to 4 it is not."""
    for K, M, Co in ((128, 64, 64), (512, 64, 64)):
        err = {}
        for r in (4.0, 16.0, 64.0):
            k = HP.linear_ln_case(K, M, Co, r)
            lib32 = HP.linear_ln_lib32(k, True, "cpu")
            err[r] = (HP.rel(k["tm_restated"], k["tm"]), HP.rel(lib32, k["tm"]))
            print(f"K {K} offset {r:g}: restated {err[r][0]:.3e}, PyTorch fp32 (CPU) {err[r][1]:.3e}")
        assert err[64.0][0] > 2 * err[64.0][1] and err[64.0][0] > 1e-5
        assert err[16.0][0] > err[16.0][1]
        assert err[4.0][0] < 1e-5
    assert HP.LINEAR_LN_FAR_OFFSETS == (16.0, 64.0) and HP.LINEAR_LN_BAR_OFFSETS == (0.0, 1.0, 4.0)


def test_constant_column_is_exact_up_to_the_two_sums():
    """On a constant column K c, K c^2, their quotients by K and c^2 are exact in fp32 for the constants and K used, so the
    variance is exactly 0 and only the two K-term sums round; the restatement stays within the bound the GPU test applies."""
    for K, M, Co in HP.LINEAR_LN_SHAPES:
        for c in HP.LINEAR_LN_CONSTS:
            c32 = np.float32(c)
            assert np.float32(K) * c32 * c32 < EXACT and np.float32(K * c) / np.float32(K) == c32
            assert np.float32(K * c * c) / np.float32(K) - c32 * c32 == 0
    for K, M, Co in ((127, 33, 40), (513, 40, 64)):
        for c in HP.LINEAR_LN_CONSTS:
            k = HP.linear_ln_case(K, M, Co, 0.0, c)
            assert bool((k["x"][:, M - 1] == c).all()) and float(k["x"][:, :M - 1].std()) > 0.9
            err = (k["tm_restated"][M - 1].double() - k["folded"][2].double()).abs()
            assert torch.isfinite(err).all() and bool((err <= HP.const_column_bound(k, c)).all())


# ---- the refusals that return before a launch ---------------------------------------------------------------------------------
def test_argument_refusals(lib):
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rc, text):
        assert rc == EINVAL and text in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())

    refused(lib.tpspp_layernorm_cm_fwd(p, p, p, 1025, 1, 1e-5, p, None), b"at most 1024 features")
    refused(lib.tpspp_layernorm_cm_fwd(p, p, p, 0, 1, 1e-5, p, None), b"bad argument")
    refused(lib.tpspp_layernorm_cm_fwd(p, None, p, 4, 1, 1e-5, p, None), b"bad argument")
    refused(lib.tpspp_transpose2d(p, 0, 4, p, None), b"bad argument")
    refused(lib.tpspp_transpose2d(p, 4, 4, None, None), b"bad argument")
    refused(lib.tpspp_linear_ln_fwd(p, 2, 2, 1e-5, p, p, 2, p, 2, None, 1, p, None), b"token-major form takes no activation")
    refused(lib.tpspp_linear_ln_fwd(p, 2, 2, 1e-5, p, p, 2, p, 0, p, 1, p, None), b"token-major form takes no activation")
    refused(lib.tpspp_linear_ln_fwd(p, 2, 2, 1e-5, p, p, 2, p, 3, None, 0, p, None), b"bad sizes / activation")
    refused(lib.tpspp_linear_ln_fwd(p, 2, 2, 1e-5, p, p, 2, p, -1, None, 0, p, None), b"bad sizes / activation")
    refused(lib.tpspp_linear_ln_fwd(p, 0, 2, 1e-5, p, p, 2, p, 0, None, 0, p, None), b"bad sizes / activation")
    refused(lib.tpspp_linear_ln_fwd(p, 2, 2, 1e-5, p, None, 2, p, 0, None, 0, p, None), b"null pointer")
    refused(lib.tpspp_attn_enc_fwd(p, 1, 64, 257, None, p, None), b"at most 256 tokens")
    refused(lib.tpspp_attn_enc_fwd(p, 1, 96, 4, None, p, None), b"multiple of 64")
    refused(lib.tpspp_attn_enc_fwd(p, 1, 64, 0, None, p, None), b"bad argument")
    refused(lib.tpspp_attn_enc_fwd(p, 65536, 64, 4, None, p, None), b"batch too large")


# ---- the tables reach every instantiation and branch --------------------------------------------------------------------------
def test_attention_tables_reach_every_path():
    assert HP.ATTN_T == (1, 32, 33, 64, 65, 96, 97, 128, 129, 256)
    assert [HP.attn_path(T) for T in HP.ATTN_T] == ["nj1", "nj1", "nj2", "nj2", "nj3", "nj3", "nj4", "nj4", "lds", "lds"]
    paths = ("nj1", "nj2", "nj3", "nj4", "lds")
    onehot = {p: [c for c in HP.ONEHOT_CASES if HP.attn_path(c["T"]) == p] for p in paths}
    for p in paths:
        assert {c["H"] for c in onehot[p]} == {1, 2}, f"{p}: C = 64 and C = 128"
    # a last workgroup with fewer than four live wavefronts, per NJ (NJ = 4: N * heads * 4 is always a multiple of 4)
    for p in ("nj1", "nj2", "nj3"):
        assert any(HP.attn_wavefronts(c["N"], c["H"], c["T"]) % 4 for c in onehot[p]), p
    assert {HP.attn_path(T) for T in HP.ATTN_B_T} == {"nj1", "nj3", "nj4", "lds"}
    assert {HP.attn_path(c["T"]) for c in HP.UNIFORM_CASES} == {"nj2", "nj3", "lds"}
    assert [c["T"] for c in HP.UNIFORM_CASES] == [33, 96, 129]
    for T in HP.ATTN_T + HP.ATTN_B_T:
        vl = HP.ragged(T)
        assert vl[0] == T + 5 and 1 <= vl[1] <= T and vl[2] == 1
    assert [HP.attn_path(c["T"]) for c in HP.ONEHOT_CASES if c["id"] in ("t33-n3-h1", "t129-n3-h1")] == ["nj2", "lds"]


def test_layernorm_table_reaches_every_instantiation():
    assert HP.LNCM_SHAPES == ((1, 5), (2, 16), (100, 1), (128, 17), (129, 33), (512, 16), (513, 15), (1000, 40), (1024, 3))
    assert {HP.layernorm_vpt(C) for C, _ in HP.LNCM_SHAPES} == {8, 32, 64}
    assert [HP.layernorm_vpt(C) for C in (128, 129, 512, 513, 1024)] == [8, 32, 32, 64, 64]
    assert any(C % 16 for C, _ in HP.LNCM_SHAPES) and any(M % 16 for _, M in HP.LNCM_SHAPES) and (100, 1) in HP.LNCM_SHAPES
    assert HP.LNCM_OFFSETS == (0.0, 16.0, 100.0)


def test_linear_ln_table_reaches_every_variant_and_branch():
    want = {(128, 64, 64): (4, {"fast"}), (127, 33, 40): (4, {"fast", "slow"}), (1, 3, 5): (4, {"slow"}),
            (2, 32, 32): (4, {"slow"}), (255, 40, 96): (4, {"slow"}), (512, 64, 64): (16, {"fast"}),
            (256, 33, 92): (16, {"slow"}), (513, 40, 64): (16, {"slow"}), (256, 545, 929): (8, {"fast", "slow"}),
            (512, 545, 929): (8, {"slow"}), (256, 512, 1024): (16, {"slow"})}
    assert set(HP.LINEAR_LN_SHAPES) == set(want)
    reached = set()
    for shape in HP.LINEAR_LN_SHAPES:
        nw, taken = HP.linear_ln_paths(*shape)
        assert (nw, taken) == want[shape], shape
        # both layouts run every shape (the GPU test's parametrisation), and the selection does not depend on the layout
        assert HP.linear_ln_paths(shape[0], shape[2], shape[1]) == (nw, taken)
        reached |= {(nw, layout, branch) for layout in HP.LAYOUT_IDS.values() for branch in taken}
    assert reached == {(nw, layout, branch) for nw in (4, 8, 16) for layout in ("channel-major", "token-major")
                       for branch in ("fast", "slow")}
    tiles = lambda s: -(-s[1] // 32) * -(-s[2] // 32)  # noqa: E731
    assert tiles((256, 512, 1024)) == 512 and tiles((256, 545, 929)) > 512
    assert any(s[0] % 2 for s in HP.LINEAR_LN_SHAPES)
    # the slow loop of (255, 40, 96) makes two trips, that of (513, 40, 64) two as well with a 3-value last slice
    assert -(-255 // 8) * 2 == 64 and -(-513 // 32) * 2 == 34 and 513 - 15 * 34 == 3


def test_outlier_cases_probe_the_shift():
    """One outlier in a sampled row leaves the median of three a typical value, and the formula on the shifted column inside
    the project's bar; a shift by row 0 alone would not be (the single-feature shift this replaces); two sampled rows on the
    same side make the median an outlier."""
    assert HP.sampled_rows(512) == (0, 256, 511) and HP.sampled_rows(2) == (0, 1, 1) and HP.sampled_rows(1) == (0, 0, 0)
    K, M, Co = 512, 64, 64
    assert (K, M, Co) in HP.LINEAR_LN_OUTLIER_SHAPES and HP.linear_ln_paths(K, M, Co) == (16, {"fast"})
    assert HP.linear_ln_paths(128, 64, 64) == (4, {"fast"}) and HP.linear_ln_paths(513, 40, 64) == (16, {"slow"})
    cases = HP.outlier_cases(K)
    assert len(cases) == 10 and sum(strict for _, _, strict in cases) == 8
    for what, outlier, strict in cases:
        k = HP.linear_ln_case(K, M, Co, 0.0, None, outlier)
        x = k["x"].numpy()
        shift = x[0] - HP.med3_shifted(x)[0]
        assert (np.abs(shift) < 5.0).all() == strict, what
        e_shifted = HP.rel(k["tm_shifted"], k["tm"])
        folded = [t.numpy() for t in k["folded"]]
        by_row0 = HP.rel(torch.from_numpy(HP.linear_ln_restated(x - x[0:1], folded, HP.LINEAR_LN_EPS)), k["tm"])
        print(f"{what}: restated as shifted {e_shifted:.3e}, shifted by row 0 alone {by_row0:.3e}, on raw values "
              f"{HP.rel(k['tm_restated'], k['tm']):.3e}")
        if strict:
            assert e_shifted < 2e-6
        if outlier == ((0,), 1000.0):
            assert by_row0 > 5e-6
