"""CPU tests of the warp backward's planner and of the case table of tests/test_gpu_warp_bwd_routes.py: every case takes the
route the table states (`ops.warp_backward_route` on CPU tensors: the query reads shapes and alignments only), the table
reaches what it claims to reach, comparison A's data are exactly representable in every accumulator (the 2^24 proof), the
float64 reference agrees with PyTorch's float64 autograd, each seeded fault of the reference moves the expected values, and
the query refuses what the entry point refuses, with the same code and text."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import warp_bwd_route_cases as W
from tps_pp_amd import _lib, build, ops

NAMES = list(W.CASES)


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


@pytest.fixture(scope="module")
def routes(_built):
    return {name: W.route_of(c) for name, c in W.CASES.items()}


@pytest.mark.parametrize("name", NAMES)
def test_every_case_takes_the_route_the_table_states(routes, name):
    assert str(routes[name]) == W.ROUTES[name]


def test_the_table_reaches_every_family_form_and_instantiation(routes):
    rs = list(routes.values())
    assert {r.family for r in rs} == {"classic", "classic_bf16", "lds2", "lds", "atomics"}
    # kernel A'': 4 (PPT, NT) forms x 2 accumulators x 2 element types
    forms = {(r.ppt, r.nt, r.f64, r.bf16) for r in rs if r.family == "lds2"}
    assert forms == {(p, t, a, b) for p, t in ((1, 256), (2, 256), (4, 256), (4, 1024)) for a in (0, 1) for b in (0, 1)}
    # ... each at both edges of its range of n, with both accumulators
    edges = {(W.n_of(W.CASES[k]), r.ppt, r.nt, r.f64) for k, r in routes.items() if r.family == "lds2"}
    for n, ppt, nt in ((256, 1, 256), (257, 2, 256), (512, 2, 256), (513, 4, 256), (1024, 4, 256), (1025, 4, 1024), (4096, 4, 1024)):
        assert {(n, ppt, nt, 0), (n, ppt, nt, 1)} <= edges, n
    assert {r.G for r in rs if r.family == "lds2"} >= {1, 3, 8}
    assert any(r.family == "lds2" and max(r.chunks0, r.chunks1) > r.G for r in rs)
    assert any(r.family == "lds2" and 0 < r.chunks1 < r.G for r in rs)
    # the parameter kernel: all 60 instantiations, every S, slice counts from 1 to 16 (every two-kernel route hands dL/d grid
    # over in slices: there is no count of 0)
    keys = {r.params_key for r in rs if r.params}
    assert len(keys) == 60 and keys == {(k, t, tr, s, g) for k in (24, 36, 64) for t in (0, 1) for tr in (0, 1)
                                        for s, g in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1))}
    assert {r.S for r in rs if r.params} == set(range(1, 9))
    assert {r.slots for r in rs if r.params} >= {1, 2, 3, 6, 16} and all(1 <= r.slots <= 16 for r in rs if r.params)
    assert {r.slots for r in rs if r.family == "atomics"} >= {1, 3} and {r.slots for r in rs if r.family == "lds"} >= {1, 4, 6}
    assert {W.CASES[k].F for k, r in routes.items() if r.params} >= {1, 21, 22, 33, 34, 61}
    assert any(c.ld_extra for c in W.CASES.values())
    # three ways into kernel A' and two into kernel A
    lds = [W.CASES[k] for k, r in routes.items() if r.family == "lds"]
    assert any(c.in0[0] * c.in0[1] % 4 for c in lds) and any(16384 < c.in0[0] * c.in0[1] * 4 <= 65536 and c.in0[0] * c.in0[1] % 4 == 0 for c in lds)
    assert any(c.misalign0 for c in lds)
    assert any(r.family == "lds" and r.cpt0 != r.cpt1 and r.chunks1 for r in rs)
    assert any(r.family == "lds" and max(r.chunks0, r.chunks1) > r.G for r in rs)
    assert any(r.family == "lds" and 0 < r.chunks1 < r.G for r in rs)
    ato = [W.CASES[k] for k, r in routes.items() if r.family == "atomics"]
    assert any(W.n_of(c) == 4100 for c in ato) and any(c.in0 == (129, 128) for c in ato)
    assert {c.in0 for c in ato} >= {(48, 160), (64, 256)}
    # the one-launch form: C0 = 1, 2, 3; n just above 1024 and 4096; F = 1, 20, 21; both element types
    one = [W.CASES[k] for k, r in routes.items() if r.family in ("classic", "classic_bf16")]
    assert {c.C0 for c in one} == {1, 2, 3} and {c.F for c in one} == {1, 20, 21}
    assert {W.n_of(c) for c in one} >= {1028, 4096} and any(c.in0 != c.out for c in one) and any(not c.need0 for c in one)
    assert {c.C0 for c in one if c.bf16} == {1, 3}


def test_ragged_slices_and_lengths_off_the_wavefront(routes):
    pers = [((W.n_of(W.CASES[k]) + r.S - 1) // r.S, W.n_of(W.CASES[k]), r.S) for k, r in routes.items() if r.params and r.S > 1]
    assert any(n % S for _, n, S in pers)                                   # a ragged last slice
    assert any(per % 256 and per % 64 for per, _, _ in pers)


@pytest.mark.parametrize("name", NAMES)
def test_comparison_a_is_exact_in_every_accumulator(name):
    """The proof that summation order cannot matter: the sum of |terms| of every accumulator, in units of its finest bit, is
    below 2^24.  And the data are not degenerate: every fault of the reference that applies to the case moves an output."""
    c = W.CASES[name]
    d = W.make_data(c)
    ref = W.reference(d)
    bits = W.exact_bits(d, ref)
    assert max(bits.values()) < 2 ** 24, bits
    assert np.abs(ref["g_grid"]).max() > 0 and np.abs(ref["g_ctrl"]).max() > 0 and np.abs(ref["g_in0"]).max() > 0
    _, _, S = W.plan_numbers(c)
    for fault in W.FAULTS:
        if fault == "ragged_channel_dropped" and not (c.C0 % 8 or c.C1 % 8):
            continue
        if (fault == "last_slice_dropped" and S == 1) or (fault == "score_on_affine_columns" and not c.score):
            continue
        bad = W.reference(d, fault)
        moved = [k for k in ("g_in0", "g_in1", "g_grid", "g_ctrl", "g_score")
                 if ref[k] is not None and not np.array_equal(ref[k], bad[k])]
        assert moved, (name, fault)


@pytest.mark.parametrize("name", ["lds2 n=513 f64", "lds: 17x33 + 17x9, C=9 | 17", next(k for k in NAMES if k.startswith("params k36 t0 T1 s1 g1")),
                                  "classic C2 24x33 -> 33x40 F=20"])
def test_reference_agrees_with_float64_autograd(name):
    """PyTorch's float64 autograd of F.grid_sample(border, align_corners=True) composed with the row construction, on real
    data and a grid without kinks (no point on a pixel centre or on the border): an independent formulation."""
    c = W.CASES[name]
    n = W.n_of(c)
    grid = 0.98 * W.synth.dyadic((c.N, n, 2), name + ".agrid", 1)
    d = W.make_data(c, exact=False, grid=grid)
    ref = W.reference(d)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()       # noqa: E731
    ctrl = tt(W.synth.dyadic((c.N, c.F, 2), name + ".ctrl", 1)).requires_grad_(True)
    # the forward in float64 with a grid OFFSET that makes it equal the case's grid: grid = rows T + const
    T = torch.matmul(tt(d["inv"])[None], torch.cat([ctrl, torch.zeros(c.N, 3, 2, dtype=torch.float64)], 1))
    ph = tt(d["ph"])
    score = tt(d["score"]).requires_grad_(True) if c.score else None
    if c.table:
        head, rbf = torch.cat([torch.ones(n, 1, dtype=torch.float64), tt(d["xy"])], 1), ph[:, :c.F]
    else:
        head, rbf = ph[:, :3], ph[:, 3:c.F + 3]
    rbf = rbf[None].expand(c.N, -1, -1) * (0.5 * score + 1.0) if c.score else rbf[None].expand(c.N, -1, -1)
    rows = torch.cat([head[None].expand(c.N, -1, -1), rbf], 2)
    g = torch.matmul(rows, T)
    g = g + (tt(d["grid"]) - g).detach()
    ins = [tt(d[f"in{i}"]).requires_grad_(True) for i in (0, 1) if d[f"in{i}"] is not None]
    L = sum((Fn.grid_sample(x, g.reshape(c.N, *c.out, 2), padding_mode="border", align_corners=True) * tt(d[f"g{i}"])).sum()
            for i, x in enumerate(ins))
    L.backward()
    for i, x in enumerate(ins):
        # (the reference's weights are the kernels' fp32 ones: ix carries three roundings of up to 2^-24 max(H, W) each,
        # and so does every weight of every term that lands on an element)
        tol = 8 * 2.0 ** -24 * max(x.shape[2:]) * ref[f"cnt{i}"].max() * np.abs(d[f"g{i}"]).max()
        assert np.abs(ref[f"g_in{i}"] - x.grad.numpy()).max() <= tol, i
    # dL/d grid through the chain: compare dL/d control points and dL/d score, computed from the reference's dL/d grid, with
    # autograd's; autograd's T is built from ctrl, the reference's dL/d score takes T as an argument
    d2 = dict(d, T=T.detach().numpy())
    g_ctrl, g_score, _ = W.params_reference(d2, ref["g_grid"])
    tol = 2.0 ** -16                                       # (dL/d grid inherits the fp32 weights' roundings)
    assert np.abs(g_ctrl - ctrl.grad.numpy()).max() <= tol * np.abs(g_ctrl).max()
    if c.score:
        assert np.abs(g_score - score.grad.numpy()).max() <= tol * np.abs(g_score).max()


# ---- refusals: the query and the entry point are one planner ---------------------------------------------------------------
G_OUT0, IN0, G_IN0 = 0, 1, 23            # positions of three pointers in the argument list


def _raw_args(c, N, flags=0, ws=None, shift=None):
    """Argument list of tpspp_warp_bwd / tpspp_warp_bwd_route (without stream / route) on one small host buffer.  `shift`:
    {position: bytes} moves single pointers off their alignment."""
    buf = torch.zeros(64)
    a = buf.data_ptr()
    assert a % 16 == 0
    n = W.n_of(c)
    nws = _lib.lib().tpspp_warp_bwd_workspace_floats(N, *c.out) if ws is None else ws
    two = a if c.C1 else 0
    args = [a, a, c.C0, *c.in0, two, two, c.C1, *(c.in1 or (0, 0)), a, 0, a, a, W.cols_of(c), 0, 0, a, flags, N, c.F, *c.out,
            a, two, a, 0, a, nws]
    for pos, nbytes in (shift or {}).items():
        args[pos] += nbytes
    return args, buf, n


REFUSED = [
    ("N = 65536", W.case("r", 65536, 1, (2, 2), (1, 1)), 0, "N > 65535"),
    ("bf16 n > 4096", W.case("r", 0, 1, (8, 8), (64, 200)), ops.IO_BF16, "4096 output pixels"),
    ("bf16 plane > 4096", W.case("r", 0, 1, (96, 64), (16, 64)), ops.IO_BF16, "more than 4096 pixels"),
    ("bf16 plane % 8", W.case("r", 0, 1, (15, 21), (16, 64)), ops.IO_BF16, "multiple of 8"),
    ("bf16 g_in0 4 bytes off", W.case("r", 0, 1, (8, 8), (16, 64)), ops.IO_BF16, "not 16-byte aligned", {G_IN0: 4}),
    ("bf16 in0 8 bytes off", W.case("r", 0, 1, (8, 8), (16, 64)), ops.IO_BF16, "not 16-byte aligned", {IN0: 8}),
    ("bf16 g_out0 1 byte off", W.case("r", 0, 1, (8, 8), (16, 64)), ops.IO_BF16, "not 2-byte aligned", {G_OUT0: 1}),
]


@pytest.mark.parametrize("what,c,flags,text,shift", [r if len(r) == 5 else r + (None,) for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_query_and_entry_point_refuse_alike(what, c, flags, text, shift):
    lib = _lib.lib()
    args, keep, _ = _raw_args(c, c.N, flags, shift=shift)
    rc_entry = lib.tpspp_warp_bwd(*args, 0)                                  # refused before any launch: no device needed
    msg_entry = lib.tpspp_last_error().decode()
    route = (ctypes.c_int * 18)()
    rc_query = lib.tpspp_warp_bwd_route(*args, ctypes.cast(route, ctypes.c_void_p), 18)
    msg_query = lib.tpspp_last_error().decode()
    assert rc_entry == rc_query == -22 and msg_entry == msg_query and text in msg_entry, (rc_entry, rc_query, msg_entry, msg_query)


def test_query_refuses_a_small_workspace_and_a_short_route_array():
    lib = _lib.lib()
    c = W.case("r", 2, 1, (8, 8), (8, 8))
    args, keep, _ = _raw_args(c, 2, ws=10)
    route = (ctypes.c_int * 18)()
    vp = ctypes.cast(route, ctypes.c_void_p)
    assert lib.tpspp_warp_bwd_route(*args, vp, 18) == -22 and "g_grid_ws too small" in lib.tpspp_last_error().decode()
    args, keep, _ = _raw_args(c, 2)
    assert lib.tpspp_warp_bwd_route(*args, vp, 17) == -22
    assert lib.tpspp_warp_bwd_route(*args, vp, 18) == 0 and route[0] == 2
    args, keep, _ = _raw_args(c, 0)                                          # an empty batch: accepted, nothing to launch
    assert lib.tpspp_warp_bwd_route(*args, vp, 18) == 0 and route[0] == -1 and lib.tpspp_warp_bwd(*args, 0) == 0


def test_query_follows_the_process_wide_accumulator():
    c = W.CASES["lds2 n=512 f64"]
    try:
        ops.set_warp_bwd_accumulator(True)
        assert "fix" in str(W.route_of(c))
    finally:
        ops.set_warp_bwd_accumulator(False)
    assert "f64" in str(W.route_of(c))


# ---- comparison B: the bars have teeth -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.REAL)
def test_every_seeded_fault_violates_the_derived_bars(routes, name):
    """A kernel with one of FAULTS would return the faulty reference's values: each must leave the case's bars in at least one
    element (stage 1: dL/d input and dL/d grid around the sound reference; stage 2: the parameter outputs, from the sound
    dL/d grid)."""
    c = W.real_case(name)
    r = W.route_of(c)
    assert r.family == routes[name].family
    d = W.make_real(c)
    ref = W.reference(d)
    bars = W.stage1_bars(c, r, ref)
    (g_ctrl, b_ctrl), (g_score, b_score) = W.stage2(d, c, r, ref["g_grid"])
    assert np.isfinite(ref["g_grid"]).all() and (bars["g_grid"] < 1e-3 * max(1.0, np.abs(ref["g_grid"]).max())).all()
    for fault in W.FAULTS:
        if fault == "ragged_channel_dropped" and not (c.C0 % 8 or c.C1 % 8):
            continue
        if fault == "last_slice_dropped" and (not r.params or r.S == 1):
            continue
        if fault == "score_on_affine_columns" and not c.score:
            continue
        if fault in ("last_slice_dropped", "score_on_affine_columns"):
            (bad_ctrl, _), (bad_score, _) = W.stage2(d, c, r, ref["g_grid"], fault)
            out = bool((np.abs(bad_ctrl - g_ctrl) > b_ctrl).any())
        else:
            bad = W.reference(d, fault)
            out = any(bool((np.abs(bad[k] - ref[k]) > bars[k]).any()) for k in bars)
        assert out, (name, fault)


def test_report_names_the_element_the_taps_and_the_route(routes):
    name = "lds: 17x33 + 17x9, C=9 | 17"
    c, r = W.CASES[name], routes[name]
    d = W.make_data(c)
    ref = W.reference(d)
    assert W.report(c, r, d, "g_in0", ref["g_in0"], ref["g_in0"] + 0.0) is None
    assert W.report(c, r, d, "g_grid", -ref["g_grid"] * 0.0, ref["g_grid"] * 0.0) is None          # -0.0 equals +0.0
    bad = ref["g_in0"].copy()
    b, ch, y, x = (int(v[0]) for v in np.nonzero(ref["cnt0"] > 1))
    bad[b, ch, y, x] += 0.5
    msg = W.report(c, r, d, "g_in0", bad, ref["g_in0"])
    assert f"the worst at ({b}, {ch}, {y}, {x})" in msg and "lds cpt8,8 G3" in msg and f"chunk {ch // 8} of 8" in msg
    assert f"{int(ref['cnt0'][b, ch, y, x])} taps land here" in msg and " w=" in msg
    bad = ref["g_grid"].copy()
    bad[0, 300, 1] = np.nan
    msg = W.report(c, r, d, "g_grid", bad, ref["g_grid"])
    assert "output pixel 300 = (11, 3)" in msg and "slice 1 of 2" in msg and "north-west tap" in msg
    bad = ref["g_ctrl"].copy()
    bad[0, 7, 0] += 1.0
    assert "control point 7" in W.report(c, r, d, "g_ctrl", bad, ref["g_ctrl"], 0.5 * np.ones_like(bad))
    assert W.report(c, r, d, "g_ctrl", bad, ref["g_ctrl"], 2.0 * np.ones_like(bad)) is None
