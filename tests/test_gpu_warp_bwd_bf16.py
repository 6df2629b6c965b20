"""-m gpu: TPSPP_IO_BF16 of tpspp_warp_bwd -- bf16 images, output gradients and input gradients; grid, tables, score, dL/d
control points, dL/d score, the workspace and all accumulation fp32 / fp64 as without the bit.

The yardstick is the fp32 kernel on the widened inputs (held to the reference's autograd by tests/test_gpu_backward.py): with
the order-independent fixed-point accumulator the bf16 call must give `fp32_call(widened).bfloat16()` bit for bit, and the
fp32 outputs (dL/d control points, dL/d score, dL/d grid in the workspace) the fp32 call's bits.  Inputs are `synth.dyadic`
rounded to bf16; the control points are perturbed as in tests/test_gpu_backward.py (amplitudes 0, 0.6 and 3: clamped borders).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import cases
from oracle import tps_oracle as O
from test_gpu_memory_safety import run_twice
from tps_pp_amd import TPS_PP, TPSPreprocessor, _lib, constants, ops, synth

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
F = 20
AMP = np.array([0.0, 0.6, 3.0], np.float32)


def rb(a):
    """An fp32 numpy array rounded to bf16 (CPU tensor)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF)


class Case:
    """CPU tensors of one call.  in0 / in1 / g0 / g1 are bf16; everything else fp32."""

    def __init__(self, name, N, C0, in_hw, out_hw, classic, C1=0, score=False, flags=0, need0=True, need1=True):
        self.name, self.N, self.out_hw, self.classic, self.flags = name, N, tuple(out_hw), classic, flags
        self.need0, self.need1 = need0, need1
        n = out_hw[0] * out_hw[1]
        amp = AMP[:N, None, None]
        if classic:
            c = O.classic_constants(F, self.out_hw)
            self.inv, self.P, self.xy = torch.from_numpy(c["inv_delta_C"]), torch.from_numpy(c["P_hat"]), None
            self.ctrl = torch.from_numpy((O.classic_initial_ctrl(F)[None] + amp * synth.dyadic((N, F, 2), "bwd.ctrl", 1))
                                         .astype(np.float32))
        else:
            K = constants.tpspp(self.out_hw, (2, 10))
            self.inv, self.P, self.xy = (torch.from_numpy(np.ascontiguousarray(K[k])) for k in ("hat_C", "P_hat", "P_xy"))
            self.ctrl = torch.from_numpy((constants.tpspp_initial_ctrl((2, 10))[None] +
                                          0.5 * amp * synth.dyadic((N, F, 2), "bwd.ctrl", 1)).astype(np.float32))
        self.in0 = rb(synth.dyadic((N, C0) + tuple(in_hw), name + ".in0", 1))
        self.g0 = rb(synth.dyadic((N, C0) + self.out_hw, name + ".g0", 1))
        self.in1 = rb(synth.dyadic((N, C1) + tuple(in_hw), name + ".in1", 1)) if C1 else None
        self.g1 = rb(synth.dyadic((N, C1) + self.out_hw, name + ".g1", 1)) if C1 else None
        self.score = torch.from_numpy(0.5 * synth.dyadic((N, n, F), name + ".score", 1)) if score else None

    def __repr__(self):
        return self.name


FIX, TWO = ops.BWD_FIXED_POINT, ops.BWD_TWO_KERNELS


@functools.lru_cache(maxsize=None)
def all_cases():
    lds2 = dict(C0=9, in_hw=(16, 64), classic=False, C1=9, score=True)
    return {c.name: c for c in [
        # the classic call: one input of <= 3 channels, transposed table, no score (the one-launch form with the default
        # accumulator; kernel A'' with 1024 threads with the fixed point; 64x64x3 exceeds the one-launch form's LDS)
        Case("cl_3x32x100", 3, 3, (32, 100), (32, 100), True),
        Case("cl_1x32x64", 2, 1, (32, 64), (32, 64), True),
        Case("cl_3x64x64", 2, 3, (64, 64), (64, 64), True),
        Case("cl_2x40x40", 2, 2, (40, 40), (40, 40), True),
        # kernel A'' + the parameter kernel: score, P_xy, two inputs of nine channels (across the 8-channel chunk)
        Case("pp_8x32", 2, out_hw=(8, 32), **lds2), Case("pp_16x32", 2, out_hw=(16, 32), **lds2),
        Case("pp_16x64", 2, out_hw=(16, 64), **lds2), Case("pp_32x64", 2, out_hw=(32, 64), **lds2),
        Case("pp_one_input_16x64", 2, 9, (16, 64), (16, 64), False),
        Case("cl_two_kernels", 3, 3, (32, 100), (32, 100), True, flags=TWO),
        Case("pp_no_g_in0", 2, out_hw=(16, 64), need0=False, **lds2),
        Case("pp_null_g_in1", 2, out_hw=(16, 64), need1=False, **lds2),
    ]}


NAMES = list(all_cases())
_REF = {}


def raw_bwd(cuda, c, dtype, flags, prefill=None):
    """tpspp_warp_bwd on buffers of this test's own: -> dict(rc, g_in0, g_in1, g_ctrl, g_score, g_grid, ...)."""
    d = lambda t: None if t is None else t.to(cuda)                                  # noqa: E731
    in0, in1, g0, g1 = (None if t is None else t.to(cuda).to(dtype) for t in (c.in0, c.in1, c.g0, c.g1))
    inv, P, xy, ctrl, score = d(c.inv), d(c.P), d(c.xy), d(c.ctrl), d(c.score)
    Ho, Wo = c.out_hw
    H0, W0 = tuple(c.in0.shape[2:])
    N, n = c.N, c.out_hw[0] * c.out_hw[1]
    _, _, grid, _ = ops.warp(in0.float(), ctrl, inv, P, c.out_hw, P_xy=xy, score=score, in1=None if in1 is None else in1.float(),
                             want_grid=True)
    T = ops.solve_T(inv, ctrl) if score is not None else None
    Pt = ops.transpose_p_hat(P) if c.classic else None
    mk = (lambda like, dt: torch.full_like(like, prefill, dtype=dt)) if prefill is not None else \
        (lambda like, dt: torch.empty_like(like, dtype=dt))
    g_in0 = mk(in0, dtype) if c.need0 else None
    g_in1 = mk(in1, dtype) if (in1 is not None and c.need1) else None
    g_ctrl = mk(ctrl, F32)
    g_score = mk(score, F32) if score is not None else None
    ws = mk(torch.empty(int(_lib.lib().tpspp_warp_bwd_workspace_floats(N, Ho, Wo)), device=cuda), F32)
    p = ops._ptr
    fl = flags | (ops.IO_BF16 if dtype == BF else 0)
    rc = _lib.lib().tpspp_warp_bwd(p(g0), p(in0), in0.shape[1], H0, W0, p(g1), p(in1), 0 if in1 is None else in1.shape[1],
                                   H0 if in1 is not None else 0, W0 if in1 is not None else 0, p(grid), p(T), p(inv), p(P),
                                   P.shape[1], p(xy), p(score), p(Pt), fl, N, F, Ho, Wo, p(g_in0), p(g_in1), p(g_ctrl),
                                   p(g_score), p(ws), ws.numel(), ops._stream(in0))
    torch.cuda.synchronize()
    return dict(rc=rc, g_in0=g_in0, g_in1=g_in1, g_ctrl=g_ctrl, g_score=g_score, g_grid=ws[:N * n * 2], ws=ws, grid=grid)


def reference(cuda, name):
    """The fp32 kernel (fixed point) on the widened inputs of a case: computed once, shared, never modified."""
    if name not in _REF:
        c = all_cases()[name]
        _REF[name] = raw_bwd(cuda, c, F32, c.flags | FIX)
        assert _REF[name]["rc"] == 0
    return _REF[name]


def same_bits(a, b):
    it = {F32: torch.int32, BF: torch.int16}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def bf16_ulps(a, b):
    ia, ib = (t.contiguous().view(torch.int16).long() for t in (a, b))
    ia = torch.where(ia < 0, -(ia & 0x7FFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFF), ib)
    return (ia - ib).abs()


# ---- 1. bits against the fp32 kernel (fixed point: order-independent) ----------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixed_point_bits_equal_the_fp32_kernel_rounded_once(cuda, name):
    c, ref = all_cases()[name], reference(cuda, name)
    got = raw_bwd(cuda, c, BF, c.flags | FIX)
    assert got["rc"] == 0, _lib.lib().tpspp_last_error()
    for k in ("g_in0", "g_in1"):
        assert (got[k] is None) == (ref[k] is None)
        if ref[k] is not None:
            assert got[k].dtype == BF and same_bits(got[k], ref[k].bfloat16()), k
    assert ref["g_in0"] is not None or not c.need0
    for k in ("g_ctrl", "g_score", "g_grid"):
        if ref[k] is not None:
            assert got[k].dtype == F32 and same_bits(got[k], ref[k]), k
    assert torch.isfinite(ref["g_ctrl"]).all() and ref["g_grid"].abs().max() > 0


# ---- 2. the default accumulator (fp64 LDS atomics; the classic calls take the one-launch form) ------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_default_accumulator_within_one_bf16_ulp(cuda, name):
    """dL/d input of the default accumulator depends on the arrival order by at most one fp32 ulp (include/tpspp.h): after
    the rounding to bf16 at most one bf16 ulp from the fp32 call's result rounded once.  dL/d score and dL/d grid do not depend
    on the accumulator: bit-equal; dL/d control points bit-equal to the fp32 call of the same form (the one-launch form sums
    other chains than the two-kernel form, so it is compared with the fp32 one-launch call)."""
    c = all_cases()[name]
    ref = raw_bwd(cuda, c, F32, c.flags)
    got = raw_bwd(cuda, c, BF, c.flags)
    assert ref["rc"] == 0 and got["rc"] == 0, _lib.lib().tpspp_last_error()
    for k in ("g_in0", "g_in1"):
        if ref[k] is not None:
            assert got[k].dtype == BF and int(bf16_ulps(got[k], ref[k].bfloat16()).max()) <= 1, k
    for k in ("g_ctrl", "g_score", "g_grid"):
        if ref[k] is not None:
            assert same_bits(got[k], ref[k]), k


# ---- 3. against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cl_3x32x100", "pp_16x64"])
def test_against_float64_autograd(cuda, name):
    """CPU float64 autograd through F.grid_sample on the widened inputs and the forward's fp32 grid, the parameter chain in
    float64 (the composition of tests/test_gpu_backward.py).  Bounds: that file's for the fp32 kernel -- dL/d input 2e-5 of
    the largest entry, dL/d control points 2e-5 (classic) / 2e-4 (TPS_PP), dL/d score 2e-4 -- plus, element by element,
    2^-8 relative for the one bf16 rounding of dL/d input.
    Observed on an MI355X (worst element, as a fraction of its bound; the margin is the rest): cl_3x32x100 dL/d input 0.92
    (max error 1.4e-2), dL/d control points 0.63; pp_16x64 dL/d input 0.90 / 0.91 (max error 2.2e-2 / 2.0e-2), dL/d control
    points 0.003, dL/d score 0.005.  The fp32 outputs have the fp32 kernel's bits (test 1), so their figures are that
    kernel's; in dL/d input the bf16 rounding (2^-9 relative at worst) fills half of its term and the fp32 kernel's own error
    part of the absolute term."""
    c = all_cases()[name]
    got = raw_bwd(cuda, c, BF, c.flags)
    assert got["rc"] == 0
    N, (Ho, Wo) = c.N, c.out_hw
    n = Ho * Wo
    with torch.enable_grad():
        gd = got["grid"].cpu().double().reshape(N, Ho, Wo, 2).requires_grad_(True)
        i0 = c.in0.double().requires_grad_(True)
        L = (Fn.grid_sample(i0, gd, padding_mode="border", align_corners=True) * c.g0.double()).sum()
        if c.in1 is not None:
            i1 = c.in1.double().requires_grad_(True)
            L = L + (Fn.grid_sample(i1, gd, padding_mode="border", align_corners=True) * c.g1.double()).sum()
        L.backward()
    gg = gd.grad.reshape(N, n, 2)
    if c.classic:
        rows = c.P.double()[None].expand(N, -1, -1)
    else:
        rows = torch.cat([torch.ones(N, n, 1, dtype=torch.float64), c.xy.double()[None].expand(N, -1, -1),
                          c.P.double()[None] * (c.score.double() * 0.5 + 1)], 2)
    gT = torch.matmul(rows.transpose(1, 2), gg)                                     # (N, K, 2)
    g_ctrl = torch.matmul(c.inv.double().t()[None], gT)[:, :F]
    worst = {}

    def check(what, g, want, rtol, rounding):
        g, want = g.cpu().double(), want.double()
        bound = rtol * want.abs().max() + (2.0 ** -8 * want.abs() if rounding else 0.0)
        err = (g - want).abs()
        worst[what] = float((err / bound).max())
        print(f"{name} {what}: max err {float(err.max()):.3e}, worst element at {worst[what]:.3f} of its bound")
        assert bool((err <= bound).all()), (what, worst[what])

    check("dL/d in0", got["g_in0"], i0.grad, 2e-5, True)
    if c.in1 is not None:
        check("dL/d in1", got["g_in1"], i1.grad, 2e-5, True)
    check("dL/d control points", got["g_ctrl"], g_ctrl, 2e-5 if c.classic else 2e-4, False)
    if c.score is not None:
        T = torch.matmul(c.inv.double()[None], torch.cat((c.ctrl.double(), torch.zeros(N, 3, 2, dtype=torch.float64)), 1))
        g_score = 0.5 * c.P.double()[None] * torch.matmul(gg, T[:, 3:].transpose(1, 2))
        check("dL/d score", got["g_score"], g_score, 2e-4, False)


# ---- 4. special values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [("pp_16x64", 0), ("pp_16x64", FIX), ("cl_3x32x100", 0), ("cl_3x32x100", FIX)])
def test_non_finite_gradient_poisons_what_the_fp32_kernel_poisons(cuda, name, flags):
    import copy
    c = copy.copy(all_cases()[name])
    c.g0 = c.g0.clone()
    c.g0[1, 0, 5, 7] = float("inf")
    c.g0[0, c.g0.shape[1] - 1, 3, 2] = float("nan")
    ref, got = raw_bwd(cuda, c, F32, flags), raw_bwd(cuda, c, BF, flags)
    assert ref["rc"] == 0 and got["rc"] == 0
    for k in ("g_in0", "g_in1"):
        if ref[k] is not None:
            assert torch.equal(torch.isnan(got[k]), torch.isnan(ref[k])), k
            assert torch.equal(torch.isinf(got[k]), torch.isinf(ref[k].bfloat16())), k
    assert torch.isnan(ref["g_in0"]).any() and not torch.isnan(ref["g_in0"]).all()


def test_mixed_magnitudes_match_the_fixed_point_fp32_result_rounded_once(cuda):
    """1e-3 next to 1e3 on one tap: neighbouring output pixels share input pixels, the planes are summed exactly."""
    import copy
    c = copy.copy(all_cases()["pp_16x64"])
    g = torch.full(c.g0.shape, 1e-3)
    g[..., ::2] = 1e3
    c.g0 = (g * c.g0.float().sign()).to(BF)
    ref, got = raw_bwd(cuda, c, F32, FIX), raw_bwd(cuda, c, BF, FIX)
    assert ref["rc"] == 0 and got["rc"] == 0
    assert same_bits(got["g_in0"], ref["g_in0"].bfloat16()) and same_bits(got["g_in1"], ref["g_in1"].bfloat16())
    assert same_bits(got["g_ctrl"], ref["g_ctrl"]) and same_bits(got["g_score"], ref["g_score"])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,what", [
    (("rf_64x200", 2, 3, (64, 200), (64, 200), True), "4096 output pixels"),    # classic 64x200: HBM accumulation in fp32
    (("rf_96x64", 2, 2, (96, 64), (16, 64), False), "more than 4096 pixels"),
    (("rf_15x21", 2, 2, (15, 21), (16, 64), False), "multiple of 8"),
], ids=["64x200", "96x64", "15x21"])
def test_refused_shapes_return_einval_and_touch_nothing(cuda, args, what):
    got = raw_bwd(cuda, Case(*args), BF, 0, prefill=float("nan"))
    msg = _lib.lib().tpspp_last_error().decode()
    assert got["rc"] == -22 and "TPSPP_IO_BF16" in msg and what in msg, (got["rc"], msg)
    for k in ("g_in0", "g_in1", "g_ctrl", "g_score", "ws"):
        if got[k] is not None:
            assert torch.isnan(got[k]).all(), k


def test_mixed_dtypes_raise_type_error(cuda):
    c = all_cases()["pp_one_input_16x64"]
    d = lambda t: t.to(cuda)                                                        # noqa: E731
    grid = torch.zeros((c.N, 1024, 2), device=cuda)
    with pytest.raises(TypeError, match="share their dtype"):
        ops.warp_backward(d(c.g0).float(), d(c.in0), grid, d(c.ctrl), d(c.inv), d(c.P), c.out_hw, P_xy=d(c.xy))
    with pytest.raises(TypeError, match="share their dtype"):
        ops.warp_backward(d(c.g0), d(c.in0), grid, d(c.ctrl), d(c.inv), d(c.P), c.out_hw, P_xy=d(c.xy),
                          in1=d(c.in0).float(), g_out1=d(c.g0))


# ---- 6. autograd and modules -----------------------------------------------------------------------------------------------
@pytest.fixture
def fixed_point_default():
    """warp_autograd passes no accumulator flag: the process-wide default makes its backward the order-independent one."""
    _lib.lib().tpspp_warp_bwd_set_accumulator(1)
    yield
    _lib.lib().tpspp_warp_bwd_set_accumulator(0)


@pytest.mark.parametrize("name", ["pp_16x64", "cl_3x32x100"])
def test_warp_autograd_on_bf16_leaves(cuda, name, fixed_point_default):
    c, ref = all_cases()[name], reference(cuda, name)
    d = lambda t, grad=False: None if t is None else t.to(cuda).requires_grad_(grad)     # noqa: E731
    in0, in1, ctrl, score = d(c.in0, True), d(c.in1, True), d(c.ctrl, True), d(c.score, True)
    inv, P, xy = d(c.inv), d(c.P), d(c.xy)
    if c.classic:
        Pt, flags = ops.prepare_mirror_table(P, c.out_hw)
        flags |= ops.TABLE_MIRROR4 if ops.table_mirror_symmetry(c.P, c.out_hw, F) else 0
    else:
        Pt, flags = ops.transpose_p_hat(P), 0
    # the saved grid: fp32, the bits of the fp32 forward for the same control points
    with torch.no_grad():
        g16 = ops.warp(in0.detach(), ctrl.detach(), inv, P, c.out_hw, P_xy=xy, score=None if score is None else score.detach(),
                       in1=None if in1 is None else in1.detach(), want_grid=True, P_hat_t=Pt, table_flags=flags)[2]
    assert g16.dtype == F32 and same_bits(g16, ref["grid"])
    out = ops.warp_autograd(in0, ctrl, inv, P, c.out_hw, P_xy=xy, score=score, in1=in1, P_hat_t=Pt, table_flags=flags)
    outs = out if isinstance(out, tuple) else (out,)
    assert all(o.dtype == BF for o in outs)
    L = (outs[0] * d(c.g0)).sum(dtype=F32)
    if in1 is not None:
        L = L + (outs[1] * d(c.g1)).sum(dtype=F32)
    L.backward()
    assert in0.grad.dtype == BF and same_bits(in0.grad, ref["g_in0"].bfloat16())
    assert ctrl.grad.dtype == F32 and same_bits(ctrl.grad, ref["g_ctrl"])
    if in1 is not None:
        assert in1.grad.dtype == BF and same_bits(in1.grad, ref["g_in1"].bfloat16())
        assert score.grad.dtype == F32 and same_bits(score.grad, ref["g_score"])


def _tps_pp(cuda):
    """(Train backend "hip_all": every layer of the regressor on this package's kernels, which are bitwise reproducible, so
    that the fp32 outputs of two modules can be compared bit for bit; the library kernels of the "torch" backend pick their
    algorithm per call.)"""
    m = TPS_PP().to(cuda).train().set_train_backend("hip_all")
    sd = cases.synth_state(m.state_dict(), 4, cases.tpspp_state_rule, cases.TPSPP_KEEP)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


def test_tps_pp_trains_with_bf16_maps_through_the_warp(cuda):
    inp = cases.g4_inputs("ResNet45v2")                                # (values rounded to bf16: both runs see the same numbers)
    x32, outs32 = rb(inp["x"]).float().to(cuda), [rb(o).float().to(cuda) for o in inp["outs"]]
    assert x32.shape[0] == 2
    before = _tps_pp(cuda)(x32, outs32)                                 # a module built before the setter is ever called
    m = _tps_pp(cuda)
    assert m.set_train_io_dtype(BF) is m
    x, outs = x32.to(BF).requires_grad_(True), [o.to(BF).requires_grad_(True) for o in outs32]
    res = m(x, outs)
    assert res["output"].dtype == BF and res["mp_img"].dtype == BF and res["output"].requires_grad
    (res["output"].float().square().mean() + res["mp_img"].float().square().mean()).backward()
    assert x.grad.dtype == BF and all(o.grad.dtype == BF for o in outs)
    assert torch.isfinite(x.grad.float()).all() and x.grad.float().abs().max() > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert m.TPE.localization_fc2.bias.grad.dtype == F32 and m.TPE.localization_fc2.bias.grad.abs().max() > 0
    # same control points and score (the regressor saw the same fp32 numbers), so mp_img is the fp32 interpolation of the
    # same bf16-exact pixels rounded once (2^-9 relative at worst); `output` also carries the rounding of feat_grid to bf16
    assert (res["mp_img"].float() - before["mp_img"]).abs().max() <= 2.0 ** -8 * x32.abs().max()
    assert (res["output"].float() - before["output"]).abs().max() <= 2.0 ** -6 * before["output"].abs().max()
    # unset: fp32 as before, bit for bit
    m.set_train_io_dtype(None)
    xg = x32.clone().requires_grad_(True)
    again = m(xg, outs32)
    assert again["output"].dtype == F32 and again["mp_img"].dtype == F32
    for k in ("output", "mp_img"):
        assert same_bits(again[k], before[k]), (k, float((again[k] - before[k]).abs().max()))
    again["output"].square().mean().backward()
    assert xg.grad.dtype == F32


def test_tps_pp_bf16_maps_with_the_default_train_backend(cuda):
    """The regressor as the PyTorch composition (train backend "torch"): it still gets fp32 inputs; dtypes only."""
    inp = cases.g4_inputs("ResNet45v2")
    m = _tps_pp(cuda).set_train_backend("torch").set_train_io_dtype(BF)
    x, outs = rb(inp["x"]).to(cuda).requires_grad_(True), [rb(o).to(cuda).requires_grad_(True) for o in inp["outs"]]
    res = m(x, outs)
    assert res["output"].dtype == BF and res["mp_img"].dtype == BF and res["pc_score"].dtype == F32
    (res["output"].float().square().mean() + res["mp_img"].float().square().mean()).backward()
    assert x.grad.dtype == BF and all(o.grad.dtype == BF for o in outs) and torch.isfinite(x.grad.float()).all()
    assert all(p.grad is not None and p.grad.dtype == F32 and torch.isfinite(p.grad).all() for p in m.parameters())


def test_tps_preprocessor_trains_with_a_bf16_image(cuda):
    img32 = rb(cases.g1_inputs()["img"][:2]).float().to(cuda)
    torch.manual_seed(3)
    p = TPSPreprocessor(20, (32, 100), (32, 100), 3).to(cuda).train()
    p(img32)                                         # (the library convolutions of the localisation network choose their
    before = p(img32)                                # algorithm on the first call)
    assert before.dtype == F32
    assert p.set_train_io_dtype(BF) is p
    img = img32.to(BF).requires_grad_(True)
    out = p(img)
    assert out.dtype == BF and out.requires_grad
    out.float().square().mean().backward()
    assert img.grad.dtype == BF and torch.isfinite(img.grad.float()).all() and img.grad.float().abs().max() > 0
    assert p.LocalizationNetwork.localization_fc2.bias.grad.abs().max() > 0
    assert (out.float() - before).abs().max() <= 2.0 ** -8 * img32.abs().max()      # one rounding of an interpolated pixel
    p.set_train_io_dtype(None)
    again = p(img32)
    assert again.dtype == F32 and same_bits(again, before), float((again - before).abs().max())


def test_a_refused_geometry_raises_at_forward(cuda):
    """64x200 is more than 4096 output pixels: the bf16 backward does not serve it, and the forward says so."""
    c = O.classic_constants(F, (64, 200))
    img = torch.zeros((2, 3, 64, 200), device=cuda, dtype=BF, requires_grad=True)
    ctrl = torch.from_numpy(O.classic_initial_ctrl(F)[None].repeat(2, 0)).to(cuda)
    with pytest.raises(_lib.TpsppError, match="TPSPP_IO_BF16"):
        ops.warp_autograd(img, ctrl, torch.from_numpy(c["inv_delta_C"]).to(cuda), torch.from_numpy(c["P_hat"]).to(cuda), (64, 200))


# ---- 7. guard bands and poison ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cl_3x32x100", "pp_16x64"])
def test_guarded_run_equals_plain_run(cuda, name):
    """Inputs between NaN bands, every output and the workspace (exactly tpspp_warp_bwd_workspace_floats) from poisoned
    buffers with guard bands: the bands stay intact, every returned element was written, the bits equal the plain run's."""
    c = all_cases()[name]

    def fn(put):
        in0, in1, g0, g1 = (None if t is None else put(t) for t in (c.in0, c.in1, c.g0, c.g1))
        inv, P, ctrl = put(c.inv), put(c.P), put(c.ctrl)
        xy, score = (None if t is None else put(t) for t in (c.xy, c.score))
        grid = ops.warp(in0.float(), ctrl, inv, P, c.out_hw, P_xy=xy, score=score, in1=None if in1 is None else in1.float(),
                        want_grid=True)[2]
        Pt = ops.transpose_p_hat(P) if c.classic else None
        return [ops.warp_backward(g0, in0, grid, ctrl, inv, P, c.out_hw, P_xy=xy, score=score, in1=in1, g_out1=g1,
                                  P_hat_t=Pt, fixed_point=True, two_kernels=two) for two in (False, True)]
    got = run_twice(cuda, fn)
    ref = reference(cuda, name)
    assert got[0][0].dtype == BF and same_bits(got[0][0], ref["g_in0"].bfloat16()) and same_bits(got[0][2], ref["g_ctrl"])
    # the default accumulator (the one-launch form on the classic call): guards and poison only
    run_twice(cuda, lambda put: fn_default(put, c), bitwise=False)


def fn_default(put, c):
    in0, in1, g0, g1 = (None if t is None else put(t) for t in (c.in0, c.in1, c.g0, c.g1))
    inv, P, ctrl = put(c.inv), put(c.P), put(c.ctrl)
    xy, score = (None if t is None else put(t) for t in (c.xy, c.score))
    grid = ops.warp(in0.float(), ctrl, inv, P, c.out_hw, P_xy=xy, score=score, in1=None if in1 is None else in1.float(),
                    want_grid=True)[2]
    Pt = ops.transpose_p_hat(P) if c.classic else None
    return ops.warp_backward(g0, in0, grid, ctrl, inv, P, c.out_hw, P_xy=xy, score=score, in1=in1, g_out1=g1, P_hat_t=Pt)
