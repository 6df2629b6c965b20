"""-m gpu: every route of tpspp_warp_bwd (tests/warp_bwd_route_cases.py) on buffers of this test's own, so that the workspace
can be read back (dL/d grid is its first N n 2 floats) and tensors that are not wanted are NULL.

Comparison A: exactly representable data -- every output of every case EQUALS the float64 reference (signed zeros aside),
whatever the order of the atomics; bf16 dL/d input equals the exact sum rounded once.  Comparison B: real data on one or two
cases per sampling family, inside bars derived from the kernels' arithmetic (k_grid, l_chain and stage1_bars / stage2 of the
case module: none is a measured number).  Two-kernel cases run twice: dL/d control points, dL/d score and dL/d grid must
repeat bit for bit on every route, dL/d input on the fixed-point one.

Observed on an MI355X, worst |error| / bound per route of comparison B: see DESIGN.md, "The warp backward's routes"."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
import warp_bwd_route_cases as W
from tps_pp_amd import TPSPreprocessor, _lib, constants, ops, synth

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


def run(cuda, c, d, guard=None):
    """One call of the entry point for case `c` on data `d`.  Outputs and the workspace (exactly
    tpspp_warp_bwd_workspace_floats) start as NaN -- or, with `guard`, as poison between guard bands, the inputs between NaN
    bands.  -> dict of the raw device tensors (g_in0, g_in1, g_ctrl, g_score in the call's layout, g_grid, ws)."""
    put = guard.input if guard is not None else (lambda t: t.to(cuda))
    new = (lambda shape, dt: torch.empty(shape, dtype=dt, device=cuda)) if guard is not None else \
        (lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=cuda))
    io = BF if c.bf16 else F32
    tt = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))     # noqa: E731
    N, n, F = c.N, W.n_of(c), c.F
    in0, g0 = put(tt(d["in0"]).to(io)), put(tt(d["g0"]).to(io))
    in1, g1 = (put(tt(d["in1"]).to(io)), put(tt(d["g1"]).to(io))) if c.C1 else (None, None)
    grid, inv, ph = put(tt(d["grid"])), put(tt(d["inv"])), put(tt(d["ph"]))
    xy = put(tt(d["xy"])) if c.table else None
    score = None
    if c.score:
        score = put(tt(d["score"].transpose(0, 2, 1) if c.score == 2 else d["score"]))
    T = put(tt(d["T"])) if c.score else None
    pt = None
    if c.transposed:
        flat = np.ascontiguousarray(d["ph"].T).reshape(-1)
        if c.pt_offset:
            pt = put(tt(np.concatenate([np.zeros(1, np.float32), flat, np.zeros(3, np.float32)])))[1:1 + flat.size]
            assert pt.data_ptr() % 16 == 4
        else:
            pt = put(tt(flat))
    numel0 = N * c.C0 * c.in0[0] * c.in0[1]
    g_in0 = None
    if c.need0:
        g_in0 = new((numel0 + 4,), io)[1:1 + numel0] if c.misalign0 else new((numel0,), io)
        g_in0 = g_in0.view(N, c.C0, *c.in0)
        assert (g_in0.data_ptr() % 16 != 0) == bool(c.misalign0)
    g_in1 = new((N, c.C1) + c.in1, io) if (c.C1 and c.need1) else None
    g_ctrl = new((N, F, 2), F32)
    g_score = new(tuple(score.shape), F32) if (c.score and c.gscore) else None
    nws = int(_lib.lib().tpspp_warp_bwd_workspace_floats(N, *c.out))
    ws = new((nws,), F32)
    flags = (ops.BWD_FIXED_POINT if c.fixed else 0) | (ops.BWD_TWO_KERNELS if c.two else 0) | (ops.IO_BF16 if c.bf16 else 0) | \
        (ops.SCORE_TRANSPOSED if c.score == 2 else 0)
    ops._call("tpspp_warp_bwd", in0, g0, in0, c.C0, *c.in0, g1, in1, c.C1, *(c.in1 or (0, 0)), grid, T, inv, ph, ph.shape[1], xy,
              score, pt, flags, N, F, *c.out, g_in0, g_in1, g_ctrl, g_score, ws, nws)
    torch.cuda.synchronize()
    return dict(g_in0=g_in0, g_in1=g_in1, g_ctrl=g_ctrl, g_score=g_score, g_grid=ws[:N * n * 2].view(N, n, 2), ws=ws)


def host(c, out, k):
    """Output `k` of a run as float64 numpy in the reference's layout (dL/d score: (N, n, F))."""
    t = out[k]
    if t is None:
        return None
    a = t.detach().double().cpu().numpy()
    return a.transpose(0, 2, 1) if (k == "g_score" and c.score == 2) else a


def bits(t):
    return t.contiguous().view({F32: torch.int32, BF: torch.int16}[t.dtype])


def check_repeat(c, r, first, second):
    for k in ("g_ctrl", "g_score", "g_grid") + (("g_in0", "g_in1") if (r.family == "lds2" and not r.f64) else ()):
        if first[k] is not None:
            assert torch.equal(bits(first[k]), bits(second[k])), f"{c.name} [{r}]: {k} differs between two runs"


# ---- comparison A -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(W.CASES))
def test_every_route_is_exact_on_representable_data(cuda, name):
    c = W.CASES[name]
    r = W.route_of(c)
    assert str(r) == W.ROUTES[name]
    d = W.make_data(c)
    ref = W.reference(d)
    assert max(W.exact_bits(d, ref).values()) < 2 ** 24
    out = run(cuda, c, d)
    msgs = []
    for k in ("g_in0", "g_in1", "g_grid", "g_ctrl", "g_score"):
        got = host(c, out, k)
        if k == "g_in0":
            assert (got is None) == (not c.need0)
        if k == "g_in1":
            assert (got is None) == (not (c.C1 and c.need1))
        if k == "g_score":
            assert (got is None) == (not (c.score and c.gscore))
        if got is None:
            continue
        want = W.round_bf16(ref[k]) if (c.bf16 and k.startswith("g_in")) else ref[k]
        msgs.append(W.report(c, r, d, k, got, want))
    msgs = [m for m in msgs if m]
    assert not msgs, "\n".join(msgs)
    if r.params:
        check_repeat(c, r, out, run(cuda, c, d))


# ---- comparison B -----------------------------------------------------------------------------------------------------------
def forward_grid(cuda, c, d):
    """The forward kernel's own fp32 grid for the case's real tables and control points."""
    dv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)     # noqa: E731
    return ops.warp(dv(d["in0"]), dv(d["ctrl"]), dv(d["inv"]), dv(d["ph"]), c.out, P_xy=dv(d["xy"]) if c.table else None,
                    score=dv(d["score"]) if c.score else None, in1=dv(d["in1"]) if c.C1 else None, want_grid=True)[2]


def ratios(c, r, d, what, got, want, bound):
    m = W.report(c, r, d, what, got, want, bound)
    worst = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print(f"RATIO {r.family}{' bf16' if c.bf16 else ''}{'' if r.f64 or r.family != 'lds2' else ' fix'} | {c.name} | {what} | "
          f"{worst:.3f} | max error {float(np.abs(got - want).max()):.3e}")
    return m


@pytest.mark.parametrize("name", W.REAL)
def test_real_data_inside_the_derived_bars(cuda, name):
    """Stage 1: dL/d input and dL/d grid against float64 on the forward's fp32 grid, element by element (stage1_bars).
    Stage 2: dL/d control points and dL/d score against float64 computed from the KERNEL's dL/d grid (stage2): the parameter
    arithmetic alone.  k_grid and l_chain were fixed from the kernel source before the first run; observed ratios: DESIGN.md."""
    c = W.real_case(name)
    r = W.route_of(c)
    assert r.family == W.route_of(W.CASES[name]).family and c.N == 3
    d = W.make_real(c)
    d["grid"] = forward_grid(cuda, c, d).cpu().numpy().reshape(c.N, -1, 2)
    assert np.isfinite(d["grid"]).all()
    # gentle, folded, clamped: the share of pixels with a clamped coordinate grows with the image's amplitude; the first image
    # is mostly inside, the last has at least a fifth outside (and never everything: interior taps remain)
    out_of = [float(((np.abs(d["grid"][b]) >= 1).any(-1)).mean()) for b in range(3)]
    print(f"CLAMPED {c.name}: {out_of}")
    assert out_of[0] < 0.5 and 0.2 < out_of[2] < 1.0 and out_of[0] < out_of[2], out_of
    ref = W.reference(d)
    bars = W.stage1_bars(c, r, ref)
    out = run(cuda, c, d)
    msgs = [ratios(c, r, d, k, host(c, out, k), ref[k], bars[k]) for k in ("g_in0", "g_in1", "g_grid") if out[k] is not None]
    gg = host(c, out, "g_grid")
    (g_ctrl, b_ctrl), (g_score, b_score) = W.stage2(d, c, r, gg)
    msgs.append(ratios(c, r, d, "g_ctrl", host(c, out, "g_ctrl"), g_ctrl, b_ctrl))
    if out["g_score"] is not None:
        msgs.append(ratios(c, r, d, "g_score", host(c, out, "g_score"), g_score, b_score))
    msgs = [m for m in msgs if m]
    assert not msgs, "\n".join(msgs)
    if r.params:
        check_repeat(c, r, out, run(cuda, c, d))


# ---- guard bands and poison: kernels A' and A ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds: 17x33 + 17x9, C=9 | 17", "lds: g_in0 one float off", "atomics: C0=9 C1=3 (blockIdx.y split)",
                                  "atomics: 129x128 plane, n=30"])
def test_guarded_run_writes_every_output_and_nothing_else(cuda, name):
    """Inputs between NaN bands; outputs and the workspace from poisoned buffers between guard bands: the guards stay intact,
    no output element keeps its poison (kernel A zeroes dL/d input itself), and the values are still exact."""
    c = W.CASES[name]
    r = W.route_of(c)
    assert r.family == name.split(":")[0]
    d = W.make_data(c)
    ref = W.reference(d)
    with GA.guarded(cuda) as g:
        out = run(cuda, c, d, guard=g)
        served = g.check([out[k] for k in ("g_in0", "g_in1", "g_ctrl", "g_score", "g_grid")], require_guarded=True)
    assert served >= 4 and not g.fallthrough
    for k in ("g_in0", "g_in1", "g_grid", "g_ctrl", "g_score"):
        assert (out[k] is None) == (ref[k] is None), k
        if out[k] is not None:
            m = W.report(c, r, d, k, host(c, out, k), ref[k])
            assert m is None, m


# ---- the classic geometries above 4096 pixels, through autograd ---------------------------------------------------------------
@pytest.mark.parametrize("hw,C", [((48, 160), 3), ((64, 256), 1)], ids=["3x48x160", "1x64x256"])
def test_classic_rectifier_trains_at_the_large_geometries(cuda, hw, C):
    """TPSPreprocessor(20, hw, hw, C) in .train() at N = 2 -- an RGB rectifier at 48x160 (a ragged chunk of 3 of 8 channels in
    kernel A, three planes to zero) and a one-channel one at 64x256: the module's own backward runs, and `ops.warp_autograd`
    on its tables takes the `atomics` route with image and control-point gradients inside the stage-1 and stage-2 bars
    (float64 on the forward's fp32 grid; dL/d control points here come from the kernel's dL/d grid, which autograd does not
    return, so its stage-1 bar is carried through |row| and |inv_delta_c| and added)."""
    N, F = 2, 20
    torch.manual_seed(5)
    m = TPSPreprocessor(F, hw, hw, C).to(cuda).train()
    img_np = synth.smooth_image((N, C) + hw, f"routes.mod.{hw}").astype(np.float32)
    x = torch.from_numpy(img_np).to(cuda).requires_grad_(True)
    m(x).square().mean().backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    gen = m.GridGenerator
    Pt, flags = gen.prepared_table()
    c = W.case(f"module {C}x{hw[0]}x{hw[1]}", N, C, hw, hw, F=F, table=0, transposed=1)
    ctrl_np = (constants.classic_initial_ctrl(F)[None] + W.AMPS[:N, None, None] * synth.dyadic((N, F, 2), "routes.mod.ctrl", 1)).astype(np.float32)
    g_np = synth.dyadic((N, C) + hw, f"routes.mod.g.{hw}", 1)
    img, ctrl = torch.from_numpy(img_np).to(cuda).requires_grad_(True), torch.from_numpy(ctrl_np).to(cuda).requires_grad_(True)
    with torch.no_grad():
        grid = ops.warp(img.detach(), ctrl.detach(), gen.inv_delta_C, gen.P_hat, hw, want_grid=True, P_hat_t=Pt, table_flags=flags)[2]
    r = ops.warp_backward_route(torch.from_numpy(g_np).to(cuda), img.detach(), grid, ctrl.detach(), gen.inv_delta_C, gen.P_hat, hw,
                                P_hat_t=Pt)
    assert r.family == "atomics" and r.params_key == (24, 0, 1, 0, 0), str(r)
    out = ops.warp_autograd(img, ctrl, gen.inv_delta_C, gen.P_hat, hw, P_hat_t=Pt, table_flags=flags)
    (out * torch.from_numpy(g_np).to(cuda)).sum().backward()
    d = dict(case=c, in0=img_np, g0=g_np, in1=None, g1=None, grid=grid.cpu().numpy().reshape(N, -1, 2),
             ph=gen.P_hat.cpu().numpy(), xy=None, inv=gen.inv_delta_C.cpu().numpy(), T=None, score=None)
    tot, mass, cnt, gg, ag = W.sample_reference(d["in0"], d["g0"], d["grid"], 8)
    ref = dict(g_in0=tot, mass0=mass, cnt0=cnt, abs_grid=ag, g_grid=gg)
    bars = W.stage1_bars(c, r, ref)
    msgs = [ratios(c, r, d, "g_in0", img.grad.double().cpu().numpy(), tot, bars["g_in0"])]
    (g_ctrl, b_ctrl), _ = W.stage2(d, c, r, gg)
    rows, _ = W.rows_of(d)
    carried = np.einsum("kf,bkx->bfx", np.abs(d["inv"]).astype(np.float64), np.einsum("bpk,bpx->bkx", np.abs(rows), bars["g_grid"]))[:, :F]
    msgs.append(ratios(c, r, d, "g_ctrl", ctrl.grad.double().cpu().numpy(), g_ctrl, b_ctrl + carried))
    msgs = [m_ for m_ in msgs if m_]
    assert not msgs, "\n".join(msgs)
