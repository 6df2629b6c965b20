"""-m gpu: every fp32 convolution kernel `tpspp_conv2d_fwd` can pick, by route (tests/conv_route_cases.py holds the table,
tests/test_conv_route_host.py that it reaches all of them).  Each test asserts the route `ops.conv2d_route` names before it
launches, with tuning bit 0 off (the case's kernel) and on (the generic kernel).  Inputs and weights sit between NaN bands
and every output comes from tests/guarded_alloc.py: nothing is written outside it and every element of it is written.

Two comparisons per case:

EXACT.  Integer-valued data (inputs in [-8, 8], weights in [-4, 4], bias and residual in [-64, 64], post-scale in
{-2, -1, 1, 2}, an integer post-shift) with K <= 4608: every product and every partial sum, in any order, is an integer
below 2^24, so the output must equal the float64 reference bit for bit on every route.  Each case runs its plain epilogue
(bias, the case's activation: the kernels' fast path) and its general one (the case's residual mode and the post-affine).
A wrong index, a dropped chunk, a swapped tap or a misplaced store shows whatever its size.  GELU is not exact and is left
to the second comparison.

ROUNDING.  Dyadic reals, weights at 1 / sqrt(fan_in), a non-zero bias, a signed residual, against float64 `F.conv2d` on the
CPU with concatenation, nearest upsampling, activation, residual order and affine written out (`conv_route_cases`), held to
the project's bar (`within_bar` of tests/test_gpu_train_primitives.py): relative L2 error <= max(1e-5, 2 x the error of
PyTorch's fp32 composition on the GPU against the same float64), for the tensor and for every image of it.  Every error is
printed with its bar."""
import pytest
import torch
import torch.nn.functional as F

import conv_route_cases as RC
import guarded_alloc as GA
from test_gpu_train_primitives import within_bar
from tps_pp_amd import _lib, ops

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Launcher:
    """One case on the device: guarded sources and weights, `run` launches one epilogue under one tuning setting after
    asserting the route, and checks the guards and the poison of its output."""

    def __init__(self, cuda, c, d, g):
        self.c, self.g, self.d = c, g, d
        self.srcs = [(g.input(x), uh, uw) for x, (_, _, _, uh, uw) in zip(d["xs"], c.srcs)]
        cw = ops.prep_conv_weight(d["w"].to(cuda), src_channels=[s[0] for s in c.srcs])
        self.wt, self.tiled = g.input(cw.wt), None if cw.tiled is None else g.input(cw.tiled)
        self.bias, self.res = g.input(d["bias"]), g.input(d["res"])
        self.ps, self.pb = g.input(d["post_scale"]), g.input(d["post_shift"])

    def run(self, force_generic, act, res_mode, bias=True, post=False):
        c = self.c
        cw = ops.ConvWeight(self.wt, self.tiled, self.bias if bias else None, c.k, self.ps if post else None,
                            self.pb if post else None)
        _lib.lib().tpspp_conv_set_tuning(1 if force_generic else 0)
        try:
            want = RC.generic_route(c) if force_generic else c.route
            assert ops.conv2d_route(self.srcs, cw, c.stride) == want, c.name
            out = ops.conv2d(self.srcs, cw, c.stride, act, self.res if res_mode else None, res_mode)
        finally:
            _lib.lib().tpspp_conv_set_tuning(0)
        self.g.check(out, require_guarded=True)
        return out


def reference(c, d, act, res_mode, bias, post, y=None, dtype=torch.float64, device="cpu"):
    """float64 on the CPU (or, for the bar, PyTorch's fp32 composition on the GPU); `y`: the convolution sum if at hand."""
    to = lambda t: t.to(device=device, dtype=dtype)      # noqa: E731
    if y is None:
        y = RC.conv_sum(c, [to(x) for x in d["xs"]], to(d["w"]))
    return RC.epilogue(y, act, res_mode, to(d["bias"]) if bias else None, to(d["res"]) if res_mode else None,
                       to(d["post_scale"]) if post else None, to(d["post_shift"]) if post else None)


def hold_exact(label, got, want64, bad):
    same = bits(got) == bits(want64.float())
    n = int((~same).sum())
    print(f"{label}: {n} of {same.numel()} outputs differ from the float64 reference")
    if n:
        first = torch.nonzero(~same)[0].tolist()
        bad[label] = (n, first, got.cpu()[tuple(first)].item(), want64[tuple(first)].item())


def hold_bar(label, got, lib32, want, bad):
    """`within_bar` for the tensor and, with the same rule, for every image of it."""
    within_bar(label, got, lib32, want, bad)
    g, l, w = (t.detach().cpu().double().flatten(1) for t in (got, lib32, want))
    n = w.norm(dim=1)
    n = torch.where(n > 0, n, torch.ones_like(n))
    err, bar = (g - w).norm(dim=1) / n, (2 * (l - w).norm(dim=1) / n).clamp_min(1e-5)
    for i, (e, b) in enumerate(zip(err.tolist(), bar.tolist())):
        print(f"{label} image {i}: rel L2 {e:.3e}, bar {b:.3e}")
        if not e <= b:
            bad[f"{label} image {i}"] = (e, b)


@pytest.mark.parametrize("c", RC.CASES, ids=[c.name for c in RC.CASES])
def test_exact_on_integers(cuda, c):
    d = RC.make_inputs(c, True)
    y = RC.conv_sum(c, [x.double() for x in d["xs"]], d["w"].double())
    assert y.abs().max() > 0
    bad = {}
    with GA.guarded(cuda) as g:
        L = Launcher(cuda, c, d, g)
        for res_mode, post in ((0, False), (c.res_mode, True)):
            want = reference(c, d, c.relu, res_mode, True, post, y)
            for force in (0, 1):
                got = L.run(force, c.relu, res_mode, True, post)
                assert got.shape == want.shape
                hold_exact(f"{c.name} res_mode={res_mode} post={post} generic={force}", got, want, bad)
    assert not bad, bad


@pytest.mark.parametrize("c", RC.CASES, ids=[c.name for c in RC.CASES])
def test_rounding_against_float64(cuda, c):
    d = RC.make_inputs(c, False)
    want = reference(c, d, c.relu, c.res_mode, True, False)
    lib32 = reference(c, d, c.relu, c.res_mode, True, False, dtype=torch.float32, device=cuda)
    bad = {}
    with GA.guarded(cuda) as g:
        L = Launcher(cuda, c, d, g)
        for force in (0, 1):
            hold_bar(f"{c.name} generic={force}", L.run(force, c.relu, c.res_mode), lib32, want, bad)
    assert not bad, bad


@pytest.mark.parametrize("family", list(RC.EPILOGUE_SHAPES))
def test_every_epilogue(cuda, family):
    """activation {none, ReLU, GELU} x residual {none, after, before} x post-affine x bias on one shape of the family:
    bit for bit on integers without GELU, within the bar on reals with it."""
    c = RC.EPILOGUE_SHAPES[family]
    bad = {}
    for exact in (True, False):
        d = RC.make_inputs(c, exact)
        y = RC.conv_sum(c, [x.double() for x in d["xs"]], d["w"].double())
        y32 = None if exact else RC.conv_sum(c, [x.to(cuda) for x in d["xs"]], d["w"].to(cuda))
        with GA.guarded(cuda) as g:
            L = Launcher(cuda, c, d, g)
            for act, res_mode, post, bias in RC.EPILOGUES:
                if (act == 2) == exact:
                    continue
                label = f"{family}: act={act} res_mode={res_mode} post={post} bias={bias}"
                got = L.run(0, act, res_mode, bias, post)
                want = reference(c, d, act, res_mode, bias, post, y)
                if exact:
                    hold_exact(label, got, want, bad)
                else:
                    hold_bar(label, got, reference(c, d, act, res_mode, bias, post, y32, torch.float32, cuda), want, bad)
    assert not bad, bad
