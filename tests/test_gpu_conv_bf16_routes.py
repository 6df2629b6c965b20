"""-m gpu: every bf16 convolution kernel `tpspp_conv2d_bf16_fwd` can pick, by route (tests/conv_bf16_route_cases.py holds the
table, tests/test_conv_bf16_route_host.py that it reaches all of them).  Every launch asserts the route `ops.conv2d_bf16_route`
names first, then runs: the case's kernel with the tuning bits clear and, for a specialised case, the tiled kernel it falls back
to with its bit set.  Inputs, weights, bias and residual sit between NaN bands and every output comes from
tests/guarded_alloc.py: nothing is written outside it and every element of it is written.

Two comparisons per case:

EXACT.  Integer-valued data (inputs in [-8, 8], weights in [-4, 4], bias and residual in [-64, 64], post-scale in
{-2, -1, 1, 2}, an integer post-shift) with K <= 4608: every operand is a bf16 number (in the three-term split hi is the value
and lo is 0) and every product and partial sum, in any order, is an integer below 2^24.  An fp32 output must equal the float64
reference bit for bit; a bf16 output must equal that reference rounded ONCE to bf16, to nearest even, bit for bit.  Sums beyond
256 that are odd are exact ties of that rounding, so the mode is tested wherever K is large enough to produce them (counted and
printed; required for K >= 64).  Each case runs its plain epilogue (bias, the case's activation) and the general one its route
accepts (the case's residual mode; on the tiled routes also the post-affine), on the specialised route and on its tiled
fallback: both must equal the reference, not just each other.

ROUNDING.  Dyadic reals, weights at 1 / sqrt(fan_in), a non-zero bias and a signed residual, against the float64 restatement of
the route's arithmetic (`conv_bf16_route_cases.conv_sum`: operands rounded to bf16, or hi*hi + hi*lo + lo*hi with
`ops._hi_lo`'s rule), the epilogue in float64.  The bars are the project's own: fp32 outputs of plain bf16 -- `within_bar` of
tests/test_gpu_train_primitives.py (relative L2 <= max(1e-5, 2 x PyTorch's fp32 composition on the GPU on the same rounded
operands), for the tensor and for every image); the three-term split -- tests/test_gpu_conv_bf16.py's 2e-5 of the tensor's scale;
bf16 outputs -- every element within one bf16 ulp of the reference (tests/test_gpu_conv_bf16.py's rule).  Every error is printed
with its bar."""
import pytest
import torch

import conv_bf16_route_cases as RC
import guarded_alloc as GA
from test_gpu_conv_routes import hold_bar
from tps_pp_amd import _lib, ops

pytestmark = pytest.mark.gpu


class Launcher:
    """One case on the device: guarded sources, weight, bias, residual and affine; `run` launches one epilogue under one tuning
    setting after asserting the route, checks the guards and the poison of its output and returns it as NCHW."""

    def __init__(self, cuda, c, d, g):
        self.c, self.g = c, g
        place = lambda t: g.input(t.to(cuda))      # noqa: E731
        self.srcs = [(RC.as_layout(x, s[5], place), s[3], s[4]) for x, s in zip(d["xs"], c.srcs)]
        self.arranged = RC.weights_of(c, d["w"].to(cuda), place=place).arranged
        self.bias, self.ps, self.pb = g.input(d["bias"]), g.input(d["post_scale"]), g.input(d["post_shift"])
        self.res = RC.as_layout(d["res"], c.res, place) if c.res else None

    def run(self, bits, act, res_mode, bias=True, post=False, want=None):
        c = self.c
        cw = ops.ConvWeightBf16(self.arranged, self.bias if bias else None, c.k, RC.cin_of(c), c.cout, self.ps if post else None,
                                self.pb if post else None, c.x3)
        args = (self.srcs, cw, c.stride, act, self.res if res_mode else None, res_mode,
                torch.float32 if c.out in ("f32", "blk32") else torch.bfloat16, c.out in ("blk", "blk32"))
        _lib.lib().tpspp_conv_set_tuning(bits)
        try:
            want = want or (c.fallback if bits else c.route)
            assert ops.conv2d_bf16_route(*args) == want, (c.name, bits)
            out = ops.conv2d_bf16(*args)
        finally:
            _lib.lib().tpspp_conv_set_tuning(0)
        self.g.check(out.t if isinstance(out, ops.Blocked) else out, require_guarded=True)
        return out.nchw() if isinstance(out, ops.Blocked) else out


def reference(c, d, act, res_mode, bias, post, y):
    """The epilogue on the convolution sum `y`, in y's dtype on y's device."""
    to = lambda t: t.to(device=y.device, dtype=y.dtype)      # noqa: E731
    return RC.epilogue(y, act, res_mode, to(d["bias"]) if bias else None, to(d["res"]) if res_mode else None,
                       to(d["post_scale"]) if post else None, to(d["post_shift"]) if post else None)


def hold_exact(label, got, want64, bad):
    """fp32: the float64 reference itself; bf16: that reference rounded once, to nearest even.  Bit for bit."""
    want = want64.to(got.dtype)           # integers below 2^24: float64 -> fp32 is exact, so the bf16 rounding happens once
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    same = got.detach().cpu().contiguous().view(it) == want.contiguous().view(it)
    n = int((~same).sum())
    print(f"{label}: {n} of {same.numel()} outputs differ from the float64 reference")
    if n:
        first = torch.nonzero(~same)[0].tolist()
        bad[label] = (n, first, got.cpu()[tuple(first)].item(), want64[tuple(first)].item())


def ties(want64):
    """Outputs that are exact ties of the bf16 rounding: integers beyond 256 that bf16 does not hold."""
    return int(((want64.abs() > 256) & (RC.rb(want64.float()).double() != want64)).sum())


def hold_rounding(label, c, got, want, lib32, bad):
    if got.dtype == torch.bfloat16:
        g, w = got.float().cpu().double(), want
        scale = float(w.abs().max())
        err, bar = (g - w).abs(), w.abs() * 2.0 ** -8 + 1e-6 * scale
        worst = float((err / bar).max())
        print(f"{label}: bf16 output, largest error / (one bf16 ulp of the reference) {worst:.3f}, bar 1")
        if not bool((err <= bar).all()):
            bad[label] = (worst, 1.0)
    elif c.x3:
        e, bar = float((got.cpu().double() - want).abs().max()), 2e-5 * float(want.abs().max())
        print(f"{label}: three-term split, max abs error {e:.3e}, bar {bar:.3e}")
        if not e <= bar:
            bad[label] = (e, bar)
    else:
        hold_bar(label, got, lib32, want, bad)


@pytest.mark.parametrize("c", RC.CASES, ids=[c.name for c in RC.CASES])
def test_exact_on_integers(cuda, c):
    d = RC.make_inputs(c, True)
    y = RC.conv_sum(c, d["xs"], d["w"])
    assert y.abs().max() > 0
    bad = {}
    with GA.guarded(cuda) as g:
        L = Launcher(cuda, c, d, g)
        for bits, res_mode, post, route in RC.runs_of(c):
            want = reference(c, d, c.relu, res_mode, True, post, y)
            got = L.run(bits, c.relu, res_mode, True, post, route)
            assert got.shape == want.shape
            label = f"{c.name} res_mode={res_mode} post={post} bits={bits}"
            if got.dtype == torch.bfloat16:
                n = ties(want)
                print(f"{label}: {n} outputs are ties of the bf16 rounding")
                assert n > 0 or RC.cin_of(c) * c.k * c.k < 64, label
            hold_exact(label, got, want, bad)
    assert not bad, bad


@pytest.mark.parametrize("c", RC.CASES, ids=[c.name for c in RC.CASES])
def test_rounding_against_float64(cuda, c):
    d = RC.make_inputs(c, False)
    want = reference(c, d, c.relu, c.res_mode, True, False, RC.conv_sum(c, d["xs"], d["w"]))
    lib32 = None
    if not c.x3 and c.out == "f32":
        lib32 = reference(c, d, c.relu, c.res_mode, True, False, RC.conv_sum(c, d["xs"], d["w"], torch.float32, cuda))
    bad = {}
    with GA.guarded(cuda) as g:
        L = Launcher(cuda, c, d, g)
        for bits in (0, c.bits) if c.bits else (0,):
            hold_rounding(f"{c.name} bits={bits}", c, L.run(bits, c.relu, c.res_mode), want, lib32, bad)
    assert not bad, bad


@pytest.mark.parametrize("form", list(RC.EPILOGUE_SHAPES))
def test_every_epilogue(cuda, form):
    """activation {none, ReLU, GELU} x residual {none, after, before} x post-affine x bias on one tiled shape per (kernel, stride)
    form and one in the three-term split: bit for bit on integers without GELU, within the bar on reals with it.  The residual is
    fp32 NCHW (plain) so that every combination reads what the reference reads."""
    c = RC.EPILOGUE_SHAPES[form]._replace(res="f32", res_mode=1)
    bad = {}
    for exact in (True, False):
        d = RC.make_inputs(c, exact)
        y = RC.conv_sum(c, d["xs"], d["w"])
        y32 = None if exact or c.x3 else RC.conv_sum(c, d["xs"], d["w"], torch.float32, cuda)
        with GA.guarded(cuda) as g:
            L = Launcher(cuda, c, d, g)
            for act, res_mode, post, bias in RC.EPILOGUES:
                if (act == 2) == exact:
                    continue
                label = f"{form}: act={act} res_mode={res_mode} post={post} bias={bias}"
                got = L.run(0, act, res_mode, bias, post, want=c.route)
                want = reference(c, d, act, res_mode, bias, post, y)
                if exact:
                    hold_exact(label, got, want, bad)
                else:
                    hold_rounding(label, c, got, want, None if y32 is None else reference(c, d, act, res_mode, bias, post, y32), bad)
    assert not bad, bad
