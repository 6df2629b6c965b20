"""-m gpu: where the kernels read and write.  Every entry point runs at ragged and edge shapes twice on the same inputs:

  plain    inputs from `.to(cuda)`, ordinary allocation;
  guarded  inputs between NaN bands (`Guard.input`), every `torch.empty` / `torch.empty_like` of the wrappers served from
           poisoned buffers with 64 KiB guard bands (tests/guarded_alloc.py), modules and weight holders built fresh
           inside the context so that the grow-only caches are allocated at exactly the queried size.

Each case asserts (a) the guards are intact, (b) the returned float tensors hold no poison (every element was written),
(c) the guarded results equal the plain ones bit for bit (integers included).  No tolerance: every kernel here is
documented as deterministic -- except tpspp_warp_bwd's default accumulator (fp64 LDS atomics: "two runs may differ by one
fp32 ulp", include/tpspp.h), which is held to (a) and (b) and to (c) with `fixed_point=True` (this call only).

Shapes come from the existing case tables (imported, not retyped).  `SWEPT` names the entry points each case reaches;
tests/test_memory_safety_host.py holds it against include/tpspp.h.  Only calls the API documents as valid are made.
"""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import guarded_alloc as GA
from tps_pp_amd import _lib, constants, ops, synth

gpu = pytest.mark.gpu
SWEPT = {}                  # entry point -> names of the sweep cases that reach it

# Regions of outputs that are, by contract, only partly written: (entry point, region, the sentence of include/tpspp.h).
# At most one entry per entry point, never a whole entry point.
PARTLY_WRITTEN = []


REACHED = {}                # sweep case -> entry points its guarded runs really called (recorded by `_Spy`)
_NOW = []                   # names reached by the case that is running


def sweeps(*names, sometimes=()):
    """Declares the entry points a case reaches.  The declaration is checked, not trusted: `run_twice` records every
    library function the guarded run calls; each case must reach every name in `names`, and over a whole run of the file
    every name in `sometimes` (reached at some shapes only) as well (test_zz_sweep_totals)."""
    def deco(fn):
        for n in names + tuple(sometimes):
            SWEPT.setdefault(n, []).append(fn.__name__)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            del _NOW[:]
            fn(*a, **kw)
            got = REACHED.setdefault(fn.__name__, set())
            got.update(_NOW)
            missing = set(names) - set(_NOW)
            assert not missing, f"{fn.__name__} declares {sorted(missing)} but its guarded run never called them"
        wrapper._sometimes = tuple(sometimes)
        return wrapper
    return deco


class _Spy:
    """Stands in for the loaded library while a guarded run is on: records the name of every function that is fetched."""

    def __init__(self, real):
        self.__dict__["_real"] = real

    def __getattr__(self, name):
        if name.startswith("tpspp_"):
            _NOW.append(name)
        return getattr(self._real, name)


def params_of(test_fn, index=0):
    """The argument list of a test's `@pytest.mark.parametrize` (so that shapes are imported, not retyped)."""
    marks = [m for m in getattr(test_fn, "pytestmark", []) if m.name == "parametrize"]
    return list(marks[index].args[1])


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def run_twice(cuda, fn, bitwise=True):
    """`fn(put)` builds its device inputs with `put` and returns a nest of tensors.  A returned float tensor that does not
    live in a guarded allocation must say so (`GA.Unguarded(tensor, why)`)."""
    plain = fn(lambda x: x.to(cuda))
    torch.cuda.synchronize()
    real = _lib.lib()
    with GA.guarded(cuda) as g:
        _lib._lib = _Spy(real)
        try:
            got = fn(g.input)
        finally:
            _lib._lib = real
        n = g.check(got, require_guarded=True)
    assert n > 0, "no allocation went through the guard"
    assert not g.fallthrough, f"allocations on the device that the guard did not serve: {g.fallthrough}"
    assert list(GA.tensors_in(got)), "the case returned nothing to check"
    if bitwise:
        ok, why = GA.same_bits(got, plain)
        assert ok, "guarded and plain runs differ: " + why
    return got


def rehome(obj, put):
    """A weight holder's tensors moved through `put` (prepared on the CPU, or re-homed from the device)."""
    for k, v in list(vars(obj).items()):
        if isinstance(v, torch.Tensor):
            setattr(obj, k, put(v.cpu()))
    return obj


def put_module(mod, put):
    """A fresh copy of `mod` whose parameters and buffers went through `put`."""
    mod = copy.deepcopy(mod)
    for p in list(mod.parameters()) + list(mod.buffers()):
        p.data = put(p.data.cpu())
    return mod


class tuning:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        _lib.lib().tpspp_conv_set_tuning(self.v)

    def __exit__(self, *a):
        _lib.lib().tpspp_conv_set_tuning(0)


# ---- self-test of the harness on the device ---------------------------------------------------------------------------

@gpu
def test_harness_catches_an_overrun_and_an_unwritten_element_on_the_device(cuda):
    """Both negative checks with torch indexing on the harness's own buffer (legal memory: no kernel writes out of bounds)."""
    with GA.guarded(cuda) as g:
        a = torch.empty((3, 5), device=cuda)
        b = torch.empty(7, device=cuda, dtype=torch.bfloat16)
        assert a.data_ptr() % GA.ALIGN == 0 and b.data_ptr() % GA.ALIGN == 0
        assert torch.isnan(a).all() and torch.isnan(b.float()).all()
        a.fill_(1.0)
        b.fill_(2.0)
        assert g.check((a, b)) == 2
        b[3] = float("nan")                                 # an ordinary NaN is not the poison word
        g.check(b)
        b.view(torch.int16)[3] = -1
        with pytest.raises(GA.GuardError, match="never written"):
            g.check({"x": [a, b]})
        b.fill_(2.0)
        torch.as_strided(a, (1,), (1,), a.storage_offset() + a.numel()).fill_(3.0)     # one float past the payload
        with pytest.raises(GA.GuardError, match="0 bytes past its end"):
            g.check(a)
    assert torch.empty is GA._REAL_EMPTY and torch.empty_like is GA._REAL_EMPTY_LIKE


# ---- 1. fp32 convolution forward --------------------------------------------------------------------------------------

import test_gpu_conv as TC            # noqa: E402


@gpu
@sweeps("tpspp_conv2d_fwd")
@pytest.mark.parametrize("case", TC.CASES, ids=[c[0] for c in TC.CASES])
def test_fp32_conv_forward(cuda, case):
    name, srcs, cout, k, stride, relu, res_mode, N = case
    xs = [t(synth.dyadic((N, c, h, w), f"{name}.x{i}", 1)) for i, (c, h, w, _, _) in enumerate(srcs)]
    cin = sum(s_[0] for s_ in srcs)
    w = t(synth.dyadic((cout, cin, k, k), name + ".w", 1, 1.0 / np.sqrt(cin * k * k)))
    b = None if "no bias" in name else t(synth.dyadic((cout,), name + ".b", 1, 0.1))
    Ho, Wo = [(d * u + 2 * ((k - 1) // 2) - k) // s + 1 for d, u, s in
              ((srcs[0][1], srcs[0][3], stride[0]), (srcs[0][2], srcs[0][4], stride[1]))]
    res = t(synth.dyadic((N, cout, Ho, Wo), name + ".r", 1)) if res_mode else None

    def fn(put):
        cw = rehome(ops.prep_conv_weight(w, conv_bias=b, src_channels=[s_[0] for s_ in srcs]), put)
        ent = [(put(x), s_[3], s_[4]) for x, s_ in zip(xs, srcs)]
        r = None if res is None else put(res)
        outs = []
        for force_generic in (0, 1):
            with tuning(force_generic):
                outs.append(ops.conv2d(ent, cw, stride, relu, r, res_mode))
        return outs
    run_twice(cuda, fn)


@gpu
@sweeps("tpspp_front_fwd", "tpspp_down_fused_f32_fwd", "tpspp_maxpool2x2_fwd", "tpspp_global_avgpool_fwd")
@pytest.mark.parametrize("N,H", [(1, 32), (3, 32), (5, 8), (3, 2)])
def test_fp32_fused_front_and_pools(cuda, N, H):
    from tps_pp_amd import TPS_PP
    torch.manual_seed(13)
    m = TPS_PP().eval()
    with torch.no_grad():
        for c in (m.down0, m.down1, m.down0_1, m.down1_1):
            c.conv.bias.uniform_(-0.5, 0.5)
    g = torch.Generator().manual_seed(N * 100 + H)
    o0, o1 = torch.randn((N, 32, H, 128), generator=g), torch.randn((N, 32, H, 128), generator=g)
    x = torch.randn((N, 64, H // 2, 64), generator=g)

    def fn(put):
        mm = put_module(m, put)
        fw = ops.FrontWeights(mm)
        cw0 = rehome(ops.prep_conv_weight(m.down0_1.conv.weight, conv_bias=m.down0_1.conv.bias), put)
        d0, d1, dx = put(o0), put(o1), put(x)
        f = ops.front(d0, d1, dx, fw)
        f_no = ops.front(d0, d1, dx, fw, store01=False)
        return (f, f_no[2:], ops.down_fused_f32(d0, fw.w0, fw.b0, cw0), ops.maxpool2x2(d0), ops.global_avgpool(dx))
    run_twice(cuda, fn)


import test_gpu_conv_bwd as TB        # noqa: E402

BWD_CASES = TB.RAGGED + TB.BACKBONE_CASES


@gpu
@sweeps("tpspp_conv2d_prep_weight", "tpspp_conv2d_fwd", "tpspp_conv2d_bwd_data", "tpspp_conv2d_bwd_weight")
@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_conv_backward(cuda, case):
    """The device-side weight preparation, the forward on it, and both backward kernels; the split-K workspace of
    tpspp_conv2d_bwd_weight is allocated by the wrapper at exactly tpspp_conv2d_bwd_weight_workspace_floats."""
    name, spec, cout, k, stride, relu, bias, N = case
    srcs, w, b, g = TB.make(spec, cout, k, bias, N, 1)
    st = (stride, stride) if isinstance(stride, int) else stride
    Ho, Wo = [(d * u + 2 * ((k - 1) // 2) - k) // s + 1 for d, u, s in
              ((spec[0][1], spec[0][3], st[0]), (spec[0][2], spec[0][4], st[1]))]
    dy = torch.randn((N, cout, Ho, Wo), generator=g)

    def fn(put):
        ds = [put(s) for s in srcs]
        ent = [(d, uh, uw) for d, (_, _, _, uh, uw) in zip(ds, spec)]
        wd = put(w)
        cw = ops.prep_conv_weight_device(wd, None if b is None else put(b), [s[0] for s in spec])
        y = ops.conv2d(ent, cw, stride, relu=bool(relu))
        dyd = put(dy)
        dx = ops.conv2d_bwd_data(dyd, wd, ent, stride, y=y, relu=bool(relu))
        dw, db = ops.conv2d_bwd_weight(ent, dyd, k, stride, y=y, relu=bool(relu), want_bias=bias)
        return (cw.wt, cw.tiled, y, dx, dw, db)
    run_twice(cuda, fn)


# ---- 2. bf16 and bf16x3 convolution -----------------------------------------------------------------------------------

import test_gpu_conv_bf16 as T16      # noqa: E402

DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def _bf16_inputs(name, srcs, cout, k, stride, res_mode, N):
    xs = [t(synth.dyadic((N, s_[0], s_[1], s_[2]), f"{name}.x{i}", 1)) for i, s_ in enumerate(srcs)]
    cin = sum(s_[0] for s_ in srcs)
    w = t(synth.dyadic((cout, cin, k, k), name + ".w", 1, 1.0 / np.sqrt(cin * k * k)))
    b = t(synth.dyadic((cout,), name + ".b", 1, 0.1))
    Ho, Wo = [(d * u + 2 * ((k - 1) // 2) - k) // s + 1 for d, u, s in
              ((srcs[0][1], srcs[0][3], stride[0]), (srcs[0][2], srcs[0][4], stride[1]))]
    res = t(synth.dyadic((N, cout, Ho, Wo), name + ".r", 1)) if res_mode else None
    return xs, w, b, res


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("case", T16.CASES, ids=[c[0] for c in T16.CASES])
def test_bf16_conv_tiled(cuda, case):
    """NCHW sources of either type, bf16 and fp32 outputs, plain and three-term-split weights."""
    name, srcs, cout, k, stride, relu, res_mode, res_dt, N = case
    xs, w, b, res = _bf16_inputs(name, srcs, cout, k, stride, res_mode, N)

    def fn(put):
        ent = [(put(x.to(DT[s_[5]])), s_[3], s_[4]) for x, s_ in zip(xs, srcs)]
        r = None if res is None else put(res.to(DT[res_dt]))
        cw = rehome(ops.prep_conv_weight_bf16(w, conv_bias=b), put)
        cw3 = rehome(ops.prep_conv_weight_bf16(w, conv_bias=b, x3=True), put)
        return (ops.conv2d_bf16(ent, cw, stride, relu, r, res_mode, out_dtype=torch.bfloat16),
                ops.conv2d_bf16(ent, cw, stride, relu, r, res_mode, out_dtype=torch.float32),
                ops.conv2d_bf16(ent, cw3, stride, relu, r, res_mode, out_dtype=torch.float32))
    run_twice(cuda, fn)


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("case", T16.BLK_CASES, ids=[c[0] for c in T16.BLK_CASES])
def test_bf16_conv_blocked_layouts(cuda, case):
    """Blocked sources, residual and output: bf16 (layout code 2) and fp32 with the three-term split (code 3)."""
    name, srcs, cout, k, stride, relu, res_mode, res_dt, N = case
    xs, w, b, res = _bf16_inputs(name, srcs, cout, k, stride, res_mode, N)

    def fn(put):
        out = []
        for B, x3, odt in ((ops.Blocked, False, torch.bfloat16), (ops.Blocked32, True, torch.float32)):
            ent = [(B(put(B.from_nchw(x).t)), s_[3], s_[4]) for x, s_ in zip(xs, srcs)]
            r = None if res is None else B(put(B.from_nchw(res).t))
            cw = rehome(ops.prep_conv_weight_bf16(w, conv_bias=b, x3=x3), put)
            out.append(ops.conv2d_bf16(ent, cw, stride, relu=relu, residual=r, res_mode=res_mode, out_dtype=odt,
                                       out_blocked=True).t)
        return out
    run_twice(cuda, fn)


def _blocked_case(cuda, srcs, cout, k, stride, res_mode, relu, f32_out, N, seed, off_bits):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((N, c, h, w), generator=g) for c, h, w, _, _ in srcs]
    cin = sum(s_[0] for s_ in srcs)
    w = torch.randn((cout, cin, k, k), generator=g) / np.sqrt(cin * k * k)
    b = torch.randn((cout,), generator=g) * 0.1
    Ho, Wo = srcs[0][1] * srcs[0][3] // stride[0], srcs[0][2] * srcs[0][4] // stride[1]
    res = torch.randn((N, cout, Ho, Wo), generator=g) if res_mode else None

    def fn(put):
        ent = [(ops.Blocked(put(ops.Blocked.from_nchw(x).t)), uh, uw) for x, (_, _, _, uh, uw) in zip(xs, srcs)]
        r = ops.Blocked(put(ops.Blocked.from_nchw(res).t)) if res_mode else None
        cw = rehome(ops.prep_conv_weight_bf16(w, conv_bias=b), put)
        kw = dict(relu=relu, residual=r, res_mode=res_mode)
        kw.update({"out_dtype": torch.float32} if f32_out else {"out_blocked": True})
        outs = []
        for bits in (0, off_bits):                     # the special kernel, then the tiled kernel on the same tensors
            with tuning(bits):
                o = ops.conv2d_bf16(ent, cw, stride, **kw)
                outs.append(o if f32_out else o.t)
        return outs
    run_twice(cuda, fn)


PERSIST = T16.PERSIST_CASES
PERSIST32 = params_of(T16.test_conv_bf16_persistent_kernel_with_32_output_channels)


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("case", PERSIST, ids=[c[0] for c in PERSIST])
def test_bf16_conv_persistent(cuda, case):
    name, srcs, stride, res_mode, f32_out, N = case
    _blocked_case(cuda, srcs, 64, 3, stride, res_mode, True, f32_out, N, len(name), 2)


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("case", PERSIST32, ids=[c[0] for c in PERSIST32])
def test_bf16_conv_persistent_32_channels(cuda, case):
    name, H, W, stride, res_mode, f32_out, N = case
    _blocked_case(cuda, [(32, H, W, 1, 1)], 32, 3, stride, res_mode, True, f32_out, N, len(name), 2)


WIDE = T16.WIDE_CASES


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("case", WIDE, ids=[c[0] for c in WIDE])
def test_bf16_conv_wide_3x3(cuda, case):
    name, C, H, W, res_mode, relu, N = case
    _blocked_case(cuda, [(C, H, W, 1, 1)], C, 3, (1, 1), res_mode, relu, "fp32 NCHW" in name, N, len(name) + C, 4)


C1X1_WIDE = params_of(T16.test_conv1x1_wide_kernel_is_the_tiled_kernel_bit_for_bit)


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("case", C1X1_WIDE, ids=[c[0] for c in C1X1_WIDE])
def test_bf16_conv_wide_1x1(cuda, case):
    name, cin, cout, H, W, relu, f32_out, N = case
    _blocked_case(cuda, [(cin, H, W, 1, 1)], cout, 1, (1, 1), 0, relu, f32_out, N, cin + cout + N, 6)


C1X1 = T16.C1X1_CASES


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("case", C1X1, ids=[c[0] for c in C1X1])
def test_bf16_conv_blocked_1x1(cuda, case):
    name, cin, cout, H, W, relu, N = case
    _blocked_case(cuda, [(cin, H, W, 1, 1)], cout, 1, (1, 1), 0, relu, False, N, cin + cout + N, 6)


STEM = params_of(T16.test_stem_kernel_is_the_tiled_kernel_bit_for_bit)


@gpu
@sweeps("tpspp_conv2d_bf16_fwd")
@pytest.mark.parametrize("C,H,N,relu", STEM)
def test_bf16_conv_stem(cuda, C, H, N, relu):
    g = torch.Generator().manual_seed(C * 100 + H + N)
    x = torch.randn((N, C, H, 128), generator=g)
    w = torch.randn((32, C, 3, 3), generator=g) / np.sqrt(C * 9.0)
    b = torch.randn((32,), generator=g) * 0.1

    def fn(put):
        cw = rehome(ops.prep_conv_weight_bf16(w, conv_bias=b), put)
        xd = put(x)
        outs = []
        for bits in (0, 4):
            with tuning(bits):
                outs += [ops.conv2d_bf16([xd], cw, 1, relu=relu), ops.conv2d_bf16([xd], cw, 1, relu=relu, out_blocked=True).t]
        return outs
    run_twice(cuda, fn)


@gpu
@sweeps("tpspp_front_bf16_fwd", "tpspp_down_fused_bf16_fwd", "tpspp_down_fused_x3_fwd", "tpspp_blocked_to_nchw_bf16")
@pytest.mark.parametrize("N,H", [(1, 32), (3, 32), (5, 8), (3, 2)])
def test_bf16_fused_front(cuda, N, H):
    from tps_pp_amd import TPS_PP
    torch.manual_seed(11)
    m = TPS_PP().eval()
    with torch.no_grad():
        for c in (m.down0, m.down1, m.down0_1, m.down1_1):
            c.conv.bias.uniform_(-0.5, 0.5)
    g = torch.Generator().manual_seed(N * 100 + H)
    o0, o1 = torch.randn((N, 32, H, 128), generator=g), torch.randn((N, 32, H, 128), generator=g)
    x = torch.randn((N, 64, H // 2, 64), generator=g)

    def fn(put):
        mm = put_module(m, put)
        outs = []
        for x3, dt in ((False, torch.bfloat16), (True, torch.float32)):
            fw = ops.FrontWeightsBf16(mm, x3)
            cw0 = rehome(ops.prep_conv_weight_bf16(m.down0_1.conv.weight, conv_bias=m.down0_1.conv.bias, x3=x3), put)
            d0, d1, dx = put(o0.to(dt)), put(o1.to(dt)), put(x.to(dt))
            for fg_dt in (torch.bfloat16, torch.float32):
                if x3 and fg_dt == torch.bfloat16:
                    continue
                for blocked in (False, True):
                    f = ops.front_bf16(d0, d1, dx, fw, fg_dt, blocked=blocked)
                    outs += [v.t if isinstance(v, ops.Blocked) else v for v in f]
            f = ops.front_bf16(d0, d1, dx, fw, torch.float32, blocked=True, store01=False)
            outs += [v.t if isinstance(v, ops.Blocked) else v for v in f if v is not None]
            outs.append(ops.down_fused_bf16(d0, fw.w0, fw.b0, cw0).t)
        if (H * 128) % 64 == 0:
            outs.append(ops.Blocked(put(ops.Blocked.from_nchw(o0).t)).nchw_hip())
        return outs
    run_twice(cuda, fn)


import test_gpu_head as TH            # noqa: E402

TOKGEMM = TH.TOKGEMM_CASES


@gpu
@sweeps("tpspp_token_gemm_bf16_fwd")
@pytest.mark.parametrize("case", TOKGEMM, ids=[c[0] for c in TOKGEMM])
def test_token_gemm(cuda, case):
    name, K, Co, M, act, res, odt, x3 = case
    g = torch.Generator().manual_seed(K * 7 + Co + M)
    w = torch.randn((Co, K, 1, 1), generator=g) * 0.05
    b = torch.randn(Co, generator=g) * 0.1
    x = torch.randn((K, M), generator=g)
    r = torch.randn((Co, M), generator=g) if res else None

    def fn(put):
        cw = rehome(ops.prep_conv_weight_bf16(w, conv_bias=b, x3=x3), put)
        return ops.token_gemm_bf16(put(x), cw, act=act, residual=None if r is None else put(r), out_dtype=odt)
    run_twice(cuda, fn)


# ---- 4. BatchNorm training ---------------------------------------------------------------------------------------------

import test_gpu_backbone_train as TBN  # noqa: E402


def _bn_case(cuda, N, C, H, W, mode, train=(True, True), relu=True, view=False):
    za, zb, gy = TBN.bn_inputs(N, C, H, W, C + N + H)
    bns = TBN.make_bns(C, C + N + H, 0.1, train)

    def fn(put):
        b = [put_module(x, put) for x in bns]
        for x, tr in zip(b, train):
            x.train(tr)
        if view:                                          # a view that does not start on a 16-byte boundary
            big = torch.cat([torch.zeros(1), za.flatten()])
            dza = put(big)[1:].view_as(za)
        else:
            dza = put(za)
        dzb, dgy = put(zb), put(gy)

        def stats(m, z):
            if m.training:
                return ops.bn_train_stats(z, m.eps, m.momentum, m.running_mean, m.running_var, m.num_batches_tracked)
            return ops.bn_eval_stats(m.running_mean, m.running_var, m.eps)
        a = b[0]
        sa, sb, kw = stats(a, dza), None, {}
        if mode == "residual":
            kw = dict(residual=dzb)
        elif mode == "branch":
            sb = stats(b[1], dzb)
            kw = dict(zb=dzb, stats_b=sb, gamma_b=b[1].weight, beta_b=b[1].bias)
        y = ops.bn_apply(dza, sa, a.weight, a.bias, relu=relu, **kw)
        two = mode == "branch"
        sums = ops.bn_bwd_reduce(dgy, y, dza, sa, dzb if two else None, sb if two else None, relu=relu)
        dres = torch.empty_like(dgy) if mode == "residual" else None
        dz = ops.bn_bwd_data(dgy, y, dza, sa, a.weight, sums, a.training, zb=dzb if two else None,
                             stats_b=sb if two else None, gamma_b=b[1].weight if two else None,
                             train_b=b[1].training if two else True, relu=relu, dres=dres,
                             dres_mode=1 if mode == "residual" else 0)
        return (sa, sb, y, sums, dres, dz, [(m.running_mean, m.running_var, m.num_batches_tracked) for m in b])
    run_twice(cuda, fn)


@gpu
@sweeps("tpspp_bn_train_stats", "tpspp_bn_apply_fwd", "tpspp_bn_bwd_reduce", "tpspp_bn_bwd_data")
@pytest.mark.parametrize("C", [32, 512])
@pytest.mark.parametrize("N,H,W", [(1, 5, 7), (3, 37, 41), (3, 40, 40)])
@pytest.mark.parametrize("mode", ["none", "residual", "branch"])
def test_bn_training_kernels(cuda, C, N, H, W, mode):
    """Workspaces allocated by the wrappers at exactly tpspp_bn_stats_workspace_floats / tpspp_bn_bwd_reduce_workspace_floats."""
    _bn_case(cuda, N, C, H, W, mode)


@gpu
@sweeps("tpspp_bn_eval_stats", "tpspp_bn_apply_fwd", "tpspp_bn_bwd_reduce", "tpspp_bn_bwd_data")
@pytest.mark.parametrize("mode", ["none", "residual", "branch"])
def test_bn_eval_mode_and_unaligned_view(cuda, mode):
    _bn_case(cuda, 3, 64, 9, 20, mode, train=(False, False))
    _bn_case(cuda, 2, 32, 8, 16, mode, train=(False, True), relu=mode != "branch", view=True)


# ---- 5. regressor training ----------------------------------------------------------------------------------------------

import test_gpu_regressor_train as TR  # noqa: E402


@gpu
@sweeps(sometimes=(                                      # each block reaches its own kernels
        "tpspp_mm_f32", "tpspp_linear_bwd_weight", "tpspp_act_bwd", "tpspp_plane_ln_fwd", "tpspp_plane_ln_bwd", "tpspp_dgab_pool_fwd",
        "tpspp_dgab_pool_bwd", "tpspp_dgab_gate_fwd", "tpspp_dgab_gate_bwd", "tpspp_cbam_train_fwd", "tpspp_cbam_bwd"))
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("kind", ["dgab", "score", "cbam", "points"])
def test_regressor_training_blocks(cuda, kind, N):
    """Forward and backward of one block through ops.*_autograd: every saved tensor, gradient and workspace
    (tpspp_linear_bwd_weight / tpspp_plane_ln_bwd / tpspp_cbam_bwd workspaces at exactly their queried sizes) is guarded."""
    mod = TR.block_module(kind)
    inputs = TR.block_inputs(kind, N, seed=N)
    if kind == "dgab":
        inputs[0][0, 7] = 0.25                            # a constant plane: variance 0
    def fn(put):
        m = put_module(mod, put)
        for p in m.parameters():
            p.grad = None
        xs = [put(x).requires_grad_(True) for x in inputs]
        call = {"dgab": lambda: ops.dgab_autograd(xs[0], xs[1], m), "score": lambda: ops.score_autograd(xs[0], xs[1], m),
                "cbam": lambda: ops.cbam_autograd(xs[0], m), "points": lambda: ops.tpe_points_autograd(xs[0], m)}[kind]
        out = call()
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(100 + N))
        out.backward(put(gout))
        return (out.detach(), [x.grad for x in xs], {k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    run_twice(cuda, fn)


# ---- 6. regressor inference ---------------------------------------------------------------------------------------------

def _tpspp_module():
    import cases
    from tps_pp_amd import TPS_PP
    m = TPS_PP().eval()
    sd = cases.synth_state(m.state_dict(), 4, cases.tpspp_state_rule, cases.TPSPP_KEEP)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


@gpu
@sweeps("tpspp_dgab_fwd", "tpspp_dgab_bf16_fwd", "tpspp_score_fwd", "tpspp_score_x3_fwd", "tpspp_cbam_fwd",
        "tpspp_tpe_points_fwd")
@pytest.mark.parametrize("N", [1, 3, 5])
def test_regressor_inference(cuda, N):
    m = _tpspp_module()
    x = t(synth.dyadic((N, 64, 16, 64), "dgab.x"))
    en = t(synth.dyadic((N, 64, 2, 16), "dgab.en"))
    e3 = en.abs()
    de2 = x[:, :, :5, :50].contiguous()                   # ragged pixel count: a partial last workgroup
    with torch.no_grad():
        p1 = m.TPE.p_linear(en.flatten(2).transpose(1, 2)).contiguous()

    def fn(put):
        mm = put_module(m, put)
        blk = mm.TPE.atten[0]
        dx, dy, dp = put(x), put(en.view(N, 64, 32)), put(p1)
        sw = ops.ScoreWeights(mm.TPE.feat_linear)
        with torch.no_grad():
            return (ops.dgab(dx, dy, ops.DgabWeights(blk)), ops.dgab_bf16(dx, dy, ops.DgabWeightsBf16(blk)),
                    ops.dgab_bf16(dx, dy, ops.DgabWeightsBf16(blk, x3=True)),
                    ops.score(dx, dp, sw, mm.TPE.scale), ops.score(dx, dp, sw, mm.TPE.scale, x3=True),
                    ops.score(put(de2), dp, sw, mm.TPE.scale), ops.score(put(de2), dp, sw, mm.TPE.scale, x3=True),
                    ops.cbam(put(e3), mm.MSFA.conv.atten), ops.tpe_points(put(e3), mm.TPE))
    run_twice(cuda, fn)


# ---- 7. warp ------------------------------------------------------------------------------------------------------------

import test_gpu_backward as TWB       # noqa: E402
import test_gpu_warp as TW            # noqa: E402

CLASSIC = params_of(TW.test_classic_warp_vs_oracle)


def _classic_inputs(N, C, H, W, Ho, Wo, F, perturb, tag):
    Kc = constants.classic(F, (Ho, Wo))
    ctrl = constants.classic_identity_ctrl(F)[None] + perturb * synth.dyadic((N, F, 2), tag + ".ctrl", N)
    img = synth.dyadic((N, C, H, W), tag + ".img", N + 1)
    return Kc, t(ctrl.astype(np.float32)), t(img)


@gpu
@sweeps("tpspp_warp_fwd", "tpspp_transpose_p_hat", "tpspp_solve_T", "tpspp_build_grid", "tpspp_grid_sample",
        sometimes=("tpspp_prepare_mirror_table",))        # only geometries with a prepared form reach it
@pytest.mark.parametrize("N,C,H,W,Ho,Wo,F,perturb", CLASSIC)
def test_classic_warp(cuda, N, C, H, W, Ho, Wo, F, perturb):
    """Generic, coalesced, mirror-symmetric and prepared-table paths (the image-pair kernel where the geometry has one: odd
    batches end in a group with a single image), with and without the optional outputs; and the unfused pieces."""
    Kc, ctrl, img = _classic_inputs(N, C, H, W, Ho, Wo, F, perturb, "ms")
    sym = ops.table_mirror_symmetry(Kc["P_hat"], (Ho, Wo), F)

    def fn(put):
        P_hat, inv = put(t(Kc["P_hat"])), put(t(Kc["inv_delta_C"]))
        dimg, dctrl = put(img), put(ctrl)
        prep, packed = ops.prepare_mirror_table(P_hat, (Ho, Wo))
        pt = ops.transpose_p_hat(P_hat)
        outs = [pt, prep]
        for P_hat_t, flags in ((None, 0), (pt, 0), (pt, ops.TABLE_MIRROR4 * sym), (prep, ops.TABLE_MIRROR4 * sym | packed)):
            outs.append(ops.warp(dimg, dctrl, inv, P_hat, (Ho, Wo), want_grid=True, want_idx=True, P_hat_t=P_hat_t,
                                 table_flags=flags))
            outs.append(ops.warp(dimg, dctrl, inv, P_hat, (Ho, Wo), P_hat_t=P_hat_t, table_flags=flags)[0])
        T = ops.solve_T(inv, dctrl)
        grid = ops.build_grid(P_hat, T)
        outs += [T, grid, ops.grid_sample(dimg, grid.view(N, Ho, Wo, 2), return_idx=True)]
        return outs
    run_twice(cuda, fn)


FORCED = ([(6,) + c for c in params_of(TW.test_inplace_kernel_vs_oracle)] +
          [(7,) + c + (0.4,) for c in params_of(TW.test_runtime_geometry_kernel_forced)] +
          [(8,) + c + (0.45,) for c in TW.SPAN_CASES])


@gpu
@sweeps("tpspp_warp_fwd")
@pytest.mark.parametrize("choice,N,C,H,W,perturb", FORCED)
def test_forced_warp_kernel_families(cuda, choice, N, C, H, W, perturb):
    """kernel_choice 6 (results staged in place), 7 (run-time geometry forced), 8 (span staging forced; a violent warp: some
    bands stage, others take their taps from global memory)."""
    Kc, ctrl, img = _classic_inputs(N, C, H, W, H, W, 20, perturb, f"msf{choice}")

    def fn(put):
        P_hat, inv = put(t(Kc["P_hat"])), put(t(Kc["inv_delta_C"]))
        prep, packed = ops.prepare_mirror_table(P_hat, (H, W))
        dimg, dctrl = put(img), put(ctrl)
        try:
            ops.set_warp_tuning(kernel_choice=choice)
            a = ops.warp(dimg, dctrl, inv, P_hat, (H, W), want_grid=True, want_idx=True, P_hat_t=prep,
                         table_flags=ops.TABLE_MIRROR4 | packed)
            b = ops.warp(dimg, dctrl, inv, P_hat, (H, W), P_hat_t=prep, table_flags=ops.TABLE_MIRROR4 | packed)[0]
        finally:
            ops.set_warp_tuning()
        return (a, b)
    run_twice(cuda, fn)


TPSPP_WARP = params_of(TW.test_tpspp_warp_vs_oracle)


def _tpspp_inputs(N, point, hw, C0, C1, tag):
    K = constants.tpspp(hw, point)
    F = point[0] * point[1]
    c = t((constants.tpspp_initial_ctrl(point)[None] + 0.02 * synth.dyadic((N, F, 2), tag + ".c", N)).astype(np.float32))
    score = t(synth.dyadic((N, hw[0] * hw[1], F), tag + ".score", N))
    in0 = t(synth.smooth_image((N, C0, 2 * hw[0], 2 * hw[1]), tag + ".fg"))
    in1 = t(synth.dyadic((N, C1, hw[0], hw[1]), tag + ".x", N)) if C1 else None
    return K, c, score, in0, in1


@gpu
@sweeps("tpspp_warp_fwd", "tpspp_warp_bwd", "tpspp_build_grid", "tpspp_solve_T")
@pytest.mark.parametrize("N,point,hw,C0,C1,with_score", TPSPP_WARP)
def test_tpspp_warp_and_its_backward(cuda, N, point, hw, C0, C1, with_score):
    """The TPS_PP geometry, fp32 and bf16 planes; its backward (workspace exactly tpspp_warp_bwd_workspace_floats) with the
    fixed-point accumulator bit for bit, and with the default accumulator for guards and poison only."""
    K, c, score, in0, in1 = _tpspp_inputs(N, tuple(point), tuple(hw), C0, C1, "mst")
    if not with_score:
        score = None
    g0 = t(synth.dyadic((N, C0) + tuple(hw), "mst.g0", N))
    g1 = t(synth.dyadic((N, C1) + tuple(hw), "mst.g1", N)) if C1 else None

    def common(put):
        d = dict(hat=put(t(K["hat_C"])), P=put(t(K["P_hat"])), xy=put(t(K["P_xy"])), c=put(c),
                 s=None if score is None else put(score), i0=put(in0), i1=None if in1 is None else put(in1),
                 g0=put(g0), g1=None if g1 is None else put(g1))
        d["fwd"] = ops.warp(d["i0"], d["c"], d["hat"], d["P"], hw, P_xy=d["xy"], score=d["s"], in1=d["i1"], want_grid=True)
        return d

    def bwd(d, fixed):
        return ops.warp_backward(d["g0"], d["i0"], d["fwd"][2], d["c"], d["hat"], d["P"], hw, P_xy=d["xy"], score=d["s"],
                                 in1=d["i1"], g_out1=d["g1"], fixed_point=fixed)

    def fn(put):
        d = common(put)
        b16 = (None, None)
        if point[0] * point[1] == 32:                     # TPSPP_IO_BF16 needs a shape the plane-streaming kernel takes
            b16 = ops.warp(put(in0.bfloat16()), d["c"], d["hat"], d["P"], hw, P_xy=d["xy"], score=d["s"],
                           in1=None if in1 is None else put(in1.bfloat16()))
        T = ops.solve_T(d["hat"], d["c"])
        return (d["fwd"], b16[:2], ops.build_grid(d["P"], T, d["xy"], d["s"]), bwd(d, True))
    run_twice(cuda, fn)
    run_twice(cuda, lambda put: bwd(common(put), False), bitwise=False)


CLASSIC_BWD = params_of(TWB.test_classic_backward_single_launch_against_the_two_kernel_route)


@gpu
@sweeps("tpspp_warp_bwd")
@pytest.mark.parametrize("C,hw,n", CLASSIC_BWD)
def test_classic_warp_backward_both_routes(cuda, C, hw, n):
    Kc, ctrl, img = _classic_inputs(n, C, hw[0], hw[1], hw[0], hw[1], 20, 0.3, "msb")
    g0 = t(synth.dyadic((n, C) + tuple(hw), "msb.g0", n))

    def run(put, fixed):
        P_hat, inv = put(t(Kc["P_hat"])), put(t(Kc["inv_delta_C"]))
        dimg, dctrl = put(img), put(ctrl)
        grid = ops.warp(dimg, dctrl, inv, P_hat, hw, want_grid=True)[2]
        return [ops.warp_backward(put(g0), dimg, grid, dctrl, inv, P_hat, hw, fixed_point=fixed, two_kernels=two)
                for two in (False, True)]
    run_twice(cuda, lambda put: run(put, True))
    run_twice(cuda, lambda put: run(put, False), bitwise=False)


@gpu
@sweeps("tpspp_warp_plan_run")
def test_prepared_warp_plan(cuda):
    Kc, ctrl, img = _classic_inputs(5, 3, 32, 100, 32, 100, 20, 0.3, "msp")

    def fn(put):
        P_hat, inv = put(t(Kc["P_hat"])), put(t(Kc["inv_delta_C"]))
        prep, packed = ops.prepare_mirror_table(P_hat, (32, 100))
        out0 = torch.empty((5, 3, 32, 100), device=cuda)
        plan = ops.WarpPlan(put(img), put(ctrl), inv, P_hat, (32, 100), out0, P_hat_t=prep,
                            table_flags=ops.TABLE_MIRROR4 | packed)
        plan.run()
        torch.cuda.synchronize()
        del plan
        return out0
    run_twice(cuda, fn)


# ---- 8. recogniser head ---------------------------------------------------------------------------------------------------

@gpu
@sweeps("tpspp_transpose2d", "tpspp_layernorm_cm_fwd", "tpspp_linear_ln_fwd", "tpspp_attn_enc_fwd")
@pytest.mark.parametrize("T", [7, 20, 64, 100])
def test_head_pieces(cuda, T):
    g = torch.Generator().manual_seed(T)
    N, C = 3, 128
    M = N * T
    x = torch.randn(C, M, generator=g)
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    Co = 40 if T == 7 else 384
    w, b = torch.randn(Co, C, generator=g) / C ** 0.5, torch.randn(Co, generator=g)
    r = torch.randn(Co, M, generator=g)
    qkv = torch.randn(3 * C, M, generator=g)
    vl = torch.tensor([T, max(1, T // 2), max(1, T // 3)], dtype=torch.int32)

    def fn(put):
        dx = put(x)
        f1 = ops.fold_layernorm(put(ga), put(be), ops.kmajor(put(w)), put(b))
        f2 = ops.fold_layernorm(put(ga), put(be), ops.kmajor(put(w)))
        dq = put(qkv)
        return (ops.transpose2d(dx), ops.layernorm_cm(dx, put(ga), put(be), 1e-5),
                ops.linear_ln(dx, f1, 1e-5, act=2, residual=put(r)), ops.linear_ln(dx, f2, 1e-5, token_major=True),
                ops.attn_enc(dq, N, T, put(vl)), ops.attn_enc(dq, N, T, None))
    run_twice(cuda, fn)


def _head_modules(full):
    import cases
    from tps_pp_amd import NRTRDecoder, NRTREncoder
    if full:
        enc = TH.load_synth(NRTREncoder().eval(), 9)
        dec = TH.load_synth(NRTRDecoder(num_classes=cases.NUM_CLASSES, start_idx=cases.START_IDX,
                                        padding_idx=cases.PAD_IDX, max_seq_len=6).eval(), 10)
        return enc, dec, 512
    cfg = dict(cases.HD_SMALL)
    enc = TH.load_synth(NRTREncoder(**cfg).eval(), 9)
    dec = TH.load_synth(NRTRDecoder(d_embedding=cfg["d_model"], num_classes=cases.NUM_CLASSES, start_idx=cases.START_IDX,
                                    padding_idx=cases.PAD_IDX, max_seq_len=cases.HD_MAXLEN, **cfg).eval(), 10)
    return enc, dec, cfg["d_model"]


HEAD_SHAPES = [(False, (1, 7), 3, None), (False, (4, 5), 3, None), (False, (2, 32), 37, None), (False, (4, 25), 3, None),
               (True, (1, 7), 3, None), (True, (2, 32), 37, None), (True, (4, 25), 3, None),
               # the reduced-precision heads lay the same workspace out differently (bf16 keys / values, extra transposes,
               # the token GEMM) while tpspp_nrtr_*_workspace takes no flags: is the queried size enough there too?
               (True, (2, 32), 37, torch.bfloat16), (True, (4, 25), 3, torch.bfloat16),
               (True, (2, 32), 37, "bf16x3"), (True, (4, 25), 3, "bf16x3")]


@gpu
@sweeps("tpspp_nrtr_encoder_fwd", "tpspp_nrtr_decoder_fwd")
@pytest.mark.parametrize("full,hw,n,cd", HEAD_SHAPES, ids=[f"{'full' if c[0] else 'small'}-{c[1][0]}x{c[1][1]}-n{c[2]}-{c[3]}"
                                                            for c in HEAD_SHAPES])
@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "pipeline"])
def test_head_encoder_and_decoder(cuda, full, hw, n, cd, persist):
    """Token counts 7, 20, 64, 100; n = 3 and 37 (no multiple of the persistent step's 32-image cluster); the small head
    (launch pipeline only) and the full-width head (persistent step kernel unless TPSPP_HEAD_NO_PERSIST), exact fp32,
    bf16 (TPSPP_HEAD_BF16) and bf16x3 (TPSPP_HEAD_BF16X3); greedy and teacher-forced; the modules are fresh, so their
    workspaces are allocated at exactly tpspp_nrtr_encoder_workspace / tpspp_nrtr_decoder_workspace bytes.  Tokens and the
    status word are integer outputs: the guarded run must equal the plain one."""
    enc, dec, C = _head_modules(full)
    enc.compute_dtype = dec.compute_dtype = cd
    feat = t(synth.dyadic((n, C) + hw, f"ms.head.{hw}", 6))
    metas = [dict(valid_ratio=(1.0, 0.37, 0.81, 0.5, 0.95)[i % 5]) for i in range(n)]
    L = dec.max_seq_len
    forced = torch.randint(0, 90, (n, L), generator=torch.Generator().manual_seed(n))
    forced[:, 0] = 91
    forced[::3, L - 1] = 92
    old = os.environ.pop("TPSPP_HEAD_NO_PERSIST", None)

    def fn(put):
        e, d = put_module(enc, put), put_module(dec, put)
        with torch.no_grad():
            oe = e(put(feat), metas)
            od = d(None, oe, None, metas, train_mode=False)
            tok = d.last_tokens.clone()
            otf = d(None, oe, dict(padded_targets=put(forced)), metas, train_mode=True)
        return (oe, od, tok, otf)
    try:
        if not persist:
            os.environ["TPSPP_HEAD_NO_PERSIST"] = "1"
        run_twice(cuda, fn)
    finally:
        os.environ.pop("TPSPP_HEAD_NO_PERSIST", None)
        if old is not None:
            os.environ["TPSPP_HEAD_NO_PERSIST"] = old


@gpu
@sweeps("tpspp_attn_tensor2idx_fwd")
@pytest.mark.parametrize("n,L,C", params_of(TH.test_attn_tensor2idx_kernel_against_the_reference_scan))
def test_tensor2idx(cuda, n, L, C):
    g = torch.Generator().manual_seed(n * 1000 + L)
    x = (torch.rand((n, L, C), generator=g) * 8).round() / 8
    x[:, :, C - 2] += (torch.rand((n, L), generator=g) < 0.08).float()
    x[:, :, C - 1] += (torch.rand((n, L), generator=g) < 0.1).float()

    def fn(put):
        idx, val = ops.attn_tensor2idx(put(x), C - 2, C - 1)
        why = "the host copy ops.attn_tensor2idx returns of its guarded int32 device buffer [idx | val bits | status]"
        return (GA.Unguarded(torch.from_numpy(idx.copy()), why), GA.Unguarded(torch.from_numpy(val.copy()), why))
    run_twice(cuda, fn)


import test_ocr_transforms as TO      # noqa: E402


@gpu
@sweeps("tpspp_resize_normalize_fwd")
@pytest.mark.parametrize("keep,mn,mx,pad", params_of(TO.test_gpu_batch_preprocessor_equals_oracle))
@pytest.mark.parametrize("backend", ["cv2", "pillow"])
def test_resize_normalize(cuda, keep, mn, mx, pad, backend):
    from tps_pp_amd.ocr_transforms import NormalizeOCR, OCRBatchPreprocessor, ResizeOCR
    imgs = TO.ragged_images(23, 3)

    def fn(put):
        pre = OCRBatchPreprocessor(ResizeOCR(32, min_width=mn, max_width=mx, keep_aspect_ratio=keep, img_pad_value=pad,
                                             **({"backend": "pillow"} if backend == "pillow" else {})),
                                   NormalizeOCR(TO.MEAN, TO.STD), cuda)
        return pre(imgs)[0]
    run_twice(cuda, fn)


@gpu
def test_zz_sweep_totals():
    """After a whole run of this file: every entry point a case declares as reached at some shapes was reached at one;
    prints how much went through the guards in this process (run with -s to see it)."""
    print(f"\nmemory-safety sweep: {GA.TOTALS['allocations']} guarded allocations and {GA.TOTALS['inputs']} guarded inputs "
          f"checked, {GA.TOTALS['bytes'] / 2 ** 20:.1f} MiB of payload")
    assert len(PARTLY_WRITTEN) == len({e[0] for e in PARTLY_WRITTEN})
    for name, reached in REACHED.items():
        missing = set(globals()[name]._sometimes) - reached
        assert not missing, f"{name} declares {sorted(missing)} but no case of it called them"
