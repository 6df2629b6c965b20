"""The case table of tests/test_warp_bwd_route_host.py (CPU) and tests/test_gpu_warp_bwd_routes.py (-m gpu): shapes, flags and
alignments that reach every kernel `tpspp_warp_bwd` can pick -- the five sampling families, the sixteen forms of kernel A''
and the 60 instantiations of the parameter kernel --, each with the route `ops.warp_backward_route` must name for it, and
the builders of their inputs and float64 references.  Nothing here needs a GPU.

The backward takes grid, T, p_hat, p_hat_t, p_xy, inv_delta_c and score as ARGUMENTS: none of them has to come from a
forward call.  Comparison A ("exact") chooses all of them so that every product and every partial sum of every accumulator
of every route is exactly representable in fp32, in any order:
  * a grid coordinate g is an fp32 number for which the kernels' own fp32 expression ((g + 1) * 0.5) * (size - 1) lands on
    a multiple of 2^-FB (FB = 3) without rounding (`axis_candidates` searches them and `exact_bits` re-checks every point):
    ix, iy, the fractions and 1 - fraction have <= 3 fractional bits, the four tap weights <= 6;
  * images, output gradients, tables, T, the score (0.5 s + 1 exact) and inv_delta_c are small integers or halves, thinned
    out per case (`Case.thin`) where many pixels meet in one accumulator.
`exact_bits(case)` evaluates every accumulator on absolute values -- the sum of |terms| in units of the accumulator's finest
bit -- and the host test requires the largest below 2^24: then no order of additions (LDS or global float atomics, slices,
per-lane chains, fp64 or fixed point) can round, and every output must EQUAL the float64 reference.

`reference(data, fault=...)` is the float64 reference; a `fault` is one of FAULTS, a seeded defect of the reference itself,
which the host test uses to show that each case's expected values would move if a kernel had that defect."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tps_pp_amd import ops, synth

f32 = np.float32
FB = 3                                   # fractional bits of ix / iy in comparison A

Case = namedtuple("Case", "name N C0 in0 C1 in1 out F table transposed score gscore ld_extra need0 need1 fixed bf16 two "
                          "misalign0 pt_offset thin")


def case(name, N, C0, in0, out, F=20, C1=0, in1=None, table=0, transposed=1, score=0, gscore=0, ld_extra=0, need0=True,
         need1=True, fixed=False, bf16=False, two=False, misalign0=False, pt_offset=False, thin=1):
    """table: 0 the classic table [1, x, y, rbf] (F + 3 columns), 1 TPS_PP (F columns + p_xy); transposed: p_hat_t given;
    score: 0 none, 1 (N, n, F), 2 (N, F, n); gscore: dL/d score wanted; ld_extra: columns p_hat carries behind the table's;
    misalign0: g_in0 is a view one float into its buffer; pt_offset: p_hat_t likewise; thin: one output gradient in `thin`
    is non-zero (keeps `exact_bits` under 2^24 where thousands of pixels meet in one accumulator)."""
    return Case(name, N, C0, tuple(in0), C1, tuple(in1) if in1 else None, tuple(out), F, table, transposed, score, gscore,
                ld_extra, need0, need1, fixed, bf16, two, misalign0, pt_offset, thin)


# ---- the table: name -> (case, route) -------------------------------------------------------------------------------------
CL = dict(table=0, transposed=1)                               # the classic rectifier's call
PP = dict(table=1, transposed=0, score=1, gscore=1)            # TPS_PP's call

CLASSIC = [
    (case("classic C1 n=1028 F=1 (LDS = 8 n exactly)", 2, 1, (4, 257), (4, 257), F=1, **CL), "classic"),
    (case("classic C1 n=4096 (LDS = 8 n exactly)", 2, 1, (64, 64), (64, 64), thin=8, **CL), "classic"),
    (case("classic C2 24x33 -> 33x40 F=20", 3, 2, (24, 33), (33, 40), **CL), "classic"),
    (case("classic C3 16x33 -> 33x40 F=21", 2, 3, (16, 33), (33, 40), F=21, **CL), "classic"),
    (case("classic C3 no g_in0", 2, 3, (16, 33), (33, 40), need0=False, **CL), "classic"),
    (case("classic bf16 C1 32x33 (LDS = 8 n exactly)", 2, 1, (32, 33), (32, 33), bf16=True, **CL), "classic_bf16"),
    (case("classic bf16 C3 32x33 -> 33x40", 2, 3, (32, 33), (33, 40), bf16=True, **CL), "classic_bf16"),
    # one step outside each condition
    (case("not classic: n=1024", 2, 1, (32, 32), (32, 32), **CL), "lds2 ppt4 nt256 f64 G1 | params k24 classic T noscore S4"),
    (case("not classic: n=1029 (n % 4)", 2, 1, (32, 33), (3, 343), **CL), "lds2 ppt4 nt1024 f64 G1 | params k24 classic T noscore S4"),
    (case("not classic: C0=4", 2, 4, (16, 33), (33, 40), **CL), "lds2 ppt4 nt1024 f64 G1 | params k24 classic T noscore S5"),
    (case("not classic: F=22", 2, 3, (16, 33), (33, 40), F=22, **CL), "lds2 ppt4 nt1024 f64 G1 | params k36 classic T noscore S5"),
    (case("not classic: no p_hat_t", 2, 3, (16, 33), (33, 40), table=0, transposed=0),
     "lds2 ppt4 nt1024 f64 G1 | params k24 classic N noscore S5"),
    (case("not classic: p_hat_t 4 bytes off", 2, 3, (16, 33), (33, 40), pt_offset=True, **CL),
     "lds2 ppt4 nt1024 f64 G1 | params k24 classic T noscore S5"),
    (case("not classic: fixed point", 2, 3, (16, 33), (33, 40), fixed=True, **CL),
     "lds2 ppt4 nt1024 fix G1 | params k24 classic T noscore S5"),
    (case("not classic: TWO_KERNELS", 2, 3, (16, 33), (33, 40), two=True, **CL),
     "lds2 ppt4 nt1024 f64 G1 | params k24 classic T noscore S5"),
]


def _lds2_forms():
    out = []
    forms = [((16, 16), 1, 256, 1), ((1, 257), 2, 256, 1), ((16, 32), 2, 256, 2), ((19, 27), 4, 256, 2), ((32, 32), 4, 256, 4),
             ((25, 41), 4, 1024, 4), ((64, 64), 4, 1024, 8)]
    for hw, ppt, nt, S in forms:
        n = hw[0] * hw[1]
        for fixed in (False, True):
            for bf16 in (False, True):
                if bf16 and n in (257, 513, 4096) and fixed:
                    continue                                   # (every form has both accumulators in bf16 at its other edge)
                acc = ("fix" if fixed else "f64") + (" bf16" if bf16 else "")
                out.append((case(f"lds2 n={n} {acc}", 2, 3, (8, 9), hw, F=20, C1=2, in1=(8, 17), fixed=fixed, bf16=bf16,
                                 thin=4 if n > 2000 else 1, **PP),
                            f"lds2 ppt{ppt} nt{nt} {acc} G1 | params k24 tpspp N score gscore S{S}"))
    return out


LDS2 = _lds2_forms() + [
    (case("lds2 C=9 | 17 (ragged chunks), G=3 > chunks1", 1, 17, (8, 9), (16, 16), C1=9, in1=(8, 17), thin=2, **PP),
     "lds2 ppt1 nt256 f64 G3 | params k24 tpspp N score gscore S1"),
    (case("lds2 C0=17 C1=3: input 1 has one chunk for G=3", 1, 17, (8, 9), (19, 27), C1=3, in1=(8, 17), fixed=True, thin=2, **PP),
     "lds2 ppt4 nt256 fix G3 | params k24 tpspp N score gscore S2"),
    (case("lds2 G=8 (57 channels, 16 slices)", 1, 57, (2, 4), (16, 16), C1=57, in1=(2, 2), thin=2, **PP),
     "lds2 ppt1 nt256 f64 G8 | params k24 tpspp N score gscore S1"),
    (case("lds2 chunks=2 > G=1 (N=2048)", 2048, 9, (2, 2), (2, 4), C1=9, in1=(2, 4), F=2, **PP),
     "lds2 ppt1 nt256 f64 G1 | params k24 tpspp N score gscore S1"),
    (case("lds2 chunks=2 > G=1 (N=2048) fix bf16", 2048, 9, (2, 4), (2, 4), C1=9, in1=(2, 4), F=2, fixed=True, bf16=True, **PP),
     "lds2 ppt1 nt256 fix bf16 G1 | params k24 tpspp N score gscore S1"),
    (case("lds2 no g_in0", 2, 3, (8, 9), (16, 32), C1=2, in1=(8, 17), need0=False, **PP),
     "lds2 ppt2 nt256 f64 G1 | params k24 tpspp N score gscore S2"),
    (case("lds2 no g_in1", 2, 3, (8, 9), (16, 32), C1=2, in1=(8, 17), need1=False, fixed=True, **PP),
     "lds2 ppt2 nt256 fix G1 | params k24 tpspp N score gscore S2"),
]

LDS = [
    (case("lds: 5x7 plane (140 bytes)", 2, 3, (5, 7), (6, 5), **PP), "lds cpt8,1 G1 | params k24 tpspp N score gscore S1"),
    (case("lds: 17x33 + 17x9, C=9 | 17", 1, 9, (17, 33), (19, 27), C1=17, in1=(17, 9), thin=2, **PP),
     "lds cpt8,8 G3 | params k24 tpspp N score gscore S2"),
    (case("lds: 80x65 plane (20800 bytes: cpt 3) + 80x9 (cpt 8), G=2 > chunks1", 1, 4, (80, 65), (24, 40), C1=3, in1=(80, 9), thin=4, **PP),
     "lds cpt3,8 G2 | params k24 tpspp N score gscore S3"),
    (case("lds: g_in0 one float off", 2, 2, (8, 9), (16, 16), misalign0=True, **PP),
     "lds cpt8,1 G1 | params k24 tpspp N score gscore S1"),
    (case("lds: chunks=3 > G=2 (N=512)", 512, 17, (5, 7), (6, 5), C1=9, in1=(5, 7), F=2, **PP),
     "lds cpt8,8 G2 | params k24 tpspp N score gscore S1"),
    (case("lds: no g_in0", 2, 3, (5, 7), (6, 5), C1=2, in1=(5, 7), need0=False, **PP),
     "lds cpt8,8 G1 | params k24 tpspp N score gscore S1"),
    (case("lds: 9 chunks, G capped at 8 slices", 1, 65, (5, 7), (6, 5), thin=4, **PP),
     "lds cpt8,1 G8 | params k24 tpspp N score gscore S1"),
]

ATOMICS = [
    (case("atomics: n=4100 (41x100), one input", 2, 2, (8, 9), (41, 100), thin=4, **PP),
     "atomics chunks1+0 | params k24 tpspp N score gscore S8"),
    (case("atomics: 129x128 plane, n=30", 2, 1, (129, 128), (6, 5), **PP), "atomics chunks1+0 | params k24 tpspp N score gscore S1"),
    (case("atomics: C0=9 C1=3 (blockIdx.y split)", 2, 9, (4, 9), (41, 100), C1=3, in1=(4, 5), thin=8, **PP),
     "atomics chunks2+1 | params k24 tpspp N score gscore S8"),
    (case("atomics: no g_in0", 2, 2, (8, 9), (41, 100), C1=2, in1=(8, 5), need0=False, thin=8, **PP),
     "atomics chunks1+1 | params k24 tpspp N score gscore S8"),
    (case("atomics: 17 chunks walk 16 slices", 1, 129, (4, 9), (41, 100), thin=32, **PP),
     "atomics chunks17+0 | params k24 tpspp N score gscore S8"),
    (case("atomics: classic 48x160", 2, 1, (48, 160), (48, 160), thin=8, **CL), "atomics chunks1+0 | params k24 classic T noscore S8"),
    (case("atomics: classic 64x256", 2, 1, (64, 256), (64, 256), thin=16, **CL), "atomics chunks1+0 | params k24 classic T noscore S8"),
]


def _params_cases():
    """Each of the 60 instantiations once, on the cheapest sampling route (kernel A'' on a 2x4 plane; every sixth after
    kernel A' on a 3x3 plane), with F, n (hence S and the slices' lengths) and p_hat_ld cycling."""
    out = []
    Fs = {24: (1, 21, 20, 7), 36: (22, 33, 27, 30), 64: (34, 61, 47, 55)}
    # n -> S for N <= 3: S is the largest count with ceil(n / S) >= 256, i.e. n >= 255 S + 1 (511, 766, 1021, 1276, 1531,
    # 1786, 2041): both sides of some thresholds, ragged last slices, lengths off 64 and 256
    ns = [(300, 1), (510, 1), (511, 2), (700, 2), (770, 3), (1030, 4), (1290, 5), (1530, 5), (1533, 6), (1790, 7), (2040, 7),
          (2045, 8), (2100, 8)]
    i = 0
    for kmax in (24, 36, 64):
        for table in (0, 1):
            for transposed in (0, 1):
                for score, gscore in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
                    F = Fs[kmax][i % 4]
                    if score == 2 and F == 1:
                        F = 2                                  # (a transposed (N, 1, n) score is the plain layout)
                    n, S = ns[i % len(ns)]
                    lds = i % 6 == 5
                    N = 1 + i % 3
                    c = case(f"params k{kmax} t{table} T{transposed} s{score} g{gscore} F={F} n={n}", N, 1, (3, 3) if lds else (2, 4),
                             (1, n), F=F, table=table, transposed=transposed, score=score, gscore=gscore, ld_extra=3 * (i % 2),
                             two=True, thin=2 if n < 1000 else 4)
                    samp = "lds cpt8,1 G1" if lds else f"lds2 ppt{1 if n <= 256 else 2 if n <= 512 else 4} nt{256 if n <= 1024 else 1024} f64 G1"
                    out.append((c, f"{samp} | params k{kmax} {'tpspp' if table else 'classic'} {'T' if transposed else 'N'} "
                                   f"{('noscore', 'score', 'score_t')[score]}{' gscore' if gscore else ''} S{S}"))
                    i += 1
    # S through N: ceil(2048 / N) workgroups per image
    out.append((case("params S=2 through N=1024", 1024, 1, (2, 2), (1, 512), F=3, table=1, transposed=0, score=1, gscore=1, thin=2),
                "lds2 ppt2 nt256 f64 G1 | params k24 tpspp N score gscore S2"))
    out.append((case("params S=3 through N=683", 683, 1, (2, 2), (1, 768), F=3, table=0, transposed=1, two=True, thin=2),
                "lds2 ppt4 nt256 f64 G1 | params k24 classic T noscore S3"))
    return out


PARAMS = _params_cases()
ALL = CLASSIC + LDS2 + LDS + ATOMICS + PARAMS
CASES = {c.name: c for c, _ in ALL}
ROUTES = {c.name: r for c, r in ALL}
assert len(CASES) == len(ALL)

# comparison B (real data): one or two cases per sampling family
REAL = ["classic C2 24x33 -> 33x40 F=20", "classic bf16 C3 32x33 -> 33x40", "lds2 n=1024 f64", "lds2 n=1025 fix",
        "lds: 17x33 + 17x9, C=9 | 17", "lds: 80x65 plane (20800 bytes: cpt 3) + 80x9 (cpt 8), G=2 > chunks1",
        "atomics: C0=9 C1=3 (blockIdx.y split)", "atomics: classic 48x160"]


# ---- shapes only: the route of a case --------------------------------------------------------------------------------------
def n_of(c):
    return c.out[0] * c.out[1]


def cols_of(c):
    return (c.F if c.table else c.F + 3) + c.ld_extra


def _offset_view(shape, dtype=torch.float32):
    """An uninitialised tensor of `shape` one element into its buffer: its address is 4 (2) bytes off a 16-byte boundary."""
    numel = int(np.prod(shape))
    return torch.empty(numel + 4, dtype=dtype)[1:1 + numel].view(shape)


def route_of(c, N=None):
    """`ops.warp_backward_route` on uninitialised CPU tensors of the case's shapes, dtypes and alignments."""
    N = c.N if N is None else N
    io = torch.bfloat16 if c.bf16 else torch.float32
    n = n_of(c)
    e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt)                   # noqa: E731
    in1 = e(N, c.C1, *c.in1, dt=io) if c.C1 else None
    score = None
    if c.score == 1:
        score = e(N, n, c.F)
    elif c.score == 2:
        score = e(N, c.F, n).transpose(1, 2)
    pt = None
    if c.transposed:
        pt = _offset_view((cols_of(c), n)) if c.pt_offset else e(cols_of(c), n)
    return ops.warp_backward_route(
        e(N, c.C0, *c.out, dt=io), e(N, c.C0, *c.in0, dt=io), e(N, n, 2), e(N, c.F, 2), e(c.F + 3, c.F + 3), e(n, cols_of(c)),
        c.out, P_xy=e(n, 2) if c.table else None, score=score, in1=in1, g_out1=e(N, c.C1, *c.out, dt=io) if c.C1 else None,
        P_hat_t=pt, need_in0=c.need0, need_in1=c.need1, need_score=bool(c.gscore), fixed_point=c.fixed, two_kernels=c.two,
        g_in0=_offset_view((N, c.C0) + c.in0, io) if c.misalign0 else None)


# ---- comparison A: exactly representable data --------------------------------------------------------------------------------
def kernel_coord(g, size):
    """ix (or iy) as every sampling kernel computes it, in fp32, before the clamp."""
    return ((g.astype(f32) + f32(1)) * f32(0.5)).astype(f32) * f32(size - 1)


@functools.lru_cache(maxsize=None)
def axis_candidates(size):
    """(g, ix): the fp32 grid coordinates whose kernel_coord is a multiple of 2^-FB inside [0, size - 1], exactly (no
    rounding in any of the three fp32 operations), sorted by ix.  u = q / 2^FB always works (ix = q (size - 1) / 2^FB: the
    two borders among them); the rest, pixel centres included, is searched."""
    t = np.arange(0, (size - 1) * 2 ** FB + 1, dtype=np.float64) / 2 ** FB
    u0 = (t / max(size - 1, 1)).astype(f32)
    us = np.concatenate([u0, np.nextafter(u0, f32(2)), np.nextafter(u0, f32(-1)), np.arange(2 ** FB + 1, dtype=f32) / f32(2 ** FB)])
    g = (2.0 * us.astype(np.float64) - 1.0).astype(f32)
    ok = ((g.astype(np.float64) + 1.0) * 0.5 == us.astype(np.float64))                       # g + 1 and * 0.5 exact
    ix = us.astype(np.float64) * (size - 1)
    ok &= (ix == kernel_coord(g, size).astype(np.float64)) & (ix * 2 ** FB == np.floor(ix * 2 ** FB))
    g, ix = g[ok], ix[ok]
    _, first = np.unique(ix, return_index=True)
    return g[first], ix[first]


BEYOND = np.array([-1.5, 1.25, -2.0, 3.0, -1.0, 1.0], f32)       # clamped on either side, far and exactly at the border


def exact_grid(c):
    """(N, n, 2) fp32.  In runs of 16 pixels (4 for tiny outputs), rotating with the image, one of four patterns:
      0 smooth: neighbouring lanes about one tap apart, a fractional offset (the classic kernel's DPP hand-over pattern);
      1 the same with a jump in the middle of the wavefront and the row order reversed at its end (the pattern breaks);
      2 edges: beyond -1 / +1, exactly on the border, exactly on pixel centres, the last column / row;
      3 a fold: every pixel of the wavefront onto one of two taps.
    Coordinates are taken from `axis_candidates` (nearest to the pattern's wish), so each is exact whatever the size."""
    H, W = c.in0
    H1, W1 = c.in1 or c.in0
    n, (Ho, Wo) = n_of(c), c.out
    run = 16 if n >= 256 else 4                                 # pixels per pattern: four patterns in every wavefront
    p = np.arange(n)
    r, col = p // Wo, p % Wo
    out = np.zeros((c.N, n, 2), f32)
    for b in range(c.N):
        pat = ((p // run) + b) % 4
        for axis, size, size1, pos, cnt in ((0, W, W1, col, Wo), (1, H, H1, r, Ho)):
            g, ix = axis_candidates(size)
            both = np.isin(g, axis_candidates(size1)[0])        # exact for input 1 as well
            g, ix = g[both], ix[both]
            lane = p % 64
            wish = pos * (size - 1) / max(cnt - 1, 1) * 0.75 + 0.375 + 0.125 * (b % 3)           # smooth
            if axis == 0:
                wish = np.where(pat == 0, (pos % size) + 0.25, wish)                             # one tap per lane
            brk = np.where(lane >= 32, wish + 3.0, wish)
            brk = np.where(lane == 63, 0.5, brk)
            fold = np.where(lane % 2 == 0, 1.0 + 0.375, 1.0 + 0.875) + (axis == 1) * (0.125 - 1.0)
            wish = np.where(pat == 1, brk, np.where(pat == 3, fold, wish))
            k = np.clip(np.searchsorted(ix, wish), 1, len(ix) - 1)
            k = np.where(np.abs(ix[k - 1] - wish) <= np.abs(ix[k] - wish), k - 1, k)
            v = g[k]
            # the edge pattern: far out, on the border, pixel centres (candidates with a whole ix), the last pixel
            whole = g[ix == np.floor(ix)]
            sel = (lane + (17 if axis else 0) + b) % 16
            edge = np.where(sel < len(BEYOND), BEYOND[sel % len(BEYOND)], whole[(p * 7 + sel) % len(whole)])
            v = np.where(pat == 2, edge, v)
            out[b, :, axis] = v
    return out


def _ints(shape, name, lo, hi):
    u = (synth.dyadic(shape, name).astype(np.float64) + 1.0) * 0.5
    return np.floor(lo + u * (hi - lo + 1)).clip(lo, hi).astype(f32)


def _thin(a, name, keep_one_in):
    if keep_one_in <= 1:
        return a
    u = (synth.dyadic(a.shape, name + ".thin").astype(np.float64) + 1.0) * 0.5
    return np.where(u * keep_one_in < 1.0, a, f32(0)).astype(f32)


def _tables(c, tag, exact):
    n, K = n_of(c), c.F + 3
    cols = cols_of(c)
    if exact:
        # (about 256 non-zero pixels per table column: dL/dT adds a column over ALL n pixels)
        ph = _thin(_ints((n, cols), tag + ".ph", -2, 2), tag + ".ph", max(1, n // 256))
        xy = _ints((n, 2), tag + ".xy", -2, 2) * f32(0.5) if c.table else None
        inv = _thin(_ints((K, K), tag + ".inv", -1, 1), tag + ".inv", max(1, K // 4))
        T = _ints((c.N, K, 2), tag + ".T", -2, 2)
        sc = _ints((c.N, n, c.F), tag + ".sc", -2, 2) if c.score else None
    else:
        ph = synth.dyadic((n, cols), tag + ".ph", 1)
        xy = synth.dyadic((n, 2), tag + ".xy", 1) if c.table else None
        inv = synth.dyadic((K, K), tag + ".inv", 1, 4.0)
        T = synth.dyadic((c.N, K, 2), tag + ".T", 1)
        sc = synth.dyadic((c.N, n, c.F), tag + ".sc", 1, 0.5) if c.score else None
    if c.ld_extra:
        ph[:, cols - c.ld_extra:] = f32(99.0)                   # columns behind the table's: nothing may read them
    return ph, xy, inv, T, sc


def make_data(c, exact=True, grid=None):
    """dict of numpy arrays (fp32 values; bf16-exact where the case is bf16): in0, g0, in1, g1, grid, T, inv, ph (n, ld),
    xy, score (N, n, F) logical layout.  exact=False: dyadic reals (rounded to bf16 for a bf16 case) and the given grid."""
    tag = c.name + (".exact" if exact else ".real")
    n = n_of(c)
    d = dict(case=c)
    for i, (C, hw) in enumerate(((c.C0, c.in0), (c.C1, c.in1))):
        if not C:
            d[f"in{i}"] = d[f"g{i}"] = None
            continue
        if exact:
            d[f"in{i}"] = _ints((c.N, C) + hw, f"{tag}.in{i}", -2, 2)
            d[f"g{i}"] = _thin(_ints((c.N, C) + c.out, f"{tag}.g{i}", -2, 2), f"{tag}.g{i}", c.thin)
        else:
            rnd = (lambda a: torch.from_numpy(a).bfloat16().float().numpy()) if c.bf16 else (lambda a: a)
            d[f"in{i}"] = rnd(synth.dyadic((c.N, C) + hw, f"{tag}.in{i}", 1))
            d[f"g{i}"] = rnd(synth.dyadic((c.N, C) + c.out, f"{tag}.g{i}", 1))
    d["grid"] = exact_grid(c) if exact else np.ascontiguousarray(grid, f32).reshape(c.N, n, 2)
    d["ph"], d["xy"], d["inv"], d["T"], d["score"] = _tables(c, tag, exact)
    return d


# ---- the float64 reference ---------------------------------------------------------------------------------------------------
FAULTS = ("drop_border_tap", "swap_ne_sw", "clip_factor_kept", "W_for_W_minus_1", "ragged_channel_dropped", "last_slice_dropped",
          "score_on_affine_columns")


def plan_numbers(c):
    """(cpt0, cpt1, S) of the case's route, from the planner."""
    r = route_of(c)
    return (r.cpt0 or 8, r.cpt1 or 8, r.S if r.params else 1)


def taps(grid, H, W, fault=None):
    """The kernels' fp32 tap expressions on an (N, n, 2) grid: dict of x0, y0 (int), w, nn, e, s (fp32 as float64), inx, iny,
    mx, my (the border-clip factors)."""
    Wm = W if fault == "W_for_W_minus_1" else W - 1
    ix = ((grid[..., 0] + f32(1)) * f32(0.5)).astype(f32) * f32(Wm)
    iy = ((grid[..., 1] + f32(1)) * f32(0.5)).astype(f32) * f32(H - 1)
    cx, cy = (ix <= 0) | (ix >= f32(W - 1)), (iy <= 0) | (iy >= f32(H - 1))
    ix = np.clip(ix, f32(0), f32(W - 1)).astype(f32)
    iy = np.clip(iy, f32(0), f32(H - 1)).astype(f32)
    fx, fy = np.floor(ix), np.floor(iy)
    w, nn = (ix - fx).astype(f32), (iy - fy).astype(f32)
    e, s = (f32(1) - w).astype(f32), (f32(1) - nn).astype(f32)
    keep = fault == "clip_factor_kept"
    t = dict(x0=fx.astype(np.int64), y0=fy.astype(np.int64), w=w, nn=nn, e=e, s=s)
    t["inx"], t["iny"] = (t["x0"] + 1) < W, (t["y0"] + 1) < H
    t["mx"] = np.where(cx & (not keep), 0.0, (W - 1) * 0.5)
    t["my"] = np.where(cy & (not keep), 0.0, (H - 1) * 0.5)
    t["wts"] = [(s * e).astype(f32), (s * w).astype(f32), (nn * e).astype(f32), (nn * w).astype(f32)]       # nw ne sw se
    return t


def sample_reference(img, g, grid, cpt, fault=None, absolute=False):
    """Sampler backward of one input in float64 on the kernels' fp32 taps: (dL/d input (N, C, H, W), its mass of |terms|, the
    number of terms per element, dL/d grid contribution (N, n, 2), the same on absolute values).  A term is the kernels'
    fp32 product weight * g (exact in comparison A)."""
    N, C, H, W = img.shape
    n = grid.shape[1]
    t = taps(grid, H, W, fault)
    gg = g.reshape(N, C, n).astype(np.float64)
    if fault == "ragged_channel_dropped" and C % cpt:
        gg = gg.copy()
        gg[:, C - 1] = 0.0
    o00 = t["y0"] * W + t["x0"]
    offs = [o00, o00 + 1, o00 + W, o00 + W + 1]
    oks = [np.ones_like(t["inx"]), t["inx"], t["iny"], t["inx"] & t["iny"]]
    wts = list(t["wts"])
    if fault == "swap_ne_sw":
        wts[1], wts[2] = wts[2], wts[1]
    if fault == "drop_border_tap":                              # the first tap with a weight on the image's border
        for k in (0, 1, 2, 3):
            yy, xx = offs[k] // W, offs[k] % W
            hit = oks[k] & (wts[k] > 0) & ((yy == 0) | (xx == 0) | (yy == H - 1) | (xx == W - 1)) & (np.abs(gg).sum(1) > 0)
            if hit.any():
                b, p = np.argwhere(hit)[0]
                wts[k] = wts[k].copy()
                wts[k][b, p] = 0
                break
    size = N * C * H * W
    tot, mass, cnt = np.zeros(size), np.zeros(size), np.zeros(size)
    base = (np.arange(N)[:, None, None] * C + np.arange(C)[None, :, None]) * (H * W)
    flat = img.reshape(N, C, H * W).astype(np.float64)
    v = []
    for wt, ok, of in zip(wts, oks, offs):
        term = (wt[:, None, :] * gg.astype(f32)).astype(f32).astype(np.float64)               # the kernels' fp32 product
        sel = np.broadcast_to(ok[:, None, :], term.shape)
        idx = (base + np.where(ok, of, 0)[:, None, :])[sel]
        tot += np.bincount(idx, term[sel], size)
        mass += np.bincount(idx, np.abs(term[sel]), size)
        cnt += np.bincount(idx, None, size)
        v.append(np.where(ok[:, None, :], np.take_along_axis(flat, np.broadcast_to(np.where(ok, of, 0)[:, None, :], term.shape), 2), 0.0))
    v00, a01, a10, a11 = v
    w, nn, e, s = (t[k].astype(np.float64)[:, None, :] for k in ("w", "nn", "e", "s"))
    A = np.abs
    gx = (((a01 - v00) * s + (a11 - a10) * nn) * gg).sum(1) * t["mx"]
    gy = (((a10 - v00) * e + (a11 - a01) * w) * gg).sum(1) * t["my"]
    ax = (((A(a01) + A(v00)) * s + (A(a11) + A(a10)) * nn) * A(gg)).sum(1) * t["mx"]
    ay = (((A(a10) + A(v00)) * e + (A(a11) + A(a01)) * w) * A(gg)).sum(1) * t["my"]
    shape = (N, C, H, W)
    return tot.reshape(shape), mass.reshape(shape), cnt.reshape(shape), np.stack([gx, gy], -1), np.stack([ax, ay], -1)


def rows_of(d, fault=None):
    """row(p) of every image in float64, (N, n, K): [1, x, y, rbf (0.5 s + 1)] (TPS_PP) or the table's K columns (classic,
    the columns from 3 on times the score factor when a score is given), and the bare rbf columns (n, F) of dL/d score."""
    c = d["case"]
    N, n, F = c.N, n_of(c), c.F
    ph = d["ph"].astype(np.float64)
    if c.table:
        head = np.concatenate([np.ones((n, 1)), d["xy"].astype(np.float64)], 1)
        rbf = ph[:, :F]
    else:
        head, rbf = ph[:, :3], ph[:, 3:F + 3]
    rows = np.broadcast_to(np.concatenate([head, rbf], 1)[None], (N, n, F + 3)).copy()
    if c.score:
        fac = 0.5 * d["score"].astype(np.float64) + 1.0
        rows[:, :, 3:] *= fac
        if fault == "score_on_affine_columns":
            rows[:, :, :3] *= fac[:, :, :3] if F >= 3 else fac[:, :, :1]
    return rows, rbf


def params_reference(d, gg, fault=None, S=1):
    """dL/d control points (N, F, 2), dL/d score (N, n, F) | None and dL/dT (N, K, 2) in float64 from dL/d grid `gg`
    (N, n, 2) -- the reference's own, or a kernel's read back from the workspace (stage 2)."""
    c = d["case"]
    rows, rbf = rows_of(d, fault)
    g2 = gg.astype(np.float64)
    if fault == "last_slice_dropped" and S > 1:
        per = (n_of(c) + S - 1) // S
        g2 = g2.copy()
        g2[:, (S - 1) * per:] = 0.0
    gT = np.einsum("bpk,bpx->bkx", rows, g2)
    g_ctrl = np.einsum("kf,bkx->bfx", d["inv"].astype(np.float64), gT)[:, :c.F]
    g_score = None
    if c.score:
        g_score = 0.5 * rbf[None] * np.einsum("bpx,bkx->bpk", gg.astype(np.float64), d["T"].astype(np.float64)[:, 3:])
    return g_ctrl, g_score, gT


def reference(d, fault=None):
    """Every output of the call in float64: g_in0, g_in1 (None where the case has no such input; computed whether or not the
    case asks for them), g_grid (N, n, 2), g_ctrl, g_score, and the masses / term counts of the bars."""
    c = d["case"]
    cpt0, cpt1, S = plan_numbers(c)
    out = dict(g_in1=None)
    gg = 0.0
    for i, cpt in ((0, cpt0), (1, cpt1)):
        if d[f"in{i}"] is None:
            continue
        tot, mass, cnt, g, ga = sample_reference(d[f"in{i}"], d[f"g{i}"], d["grid"], cpt, fault)
        out[f"g_in{i}"], out[f"mass{i}"], out[f"cnt{i}"] = tot, mass, cnt
        gg = gg + g
        out["abs_grid"] = out.get("abs_grid", 0.0) + ga
    out["g_grid"] = gg
    out["g_ctrl"], out["g_score"], out["gT"] = params_reference(d, gg, fault, S)
    return out


def exact_bits(d, ref=None):
    """Comparison A's proof obligation: for every kind of accumulator the largest sum of |terms| in units of its finest bit
    (dict kind -> float); all below 2^24 means that no partial sum in any order needs more than fp32's 24 bits.  Also
    checks that every grid point sits on the 2^-FB lattice.  Units: a tap weight has 2 FB fractional bits and the data are
    integers (dL/d input: 2^-2FB); a coordinate-gradient term has FB, times a half-integer border-clip factor (dL/d grid:
    2^-(FB+1)); a row entry is a half -- p_xy, or a whole table entry times the half-integer score factor -- (dL/dT:
    2^-(FB+2)); dL/d score is 0.5 x a whole table entry x dL/d grid x a whole T (2^-(FB+2)); inv_delta_c is whole (dL/d
    control points: dL/dT's unit)."""
    c = d["case"]
    ref = ref or reference(d)
    for i in (0, 1):
        if d[f"in{i}"] is not None:
            H, W = d[f"in{i}"].shape[2:]
            for ax, size in ((0, W), (1, H)):
                v = kernel_coord(d["grid"][..., ax], size).astype(np.float64)
                assert (v * 2 ** FB == np.floor(v * 2 ** FB)).all(), (c.name, "grid off the lattice")
    bits = {}
    bits["dL/d input"] = max(float(ref[f"mass{i}"].max()) for i in (0, 1) if d[f"in{i}"] is not None) * 2 ** (2 * FB)
    ag = ref["abs_grid"]
    bits["dL/d grid"] = float(ag.max()) * 2 ** (FB + 1)
    rows, rbf = rows_of(d)
    aT = np.einsum("bpk,bpx->bkx", np.abs(rows), ag)
    unit = 2 ** (FB + 2)
    bits["dL/dT"] = float(aT.max()) * unit
    bits["dL/d control points"] = float(np.einsum("kf,bkx->bfx", np.abs(d["inv"]).astype(np.float64), aT).max()) * unit
    if c.score:
        bits["dL/d score"] = float((0.5 * np.abs(rbf)[None] * np.einsum("bpx,bkx->bpk", ag, np.abs(d["T"]).astype(np.float64)[:, 3:])).max()) * unit
    return bits


def round_bf16(a):
    """float64 -> the nearest bf16 (ties to even) as float64; comparison A's sums are fp32 numbers, so this is one rounding."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
    assert torch.equal(t.double(), torch.from_numpy(np.ascontiguousarray(a))), "the exact sum is not an fp32 number"
    return t.bfloat16().double().numpy()


# ---- comparison B: real data and derived bars ---------------------------------------------------------------------------------
AMPS = np.array([0.1, 0.6, 3.0], f32)        # control-point perturbations per image: gentle, folded, clamped borders
U = 2.0 ** -24                               # one fp32 rounding, relative


def real_case(name):
    """The REAL case `name` at N = 3, so that it sees all of AMPS: one gentle, one folded and one clamped image."""
    return CASES[name]._replace(N=3)


def make_real(c):
    """Real-valued inputs of a REAL case with the project's own tables for its output geometry (F = 20): dict as make_data's
    plus ctrl (N, F, 2); T = inv_delta_c [ctrl; 0] in float64, rounded to fp32; `grid` is a host rendering of row(p) T
    (float64, rounded) that the GPU test replaces by the forward kernel's own grid output."""
    from tps_pp_amd import constants
    assert c.F == 20 and not c.ld_extra
    d = make_data(c, exact=False, grid=np.zeros((c.N, n_of(c), 2), f32))
    amp = AMPS[np.arange(c.N) % 3, None, None]
    if c.table:
        K = constants.tpspp(c.out, (2, 10))
        d["inv"], d["ph"], d["xy"] = (np.ascontiguousarray(K[k], f32) for k in ("hat_C", "P_hat", "P_xy"))
        d["ctrl"] = (constants.tpspp_initial_ctrl((2, 10))[None] + 0.1 * amp * synth.dyadic((c.N, 20, 2), c.name + ".ctrl", 1)).astype(f32)
    else:
        K = constants.classic(20, c.out)
        d["inv"], d["ph"], d["xy"] = np.ascontiguousarray(K["inv_delta_C"], f32), np.ascontiguousarray(K["P_hat"], f32), None
        d["ctrl"] = (constants.classic_initial_ctrl(20)[None] + amp * synth.dyadic((c.N, 20, 2), c.name + ".ctrl", 1)).astype(f32)
    full = np.concatenate([d["ctrl"].astype(np.float64), np.zeros((c.N, 3, 2))], 1)
    d["T"] = np.einsum("kj,bjx->bkx", d["inv"].astype(np.float64), full).astype(f32)
    rows, _ = rows_of(d)
    d["grid"] = np.einsum("bpk,bkx->bpx", rows, d["T"].astype(np.float64)).astype(f32)
    return d


def k_grid(c, r):
    """The count of fp32 roundings on the longest path from the inputs to one element of dL/d grid, read off
    tpspp_warp_bwd.hip (tap weights and fractions are the reference's own fp32 values and cost nothing):
      4  the per-channel expression ((a01 - v00) * s + (a11 - a10) * nn) * g: subtract, multiply, add, multiply
         (contraction into FMAs can only remove roundings);
      +  one addition per channel of the longest chain gx += ...: every channel a workgroup handles (classic: C0; A'': all
         channels of its chunks, at most max(C0, C1); A': cpt per chunk; A: 8);
      1  the product with the border-clip factor;
      +  the additions that join partial results: one per chunk a workgroup (A': into its LDS sum) or a thread (A: in a
         register) walks, then slots - 1 for the slices, which the parameter kernel adds in ascending order (all routes)."""
    if r.family in ("classic", "classic_bf16"):
        return 4 + c.C0 + 1
    if r.family == "lds2":
        return 4 + max(c.C0, c.C1) + 1 + (r.slots - 1)
    if r.family == "lds":
        walks = -(-max(r.chunks0, r.chunks1) // r.G)
        return 4 + max(r.cpt0, r.cpt1) + 1 + walks + (r.slots - 1)
    walks = -(-(r.chunks0 + r.chunks1) // r.slots)
    return 4 + 8 + 1 + walks + (r.slots - 1)


def l_chain(c, r):
    """L, the longest per-lane fp32 FMA chain of dL/dT: the parameter kernel gives a lane four pixels of every 256 of its
    slice of ceil(n / S) pixels (4 ceil(ceil(n / S) / 256) FMAs, then fp64); the one-launch kernel adds 8-term chains in fp64."""
    if not r.params:
        return 8
    per = -(-n_of(c) // r.S)
    return 4 * -(-per // 256)


def stage1_bars(c, r, ref):
    """Element-wise bounds of stage 1 (dict like the outputs').  dL/d input: |error| <= 2^-24 |S| + 1e-14 M where the
    accumulator is fp64 or fixed point (one final rounding), 2^-24 |S| + t 2^-24 M on the fp32-atomic routes (A', A: one
    rounding per addition, t terms), S the exact sum of the kernel's fp32 terms, M their absolute mass; bf16 I/O adds the one
    rounding to bf16, 2^-8 relative (8 significant bits).  dL/d grid: k_grid 2^-24 A, A the expression on absolute values."""
    out = {}
    for i in (0, 1):
        if ref.get(f"g_in{i}") is None:
            continue
        S, M, t = np.abs(ref[f"g_in{i}"]), ref[f"mass{i}"], ref[f"cnt{i}"]
        b = U * S + (t * U * M if r.family in ("lds", "atomics") else 1e-14 * M)
        if c.bf16:
            b = b + 2.0 ** -8 * (S + b)
        out[f"g_in{i}"] = b
    out["g_grid"] = k_grid(c, r) * U * ref["abs_grid"] * (1 + 64 * U)
    return out


def stage2(d, c, r, gg, fault=None):
    """Stage 2: (reference, bound) of dL/d control points and of dL/d score in float64 from a given dL/d grid `gg` (the
    kernel's own, read back from the workspace).  dL/dT[k] is off by at most (L + 2) 2^-24 A_T[k] -- L FMA roundings of the
    lane's chain plus the two of row = rbf * (0.5 s + 1), A_T = sum_p |row| |dL/d grid| --, which inv_delta_c^T carries into
    dL/d control points in float64 (sum_k |inv[k, f]| bound_k), plus the one final rounding; dL/d score = 0.5 rbf (gx T0 +
    gy T1): four roundings of the expression on absolute values."""
    g_ctrl, g_score, gT = params_reference(d, gg, fault, r.S if r.params else 1)
    rows, rbf = rows_of(d)
    A = np.abs
    aT = np.einsum("bpk,bpx->bkx", A(rows), A(gg.astype(np.float64)))
    bT = (l_chain(c, r) + 2) * U * aT + 1e-14 * aT
    b_ctrl = np.einsum("kf,bkx->bfx", A(d["inv"].astype(np.float64)), bT)[:, :c.F] + U * A(g_ctrl)
    b_score = None
    if c.score:
        b_score = 4 * U * 0.5 * A(rbf)[None] * np.einsum("bpx,bkx->bpk", A(gg.astype(np.float64)), A(d["T"].astype(np.float64))[:, 3:])
    return (g_ctrl, b_ctrl), (g_score, b_score)


# ---- failure reports -------------------------------------------------------------------------------------------------------------
TAP_NAMES = ("nw", "ne", "sw", "se")


def report(c, r, d, what, got, want, bound=None):
    """None if `got` matches `want` (equal by value without a bound, |got - want| <= bound with one), else a message that
    names the route, the worst element, and where the kernels meet it: for dL/d input the plane, its channel chunk and the
    output pixels whose taps land on the element (pixel, tap, weight); for dL/d grid the output pixel, its north-west tap in
    either input and its slice of the parameter kernel; for the parameter outputs the control point / the pixel and column."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return f"{c.name} [{r}] {what}: shape {got.shape}, expected {want.shape}"
    err = np.abs(got - want)
    err = np.where(np.isnan(got), np.inf, err)
    bad = err > (0.0 if bound is None else bound)
    if not bad.any():
        return None
    score = np.where(bad, err / (1e-300 if bound is None else np.maximum(bound, 1e-300)), 0.0)
    at = np.unravel_index(int(np.argmax(score)), got.shape)
    head = (f"{c.name} [{r}] {what}: {int(bad.sum())} of {bad.size} elements wrong; the worst at {tuple(int(i) for i in at)}: got "
            f"{got[at]!r}, expected {want[at]!r}" + ("" if bound is None else f", |error| {err[at]:.3e} > bound {np.broadcast_to(bound, got.shape)[at]:.3e}"))
    n, Wo = n_of(c), c.out[1]
    per = -(-n // max(r.S, 1))
    if what in ("g_in0", "g_in1"):
        i = int(what[-1])
        b, ch, y, x = (int(v) for v in at)
        H, W = d[f"in{i}"].shape[2:]
        t = taps(d["grid"][b:b + 1], H, W)
        o00 = (t["y0"] * W + t["x0"])[0]
        offs = [o00, o00 + 1, o00 + W, o00 + W + 1]
        oks = [np.ones(n, bool), t["inx"][0], t["iny"][0], (t["inx"] & t["iny"])[0]]
        hits = [(int(p), TAP_NAMES[k], float(t["wts"][k][0][p])) for k in range(4) for p in np.nonzero(oks[k] & (offs[k] == y * W + x))[0]]
        cpt = (r.cpt1 if i else r.cpt0) or 8
        tail = (f"; input {i} plane {ch} (chunk {ch // cpt} of {cpt} channels, channel {ch % cpt} in it), pixel ({y}, {x}); "
                f"{len(hits)} taps land here: " + ", ".join(f"p={p} ({p // Wo}, {p % Wo}) {k} w={w:g}" for p, k, w in hits[:8]))
    elif what == "g_grid":
        b, p, xy = (int(v) for v in at)
        tail = f"; image {b}, output pixel {p} = ({p // Wo}, {p % Wo}), d/d{'xy'[xy]}, slice {p // per} of {r.S}, grid point {d['grid'][b, p]!r}"
        for i in (0, 1):
            if d[f"in{i}"] is not None:
                H, W = d[f"in{i}"].shape[2:]
                t = taps(d["grid"][b:b + 1, p:p + 1], H, W)
                tail += (f"; input {i}: north-west tap ({int(t['y0'][0, 0])}, {int(t['x0'][0, 0])}), fractions w={float(t['w'][0, 0]):g} "
                         f"n={float(t['nn'][0, 0]):g}, clip factors {float(t['mx'][0, 0]):g} {float(t['my'][0, 0]):g}")
    elif what == "g_ctrl":
        b, f, xy = (int(v) for v in at)
        tail = f"; image {b}, control point {f}, d/d{'xy'[xy]} (KMAX {r.kmax}, {r.S} slices of {per} pixels)"
    else:
        b, p, k = (int(v) for v in at)
        tail = f"; image {b}, output pixel {p} = ({p // Wo}, {p % Wo}), slice {p // per} of {r.S}, table column {k + 3} (score column {k})"
    return head + tail
