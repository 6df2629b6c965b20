"""The case table of tests/test_conv_route_host.py (CPU) and tests/test_gpu_conv_routes.py (-m gpu): shapes that reach every
fp32 convolution kernel `tpspp_conv2d_fwd` can pick, each with the route `ops.conv2d_route` must name for it, and the
builders of their inputs and float64 references.  Nothing here needs a GPU.

A case's `route` is the kernel without tuning bit 0; with the bit every case takes the generic kernel (`generic_route`).
Ragged edges on every axis: output maps 3x70 (2x64 tile), 5x50 (4x32), 9x27 (8x16), 3x13 with an odd batch (the two-image
tile) and 2x130 (1x128); Cin = 6 (3x3: a last chunk of 2 of 4 channels) and 40 (1x1: a last chunk of 8 of 32); Cout = 24
(one accumulator, a ragged channel tile) and 72 (two accumulators, one full and one ragged channel tile)."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tps_pp_amd import ops, synth

Case = namedtuple("Case", "name srcs cout k stride N route relu res_mode generic zero_extended")


def case(name, srcs, cout, k, stride, N, route, relu=1, res_mode=0, generic=None, zero_extended=False):
    """`generic`: the route under tuning bit 0 where it is not `generic KxK kc32|kc8`; `zero_extended`: the 3x3 weight is
    CRNN's 2x2 kernel with a zero first row and column (`VeryDeepVgg._hip_weights`)."""
    return Case(name, srcs, cout, k, stride, N, route, relu, res_mode, generic, zero_extended)


def generic_route(c):
    return c.generic or f"generic {c.k}x{c.k} kc{32 if c.k == 1 else 8}"


# output map -> (tile, images per tile)
TILE_MAPS = {(3, 13): ("4x16", 2), (3, 70): ("2x64", 1), (5, 50): ("4x32", 1), (9, 27): ("8x16", 1), (2, 130): ("1x128", 1)}
# batch sizes that take a single-source stride-1 1x1 layer past the skinny kernel: N * ceil(HoWo/128) * ceil(Cout/64) >= 256
PAST_SKINNY = {((3, 13), 24): 257, ((3, 13), 72): 129, ((3, 70), 24): 129, ((3, 70), 72): 65, ((5, 50), 24): 129,
               ((5, 50), 72): 65, ((9, 27), 24): 129, ((9, 27), 72): 65, ((2, 130), 24): 87, ((2, 130), 72): 43}


def _tile_cases():
    out = []
    epi = 0
    for k, stride in ((3, (1, 1)), (3, (2, 2)), (3, (2, 1)), (1, (1, 1)), (1, (2, 2))):
        cin = 6 if k == 3 else 40
        for (ho, wo), (tile, ni) in TILE_MAPS.items():
            if tile == "1x128" and (k, stride) != (1, (1, 1)):
                continue
            if stride == (2, 1) and tile != "8x16":
                continue
            hi = ho if stride[0] == 1 else 2 * ho - 1
            wi = wo if stride[1] == 1 else 2 * wo - 1
            for cout in (24, 72):
                N = PAST_SKINNY[(ho, wo), cout] if (k, stride) == (1, (1, 1)) else 3
                route = f"tiled {k}x{k} s{stride[0]}x{stride[1]} {tile} ni{ni} nb{1 if cout <= 32 else 2}"
                out.append(case(f"{route}: {cin}->{cout} @{hi}x{wi} N={N}", [(cin, hi, wi, 1, 1)], cout, k, stride, N, route,
                                relu=epi % 2, res_mode=epi % 3))
                epi += 1
    return out


TILES = _tile_cases()

# each 1x1 stride-1 tile a second way: a small batch that stays off the skinny kernel through two sources or upsampling
TILES_1X1_SMALL_N = [
    case("1x1 two sources @3x13", [(32, 3, 13, 1, 1), (32, 3, 13, 1, 1)], 72, 1, (1, 1), 3, "tiled 1x1 s1x1 4x16 ni2 nb2", 1, 1),
    case("1x1 up(2,2) @1x65 -> 2x130", [(32, 1, 65, 2, 2)], 24, 1, (1, 1), 3, "tiled 1x1 s1x1 1x128 ni1 nb1", 1, 2),
    case("1x1 cat(full, up(3,2)) @3x70", [(32, 3, 70, 1, 1), (32, 1, 35, 3, 2)], 72, 1, (1, 1), 3, "tiled 1x1 s1x1 2x64 ni1 nb2", 0, 1),
    case("1x1 up(1,2) K=40 @5x25 -> 5x50", [(40, 5, 25, 1, 2)], 24, 1, (1, 1), 3, "tiled 1x1 s1x1 4x32 ni1 nb1", 1, 0),
    case("1x1 cat(full, up(3,3)) @9x27", [(32, 9, 27, 1, 1), (64, 3, 9, 3, 3)], 72, 1, (1, 1), 3, "tiled 1x1 s1x1 8x16 ni1 nb2", 1, 2),
]

# three sources with different upsampling, a factor that is no power of two; under tuning bit 0 the generic kernel's last
# chunk of 8 holds the last 4 channels of the last source
SOURCES = [
    case("3x3 cat(8 full, 16 up(2,2), 12 up(3,1)) @6x20", [(8, 6, 20, 1, 1), (16, 3, 10, 2, 2), (12, 2, 20, 3, 1)], 40, 3, (1, 1), 3,
         "tiled 3x3 s1x1 8x16 ni1 nb2", 1, 2),
    case("3x3 s2 cat(8 full, 16 up(2,2), 12 up(3,1)) @6x20", [(8, 6, 20, 1, 1), (16, 3, 10, 2, 2), (12, 2, 20, 3, 1)], 24, 3, (2, 2), 3,
         "tiled 3x3 s2x2 4x16 ni2 nb1", 1, 1),          # a 3x10 output: the two-image tile, odd batch
    case("1x1 cat(32 full, 32 up(2,2), 64 up(3,1)) @6x20", [(32, 6, 20, 1, 1), (32, 3, 10, 2, 2), (64, 2, 20, 3, 1)], 72, 1, (1, 1), 3,
         "tiled 1x1 s1x1 8x16 ni1 nb2", 0, 1),
]

# the recogniser's VGG at N = 2 (tests/test_conv_route_host.py holds the same routes at N = 512)
CRNN = [
    case("crnn conv0 1->64 @32x100", [(1, 32, 100, 1, 1)], 64, 3, (1, 1), 2, "tiled 3x3 s1x1 2x64 ni1 nb2"),
    case("crnn conv1 64->128 @16x50", [(64, 16, 50, 1, 1)], 128, 3, (1, 1), 2, "tiled 3x3 s1x1 4x32 ni1 nb2"),
    case("crnn conv2 128->256 @8x25", [(128, 8, 25, 1, 1)], 256, 3, (1, 1), 2, "tiled 3x3 s1x1 8x16 ni1 nb2"),
    case("crnn conv4 256->512 @4x26", [(256, 4, 26, 1, 1)], 512, 3, (1, 1), 2, "tiled 3x3 s1x1 8x16 ni1 nb2"),
    case("crnn conv5 512->512 @4x26", [(512, 4, 26, 1, 1)], 512, 3, (1, 1), 2, "tiled 3x3 s1x1 8x16 ni1 nb2"),
    case("crnn conv6 512->512 @2x27 s(2,1) zero-extended 2x2", [(512, 2, 27, 1, 1)], 512, 3, (2, 1), 2,
         "tiled 3x3 s2x1 8x16 ni1 nb2", zero_extended=True),
]

GENERIC = [
    case("3x3 Cout=38", [(6, 9, 13, 1, 1)], 38, 3, (1, 1), 3, "generic 3x3 kc8", 1, 2),
    case("1x1 Cout=38 two sources", [(32, 9, 13, 1, 1), (32, 9, 13, 1, 1)], 38, 1, (1, 1), 3, "generic 1x1 kc32", 1, 1),
    case("3x3 stride (1,2)", [(6, 9, 13, 1, 1)], 40, 3, (1, 2), 3, "generic 3x3 kc8", 0, 1),
    case("1x1 stride (2,1) K=40", [(40, 9, 13, 1, 1)], 40, 1, (2, 1), 3, "generic 1x1 kc32", 1, 0),
    # the grid limit from both sides: N * ceil(Cout/64) = 65535 is the last the tiled kernel's grid z holds
    case("3x3 @1x1 Cout=1028 N=3855 (z = 65535)", [(4, 1, 1, 1, 1)], 1028, 3, (1, 1), 3855, "tiled 3x3 s1x1 4x16 ni2 nb2"),
    case("3x3 @1x1 Cout=1028 N=3856 (z would be 65552)", [(4, 1, 1, 1, 1)], 1028, 3, (1, 1), 3856, "generic 3x3 kc8"),
    # concatenated 3x3 sources that are multiples of 4 but not of 8: the generic kernel with 4 channels per chunk
    case("3x3 cat(4,4) Cout=38", [(4, 9, 13, 1, 1), (4, 9, 13, 1, 1)], 38, 3, (1, 1), 3, "generic 3x3 kc4", 1, 1, "generic 3x3 kc4"),
    case("3x3 cat(12, 4 up(3,1), 8) Cout=38", [(12, 9, 13, 1, 1), (4, 3, 13, 3, 1), (8, 9, 13, 1, 1)], 38, 3, (1, 1), 3,
         "generic 3x3 kc4", 1, 2, "generic 3x3 kc4"),
    case("3x3 cat(4,4) Cout=40", [(4, 9, 13, 1, 1), (4, 9, 13, 1, 1)], 40, 3, (1, 1), 3, "tiled 3x3 s1x1 8x16 ni1 nb2", 1, 0,
         "generic 3x3 kc4"),
]

WIDE = [
    # a ragged pixel tile (132 = 128 + 4), a last channel tile of 4, 2 * 2 * 128 = 512 workgroups: the general epilogue
    case("wide K=40 HoWo=132 Cout=132 N=128", [(40, 12, 11, 1, 1)], 132, 1, (1, 1), 128, "wide", 1, 2),
]


def _skinny(K, hw, cout, N, relu, res_mode):
    h, w = {5: (1, 5), 32: (4, 8), 77: (7, 11)}[hw]
    return case(f"skinny K={K} HoWo={hw} Cout={cout}", [(K, h, w, 1, 1)], cout, 1, (1, 1), N,
                f"skinny nw{16 if K >= 256 else 4}", relu, res_mode)


SKINNY = [
    _skinny(1, 5, 8, 3, 1, 0), _skinny(2, 77, 37, 3, 0, 1), _skinny(6, 32, 64, 3, 1, 2), _skinny(127, 77, 37, 2, 1, 1),
    _skinny(128, 32, 64, 3, 0, 2),        # 4 wavefronts, each on the unguarded path (32 k, full 32x32 tiles)
    _skinny(255, 5, 8, 3, 1, 0), _skinny(256, 77, 37, 2, 1, 2),
    _skinny(500, 32, 64, 3, 1, 1),        # 16 wavefronts: 15 on the unguarded path, the last one (20 k) guarded
    _skinny(512, 32, 64, 3, 0, 0),        # 16 wavefronts, all unguarded
    _skinny(512, 77, 37, 1, 1, 2),
]

# both sides of a threshold: the two cases of a pair differ only in N
THRESHOLDS = [
    case("big = 252 < 256: N=63", [(40, 5, 50, 1, 1)], 72, 1, (1, 1), 63, "skinny nw4", 1, 1),
    case("big = 256: N=64", [(40, 5, 50, 1, 1)], 72, 1, (1, 1), 64, "tiled 1x1 s1x1 4x32 ni1 nb2", 1, 1),
    case("wide workgroups = 508 < 512: N=127", [(40, 12, 11, 1, 1)], 132, 1, (1, 1), 127, "tiled 1x1 s1x1 8x16 ni1 nb2", 1, 2),
    # (512 workgroups, N = 128, is WIDE[0])
]

CASES = TILES + TILES_1X1_SMALL_N + SOURCES + CRNN + GENERIC + WIDE + SKINNY + THRESHOLDS
assert len({c.name for c in CASES}) == len(CASES)

# one shape per family for the full product of epilogues
EPILOGUE_SHAPES = {
    "tiled, one accumulator": case("epi nb1", [(6, 5, 50, 1, 1)], 24, 3, (1, 1), 3, "tiled 3x3 s1x1 4x32 ni1 nb1"),
    "tiled, two accumulators, full": case("epi nb2 full", [(6, 3, 70, 1, 1)], 64, 3, (1, 1), 3, "tiled 3x3 s1x1 2x64 ni1 nb2"),
    "tiled, two accumulators, ragged": case("epi nb2 ragged", [(6, 9, 27, 1, 1)], 72, 3, (1, 1), 3, "tiled 3x3 s1x1 8x16 ni1 nb2"),
    "generic": case("epi generic", [(6, 9, 13, 1, 1)], 38, 3, (1, 1), 3, "generic 3x3 kc8"),
    "wide": case("epi wide", [(40, 12, 11, 1, 1)], 132, 1, (1, 1), 128, "wide"),
    "skinny 4": case("epi skinny 4", [(127, 7, 11, 1, 1)], 37, 1, (1, 1), 2, "skinny nw4"),
    "skinny 16": case("epi skinny 16", [(500, 7, 11, 1, 1)], 37, 1, (1, 1), 2, "skinny nw16"),
}
# activation (0 none, 1 ReLU, 2 GELU) x residual (0 none, 1 after, 2 before the activation) x post-affine x bias
EPILOGUES = [(act, res, post, bias) for act in (0, 1, 2) for res in (0, 1, 2) for post in (False, True) for bias in (False, True)]

EXACT_MAX_K = 4608        # 4608 * 8 * 4 + 64 + 64, times 2, plus 64 < 2**24: every partial sum is an exact fp32 integer


# ---- shapes only (the host test) ----------------------------------------------------------------------------------------
def cin_of(c):
    return sum(s[0] for s in c.srcs)


def out_size(c):
    hi, wi = c.srcs[0][1] * c.srcs[0][3], c.srcs[0][2] * c.srcs[0][4]
    p = (c.k - 1) // 2
    return (hi + 2 * p - c.k) // c.stride[0] + 1, (wi + 2 * p - c.k) // c.stride[1] + 1


def route_of(c, N=None):
    """`ops.conv2d_route` of the case's shapes on the meta device: no data, no GPU."""
    N = c.N if N is None else N
    srcs = [(torch.empty((N, ch, h, w), device="meta"), uh, uw) for ch, h, w, uh, uw in c.srcs]
    cw = ops.prep_conv_weight(torch.empty((c.cout, cin_of(c), c.k, c.k), device="meta"), src_channels=[s[0] for s in c.srcs])
    return ops.conv2d_route(srcs, cw, c.stride)


# ---- data -----------------------------------------------------------------------------------------------------------------
def _ints(shape, name, lo, hi):
    """Integers in [lo, hi] as fp32, a function of `name` alone."""
    u = (synth.dyadic(shape, name).astype(np.float64) + 1.0) * 0.5            # [0, 1)
    return torch.from_numpy(np.floor(lo + u * (hi - lo + 1)).clip(lo, hi).astype(np.float32))


def _real(shape, name, scale=1.0):
    return torch.from_numpy(np.ascontiguousarray(synth.dyadic(shape, name, 1, scale)))


def make_inputs(c, exact):
    """dict of fp32 CPU tensors: xs (one per source), w (Cout, Cin, k, k), bias, res, post_scale, post_shift.  `exact`:
    integers (inputs in [-8, 8], weights in [-4, 4], bias and residual in [-64, 64], post-scale in {-2, -1, 1, 2}, an integer
    post-shift); otherwise dyadic reals with weights at 1 / sqrt(fan_in), a non-zero bias and a signed residual."""
    cin, (ho, wo) = cin_of(c), out_size(c)
    tag = c.name + (".int" if exact else ".real")
    wshape = (c.cout, cin, 2, 2) if c.zero_extended else (c.cout, cin, c.k, c.k)
    if exact:
        xs = [_ints((c.N, ch, h, w), f"{tag}.x{i}", -8, 8) for i, (ch, h, w, _, _) in enumerate(c.srcs)]
        w = _ints(wshape, tag + ".w", -4, 4)
        bias, res = _ints((c.cout,), tag + ".b", -64, 64), _ints((c.N, c.cout, ho, wo), tag + ".r", -64, 64)
        ps = torch.tensor([-2.0, -1.0, 1.0, 2.0])[_ints((c.cout,), tag + ".ps", 0, 3).long()]
        pb = _ints((c.cout,), tag + ".pb", -64, 64)
    else:
        xs = [_real((c.N, ch, h, w), f"{tag}.x{i}") for i, (ch, h, w, _, _) in enumerate(c.srcs)]
        fan_in = cin * (4 if c.zero_extended else c.k * c.k)
        w = _real(wshape, tag + ".w", 1.0 / np.sqrt(fan_in))
        bias, res = _real((c.cout,), tag + ".b", 0.5), _real((c.N, c.cout, ho, wo), tag + ".r")
        ps, pb = 1.0 + _real((c.cout,), tag + ".ps", 0.5), _real((c.cout,), tag + ".pb", 0.25)
        ps = torch.where(_real((c.cout,), tag + ".sign") < 0, -ps, ps)
    if c.zero_extended:
        w = F.pad(w, (1, 0, 1, 0))
    return dict(xs=xs, w=w, bias=bias, res=res, post_scale=ps, post_shift=pb)


def conv_sum(c, xs, w):
    """The convolution alone, in the dtype and on the device of its arguments: concatenation, nearest upsampling and
    "same" padding written out.  Adding 0.0 makes a sum that is zero +0.0, as every kernel's chain starts from +0.0."""
    ups = [x if (uh, uw) == (1, 1) else x.repeat_interleave(uh, 2).repeat_interleave(uw, 3)
           for x, (_, _, _, uh, uw) in zip(xs, c.srcs)]
    return F.conv2d(torch.cat(ups, 1), w, None, stride=c.stride, padding=(c.k - 1) // 2) + 0.0


def epilogue(y, act, res_mode, bias=None, res=None, post_scale=None, post_shift=None):
    """The kernels' epilogue in the kernels' order: + bias, + residual (mode 2), activation, + residual (mode 1), affine."""
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if res_mode == 2:
        y = y + res
    if act == 1:
        y = torch.where(y > 0, y, torch.zeros_like(y))
    elif act == 2:
        y = F.gelu(y)
    if res_mode == 1:
        y = y + res
    if post_scale is not None:
        y = y * post_scale.view(1, -1, 1, 1) + post_shift.view(1, -1, 1, 1)
    return y
