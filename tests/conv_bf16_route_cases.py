"""The case table of tests/test_conv_bf16_route_host.py (CPU) and tests/test_gpu_conv_bf16_routes.py (-m gpu): one case per
route code `tpspp_conv2d_bf16_route` can return (a few routes a second way), each at the smallest shape that still takes the
route, with the route `ops.conv2d_bf16_route` must name for it, and the builders of inputs and float64 references.  Nothing
here needs a GPU.

A case's `route` is the kernel with the tuning bits clear.  A specialised case (wide3, wide1, stem, persist, blk1) also records
`bits`, the value of `tpspp_conv_set_tuning` that switches its family off (4: the wide-tile kernels and the stem, 2: the
persistent and the blocked 1x1 kernel), and `fallback`, the tiled route it takes then; a tiled case has bits = 0.

Sources are (C, H, W, uh, uw, layout); layouts: "bf16" / "f32" NCHW, "blk" (`ops.Blocked`), "blk32" (`ops.Blocked32`) and
"bf16off", a bf16 NCHW tensor that starts one element into its allocation (2 bytes off 16-byte alignment: what a sliced view of a
larger buffer is), which the tiled kernel's wide staging must decline.  The residual and the output carry the same names.

Ragged edges: no tiled map is a whole number of tiles on either axis (1x130, 3x70, 5x40, 5x20, 9x13, 6x13, 3x13, 2x13; with
wide staging, whose rows are whole 16-byte pieces, 1x136, 3x72, 5x40, 5x24, 9x8, 6x16, 3x8, 2x16); batches are odd (3, or 5 on
the four-image tiles); Cin = 24 (3x3: a last chunk of 8 of 16 channels) and 40 (1x1: 8 of 32); Cout = 24 and 72 (a ragged channel
tile) beside 32 and 64."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from conv_route_cases import _ints, _real, epilogue           # noqa: F401  (epilogue: re-exported for the tests)
from tps_pp_amd import ops

Case = namedtuple("Case", "name srcs cout k stride N route bits fallback relu res_mode res out x3")


def case(name, srcs, cout, k, stride, N, route, bits=0, fallback=None, relu=1, res_mode=0, res=None, out="bf16", x3=False):
    assert (res_mode == 0) == (res is None) and (bits == 0) == (fallback is None), name
    return Case(name, srcs, cout, k, stride, N, route, bits, fallback, relu, res_mode, res, out, x3)


def _label(srcs):
    return "cat(" + ", ".join(f"{c} {lay}" + (f" up({uh},{uw})" if (uh, uw) != (1, 1) else "") for c, _, _, uh, uw, lay in srcs) + ")"


# ---- wide3 / wide1: both tiles x the four epilogues, res_mode 1 and 2, N = 5 on the four-image tile --------------------------------
def _wide_cases(k):
    fam, cin = ("wide3", 64) if k == 3 else ("wide1", 256)
    out = []
    for (h, w, ni, N, fb) in ((8, 32, 1, 3, "4x32 ni1 nf1" if k == 3 else "8x32 ni1 nf2"), (4, 16, 4, 5, "4x16 ni2 nf1")):
        for epi in range(4):
            res_mode = 0 if epi % 2 == 0 else (1 + (epi // 2 + ni) % 2)       # 8x32: epi1 -> 2, epi3 -> 1; 4x16: epi1 -> 1, epi3 -> 2
            out.append(case(f"{fam} {cin}->128 @{h}x{w} epi{epi} N={N}", [(cin, h, w, 1, 1, "blk")], 128, k, (1, 1), N,
                            f"{fam} {k}x{k} s1x1 {h}x{w} ni{ni} nf4 epi{epi}", 4, f"tiled {k}x{k} s1x1 {fb} wide0 nb2",
                            relu=epi % 2 if k == 3 else 1 - epi % 2, res_mode=res_mode, res="blk" if res_mode else None,
                            out="f32" if epi >= 2 else "blk"))
    return out


WIDE3, WIDE1 = _wide_cases(3), _wide_cases(1)
# the largest K an exact case may have (512 * 9 = 4608: the backbone's last stage), on the four-image tile with a ragged group
WIDE3.append(case("wide3 512->128 @4x16 epi1 N=5 (K = 4608)", [(512, 4, 16, 1, 1, "blk")], 128, 3, (1, 1), 5,
                  "wide3 3x3 s1x1 4x16 ni4 nf4 epi1", 4, "tiled 3x3 s1x1 4x16 ni2 nf1 wide0 nb2", 1, 2, "blk", "blk"))

# ---- stem: C = 1 and 3, both output forms -------------------------------------------------------------------------------------------
STEM = [case(f"stem {c}->32 @4x128 {out}", [(c, 4, 128, 1, 1, "f32")], 32, 3, (1, 1), 3, f"stem 3x3 s1x1 4x128 ni1 nf4 blocked{int(out == 'blk')}",
             4, "tiled 3x3 s1x1 2x128 ni1 nf2 wide0 nb2", relu=c % 2, out=out) for c in (1, 3) for out in ("bf16", "blk")]


# ---- persist: four tiles x {resident weight with 2 chunks per slot, resident with 1, streamed} x three epilogues ----------------
def _persist_cases():
    out = []
    i = 0
    # (stride, tile, NF, sources at the tile's one- or two-tile map, fallback tile)
    tiles = (((1, 1), "4x64", 2, (8, 64), "4x64 ni1 nf2"), ((1, 1), "8x32", 2, (8, 32), "4x32 ni1 nf1"),
             ((2, 2), "2x64", 1, (4, 128), "2x64 ni1 nf1"), ((2, 2), "4x32", 1, (8, 64), "4x32 ni1 nf1"))
    for stride, tile, nf, (hi, wi), fb in tiles:
        # Cin 32: two chunks (an even count: two per ring slot where such a ring fits, stride 1); 48: three (odd: one per slot);
        # three sources of 64: the streamed weight
        weights = ((32, 1, 2), (48, 1, 1), (192, 0, 1)) if stride == (1, 1) else ((32, 1, 1), (192, 0, 1))
        for cin, wres, cpb in weights:
            for epi in range(3):
                srcs = [(64, hi, wi, 1, 1, "blk")] * 3 if cin == 192 else [(cin, hi, wi, 1, 1, "blk")]
                if tile == "8x32" and cin == 32:                       # an upsampled source (the MSFA's decoder)
                    srcs = [(32, hi // 2, wi // 2, 2, 2, "blk")]
                cout = 32 if i % 2 else 64
                s = f"s{stride[0]}x{stride[1]}"
                out.append(case(f"persist {s} {tile} {_label(srcs)}->{cout} epi{epi}", srcs, cout, 3, stride, 3,
                                f"persist 3x3 {s} {tile} ni1 nf{nf} wres{wres} epi{epi} cpb{cpb}", 2, f"tiled 3x3 {s} {fb} wide0 nb2",
                                relu=(i // 2) % 2, res_mode=(1 + i % 2) if epi == 1 else 0, res="blk" if epi == 1 else None,
                                out="f32" if epi == 2 else "blk"))
                i += 1
    return out


PERSIST = _persist_cases()

# ---- blk1: every (Cin, Cout) instantiation on a 4x8 map (one 32-pixel row of a tile per image) ------------------------------------
# NW = 8 wavefronts (256-pixel tiles: N = 8) unless accumulators + operands pass 160 registers (256 input channels: NW = 4, N = 4)
_BLK1 = ((64, 64, 2, 4, 1, 8), (64, 128, 4, 4, 1, 8), (128, 128, 4, 8, 1, 8), (128, 256, 8, 8, 1, 8), (256, 256, 8, 16, 1, 4),
         (32, 32, 1, 2, 1, 8), (32, 64, 2, 2, 1, 8), (256, 512, 8, 16, 2, 4))
_BLK1_FB = "tiled 1x1 s1x1 4x16 ni2 nf1 wide0 nb2"
BLK1 = [case(f"blk1 {ci}->{co} @4x8 N={nw}", [(ci, 4, 8, 1, 1, "blk")], co, 1, (1, 1), nw, f"blk1 1x1 s1x1 nt{nt} nks{nks} sl{sl} nw{nw}",
             2, _BLK1_FB, relu=j % 2, out="blk") for j, (ci, co, nt, nks, sl, nw) in enumerate(_BLK1)]
BLK1 += [
    case("blk1 128->256 @4x16 N=4: a tile spans four images", [(128, 4, 16, 1, 1, "blk")], 256, 1, (1, 1), 4,
         "blk1 1x1 s1x1 nt8 nks8 sl1 nw8", 2, _BLK1_FB, out="blk"),
    # just off the whole-tile condition: 7 * 32 pixels are no multiple of 256
    case("blk1's 64->64 @4x8 with N=7: tiled", [(64, 4, 8, 1, 1, "blk")], 64, 1, (1, 1), 7, _BLK1_FB, out="blk"),
]

# ---- tiled and tiled-x3 ---------------------------------------------------------------------------------------------------------------
FORMS = ((3, (1, 1)), (3, (2, 2)), (3, (2, 1)), (1, (1, 1)), (1, (2, 2)))
# output map -> tile, images per tile, fragments per wavefront.  B: 1x1 kernels and the plain 3x3 at stride 1; A: 128-pixel tiles
# (3x3 at stride 2 and the three-term split's 3x3)
B_MAPS = {(1, 130): "1x256 ni1 nf2", (3, 70): "2x128 ni1 nf2", (5, 40): "4x64 ni1 nf2", (5, 20): {3: "4x32 ni1 nf1", 1: "8x32 ni1 nf2"},
          (9, 13): "16x16 ni1 nf2", (6, 13): "8x16 ni2 nf2", (3, 13): "4x16 ni2 nf1", (2, 13): "2x16 ni4 nf1"}
A_MAPS = {(2, 70): "1x128 ni1 nf1", (3, 40): "2x64 ni1 nf1", (5, 20): "4x32 ni1 nf1", (6, 13): "8x16 ni1 nf1", (3, 13): "4x16 ni2 nf1",
          (2, 13): "2x16 ni4 nf1"}
# the plain 3x3 at stride 1 with wide staging: rows of whole 16-byte pieces
WIDE_MAPS = {(1, 136): "1x256 ni1 nf2", (3, 72): "2x128 ni1 nf2", (5, 40): "4x64 ni1 nf2", (5, 24): "4x32 ni1 nf1", (9, 8): "16x16 ni1 nf2",
             (6, 16): "8x16 ni2 nf2", (3, 8): "4x16 ni2 nf1", (2, 16): "2x16 ni4 nf1"}


def _sources(i, k, hi, wi, x3):
    """Sources for the i-th generated case: a ragged last chunk, two sources (the second upsampled along W where W is even),
    one source of whole chunks, three sources (the third upsampled by 4 where W allows); layouts rotate."""
    lays = ("f32", "blk32", "bf16") if x3 else ("bf16", "f32", "blk")
    L = lambda j: lays[(i + j) % 3]      # noqa: E731
    c = 16 if k == 3 else 32
    pick = ([(24 if k == 3 else 40, 1, 1, L(0))], [(c, 1, 1, L(0)), (2 * c, 1, 2, L(1))], [(2 * c, 1, 1, L(2))],
            [(c, 1, 1, L(1)), (c, 1, 1, L(0)), (c, 1, 4, L(2))])[i % 4]
    return [(ch, hi // uh, wi // (uw if wi % uw == 0 else 1), uh, uw if wi % uw == 0 else 1, lay) for ch, uh, uw, lay in pick]


def _tiled_cases(x3):
    fam = "tiled-x3" if x3 else "tiled"
    out = []
    i = 0
    for k, stride in FORMS:
        maps = A_MAPS if k == 3 and (stride[0] == 2 or x3) else B_MAPS
        for (ho, wo), tile in maps.items():
            tile = tile[k] if isinstance(tile, dict) else tile
            ni = int(tile.split(" ni")[1][0])
            hi, wi = (ho if stride[0] == 1 else 2 * ho - 1), (wo if stride[1] == 1 else 2 * wo - 1)
            for nb in ((1, 2) if x3 else (2,)):
                srcs = _sources(i, k, hi, wi, x3)
                if not x3 and (k, stride) == (3, (1, 1)) and wi % 8 == 0 and all(s[3:] == (1, 1, "bf16") for s in srcs):
                    srcs = [s[:5] + ("bf16off",) for s in srcs]          # would be wide staging but for the alignment
                cout = (24, 32)[i % 2] if nb == 1 else (72, 64)[i % 2]
                lay = (("f32", "blk32", "f32", "bf16") if x3 else ("bf16", "f32", "blk"))
                rl = ("f32", "blk32", "bf16") if x3 else ("bf16", "f32", "blk")
                res_mode = i % 3
                s = f"s{stride[0]}x{stride[1]}"
                out.append(case(f"{fam} {k}x{k} {s} {_label(srcs)}->{cout} @{hi}x{wi} nb{nb}", srcs, cout, k, stride, {1: 3, 2: 3, 4: 5}[ni],
                                f"{fam} {k}x{k} {s} {tile} wide0 nb{nb}", relu=i % 2, res_mode=res_mode,
                                res=rl[(i // 3) % 3] if res_mode else None, out=lay[i % len(lay)], x3=x3))
                i += 1
    return out


TILED, TILED_X3 = _tiled_cases(False), _tiled_cases(True)


def _wide_staging_cases():
    out = []
    for i, ((h, w), tile) in enumerate(WIDE_MAPS.items()):
        ni = int(tile.split(" ni")[1][0])
        srcs = [(24, h, w, 1, 1, "bf16")] if i % 2 == 0 else [(16, h, w, 1, 1, "bf16"), (32, h, w, 1, 1, "bf16")]
        cout = (72, 64)[i % 2]            # 64: the wide epilogue (whole channel tile, bf16 NCHW rows of 16-byte pieces) where the tile fits
        out.append(case(f"tiled 3x3 s1x1 wide staging {_label(srcs)}->{cout} @{h}x{w}", srcs, cout, 3, (1, 1), {1: 3, 2: 3, 4: 5}[ni],
                        f"tiled 3x3 s1x1 {tile} wide1 nb2", relu=i % 2, res_mode=i % 3, res=("bf16", "f32")[i % 2] if i % 3 else None,
                        out=("bf16", "f32")[(i // 2) % 2]))
    return out


TILED_WIDE = _wide_staging_cases()
# wide staging declined for one reason each, on maps whose rows ARE whole 16-byte pieces
TILED_NOT_WIDE = [
    case("3x3 fp32 source @5x24: no wide staging", [(32, 5, 24, 1, 1, "f32")], 64, 3, (1, 1), 3, "tiled 3x3 s1x1 4x32 ni1 nf1 wide0 nb2"),
    case("3x3 bf16 source one element off alignment @3x72", [(32, 3, 72, 1, 1, "bf16off")], 64, 3, (1, 1), 3,
         "tiled 3x3 s1x1 2x128 ni1 nf2 wide0 nb2", res_mode=2, res="bf16"),
    case("3x3 second source off alignment @6x16", [(16, 6, 16, 1, 1, "bf16"), (16, 6, 16, 1, 1, "bf16off")], 72, 3, (1, 1), 3,
         "tiled 3x3 s1x1 8x16 ni2 nf2 wide0 nb2", out="f32"),
    case("3x3 bf16 source upsampled from 4x16 to 8x32",[(32, 4, 16, 2, 2, "bf16")], 64, 3, (1, 1), 3,
         "tiled 3x3 s1x1 4x32 ni1 nf1 wide0 nb2", res_mode=1, res="f32"),
    case("3x3 blocked source @2x16", [(32, 2, 16, 1, 1, "blk")], 40, 3, (1, 1), 5, "tiled 3x3 s1x1 2x16 ni4 nf1 wide0 nb2", out="blk"),
    # the stem's shape with four channels: no specialised kernel, the tiled one on an fp32 image
    case("3x3 4->32 @4x128 fp32 image", [(4, 4, 128, 1, 1, "f32")], 32, 3, (1, 1), 3, "tiled 3x3 s1x1 2x128 ni1 nf2 wide0 nb2"),
]

SPECIALISED = WIDE3 + WIDE1 + STEM + PERSIST + [c for c in BLK1 if c.bits]
CASES = SPECIALISED + [c for c in BLK1 if not c.bits] + TILED + TILED_WIDE + TILED_NOT_WIDE + TILED_X3
assert len({c.name for c in CASES}) == len(CASES)

# one tiled case per (kernel, stride) form in plain bf16 and one in the three-term split for the full product of epilogues
EPILOGUE_SHAPES = {
    "3x3 s1x1": case("epi 3x3 s1x1", [(24, 5, 40, 1, 1, "bf16")], 72, 3, (1, 1), 3, "tiled 3x3 s1x1 4x64 ni1 nf2 wide1 nb2", out="f32"),
    "3x3 s2x2": case("epi 3x3 s2x2", [(24, 9, 39, 1, 1, "f32")], 64, 3, (2, 2), 3, "tiled 3x3 s2x2 4x32 ni1 nf1 wide0 nb2", out="f32"),
    "3x3 s2x1": case("epi 3x3 s2x1", [(24, 5, 13, 1, 1, "bf16")], 40, 3, (2, 1), 3, "tiled 3x3 s2x1 4x16 ni2 nf1 wide0 nb2", out="f32"),
    "1x1 s1x1": case("epi 1x1 s1x1", [(40, 3, 70, 1, 1, "bf16")], 72, 1, (1, 1), 3, "tiled 1x1 s1x1 2x128 ni1 nf2 wide0 nb2", out="f32"),
    "1x1 s2x2": case("epi 1x1 s2x2", [(64, 11, 25, 1, 1, "blk")], 64, 1, (2, 2), 3, "tiled 1x1 s2x2 8x16 ni2 nf2 wide0 nb2", out="f32"),
    "x3 3x3 s1x1": case("epi x3 3x3 s1x1", [(24, 5, 20, 1, 1, "f32")], 24, 3, (1, 1), 3, "tiled-x3 3x3 s1x1 4x32 ni1 nf1 wide0 nb1",
                        out="f32", x3=True),
}
# activation (0 none, 1 ReLU, 2 GELU) x residual (0 none, 1 after, 2 before the activation) x post-affine x bias
EPILOGUES = [(act, res, post, bias) for act in (0, 1, 2) for res in (0, 1, 2) for post in (False, True) for bias in (False, True)]

EXACT_MAX_K = 4608        # 4608 * 8 * 4 + 64 + 64, times 2, plus 64 < 2**24: every partial sum is an exact fp32 integer
assert all(sum(s[0] for s in c.srcs) * c.k * c.k <= EXACT_MAX_K for c in CASES)


def plain_route(c):
    """The case's route when it runs without its residual: the wide and the persistent kernels name their epilogue."""
    fam = c.route.split()[0]
    if c.res_mode and fam in ("wide3", "wide1"):
        return c.route.replace(" epi1", " epi0").replace(" epi3", " epi2")
    if c.res_mode and fam == "persist":
        return c.route.replace(" epi1 ", " epi0 ")
    return c.route


def runs_of(c):
    """(tuning bits, residual mode, post-affine, route) of a case's exact launches: the plain epilogue and the general one the
    route accepts (its residual mode; the tiled routes also the post-affine), a specialised case on its own route and on its
    tiled fallback."""
    if not c.bits:
        return [(0, 0, False, c.route), (0, c.res_mode, True, c.route)]
    modes = [0, c.res_mode] if c.res_mode else [0]
    return [(bits, m, False, c.fallback if bits else (c.route if m else plain_route(c))) for m in modes for bits in (0, c.bits)]


# ---- shapes only (the host test) ---------------------------------------------------------------------------------------------------------
def cin_of(c):
    return sum(s[0] for s in c.srcs)


def out_size(c):
    hi, wi = c.srcs[0][1] * c.srcs[0][3], c.srcs[0][2] * c.srcs[0][4]
    p = (c.k - 1) // 2
    return (hi + 2 * p - c.k) // c.stride[0] + 1, (wi + 2 * p - c.k) // c.stride[1] + 1


_DT = {"bf16": torch.bfloat16, "bf16off": torch.bfloat16, "f32": torch.float32}


def as_layout(x, lay, place):
    """The fp32 NCHW tensor `x` (or, `x` a shape, no data) in the layout `lay`; `place(t)` puts a contiguous tensor where the
    test wants it (a guarded device input; the meta device)."""
    blank = not isinstance(x, torch.Tensor)
    if lay in ("blk", "blk32"):
        cls, dt = (ops.Blocked, torch.bfloat16) if lay == "blk" else (ops.Blocked32, torch.float32)
        if blank:
            n, ch, h, w = x
            return cls(place(torch.empty((n, ch // 8, h, w, 8), dtype=dt, device="meta")))
        return cls(place(cls.from_nchw(x).t))
    shape = tuple(x) if blank else tuple(x.shape)
    numel = int(np.prod(shape))
    if lay == "bf16off":
        # one element into a larger buffer; the slack on both sides holds NaN like the bands around it
        flat = torch.empty((numel + 8,), dtype=torch.bfloat16, device="meta") if blank else torch.full((numel + 8,), float("nan"), dtype=torch.bfloat16)
        if not blank:
            flat[1:1 + numel] = x.reshape(-1).to(torch.bfloat16)
        return place(flat)[1:1 + numel].view(shape)
    return place(torch.empty(shape, dtype=_DT[lay], device="meta") if blank else x.to(_DT[lay]))


def weights_of(c, w=None, bias=None, post_scale=None, post_shift=None, place=lambda t: t):
    """`ops.ConvWeightBf16` of the case: from `w` (Cout, Cin, k, k) on any device, or, without one, on the meta device."""
    if w is None:
        w = torch.empty((c.cout, cin_of(c), c.k, c.k), device="meta")
    cw = ops.prep_conv_weight_bf16(w, x3=c.x3)
    return ops.ConvWeightBf16(place(cw.arranged), bias, c.k, cw.cin, cw.cout, post_scale, post_shift, c.x3)


def route_of(c, N=None, res_mode=None, bits=0, relu=None, post=False):
    """`ops.conv2d_bf16_route` of the case's shapes on the meta device under `tpspp_conv_set_tuning(bits)`: no data, no GPU."""
    from tps_pp_amd import _lib
    N = c.N if N is None else N
    res_mode = c.res_mode if res_mode is None else res_mode
    meta = lambda t: t.to("meta")      # noqa: E731
    srcs = [(as_layout((N, ch, h, w), lay, meta), uh, uw) for ch, h, w, uh, uw, lay in c.srcs]
    one = torch.empty((c.cout,), device="meta")
    cw = weights_of(c, None, one, one if post else None, one if post else None)
    res = as_layout((N, c.cout) + out_size(c), c.res, meta) if res_mode else None
    _lib.lib().tpspp_conv_set_tuning(bits)
    try:
        return ops.conv2d_bf16_route(srcs, cw, c.stride, c.relu if relu is None else relu, res, res_mode,
                                     torch.float32 if c.out in ("f32", "blk32") else torch.bfloat16, c.out in ("blk", "blk32"))
    finally:
        _lib.lib().tpspp_conv_set_tuning(0)


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def rb(x):
    """Round to bf16 (to nearest even), keep the dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def make_inputs(c, exact):
    """dict of fp32 CPU tensors: xs (one per source), w (Cout, Cin, k, k), bias, res, post_scale, post_shift.  `exact`:
    integers (inputs in [-8, 8], weights in [-4, 4], bias and residual in [-64, 64], post-scale in {-2, -1, 1, 2}, an integer
    post-shift): every one a bf16 number, so that no layout and no split rounds anything.  Otherwise dyadic reals with weights at
    1 / sqrt(fan_in), a non-zero bias and a signed residual; what a case keeps in bf16 (sources, residual) is rounded here, so
    that the tensors ARE what the kernel reads."""
    cin, (ho, wo) = cin_of(c), out_size(c)
    tag = c.name + (".int" if exact else ".real")
    if exact:
        xs = [_ints((c.N, ch, h, w), f"{tag}.x{i}", -8, 8) for i, (ch, h, w, *_) in enumerate(c.srcs)]
        w = _ints((c.cout, cin, c.k, c.k), tag + ".w", -4, 4)
        bias, res = _ints((c.cout,), tag + ".b", -64, 64), _ints((c.N, c.cout, ho, wo), tag + ".r", -64, 64)
        ps = torch.tensor([-2.0, -1.0, 1.0, 2.0])[_ints((c.cout,), tag + ".ps", 0, 3).long()]
        pb = _ints((c.cout,), tag + ".pb", -64, 64)
    else:
        xs = [_real((c.N, ch, h, w), f"{tag}.x{i}") for i, (ch, h, w, *_) in enumerate(c.srcs)]
        xs = [rb(x) if s[5] in ("bf16", "bf16off", "blk") else x for x, s in zip(xs, c.srcs)]
        w = _real((c.cout, cin, c.k, c.k), tag + ".w", 1.0 / np.sqrt(cin * c.k * c.k))
        bias, res = _real((c.cout,), tag + ".b", 0.5), _real((c.N, c.cout, ho, wo), tag + ".r")
        if c.res in ("bf16", "blk"):
            res = rb(res)
        ps, pb = 1.0 + _real((c.cout,), tag + ".ps", 0.5), _real((c.cout,), tag + ".pb", 0.25)
        ps = torch.where(_real((c.cout,), tag + ".sign") < 0, -ps, ps)
    return dict(xs=xs, w=w, bias=bias, res=res, post_scale=ps, post_shift=pb)


def _conv(c, xs, w):
    ups = [x if (uh, uw) == (1, 1) else x.repeat_interleave(uh, 2).repeat_interleave(uw, 3)
           for x, (_, _, _, uh, uw, _) in zip(xs, c.srcs)]
    return F.conv2d(torch.cat(ups, 1), w, None, stride=c.stride, padding=(c.k - 1) // 2)


def conv_sum(c, xs, w, dtype=torch.float64, device="cpu"):
    """The convolution alone as the route computes it, carried out in `dtype` on `device`: concatenation, nearest upsampling and
    "same" padding written out.  Plain bf16: both operands rounded to bf16.  The three-term split: hi = bf16(v),
    lo = bf16(v - hi) (`ops._hi_lo`), a product is hi * hi + hi * lo + lo * hi.  Adding 0.0 makes a zero sum +0.0."""
    to = lambda t: t.to(device=device, dtype=dtype)      # noqa: E731
    if not c.x3:
        return _conv(c, [to(rb(x)) for x in xs], to(rb(w))) + 0.0
    wh, wl = (to(t.float()) for t in ops._hi_lo(w))
    xh, xl = zip(*[[to(t.float()) for t in ops._hi_lo(x)] for x in xs])
    return _conv(c, xh, wh) + _conv(c, xl, wh) + _conv(c, xh, wl) + 0.0
