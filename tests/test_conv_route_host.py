"""Host side of tests/test_gpu_conv_routes.py (no GPU): `tpspp_conv2d_route` names, for every case of
tests/conv_route_cases.py, the kernel the case was written for; the table reaches every kernel the dispatcher of
tpspp_conv2d_fwd can pick (36 tiled instantiations, the generic 1x1 and 3x3 kernels, the wide kernel, both skinny widths);
sizes the forward refuses are refused by the query with the forward's text; the integer data of the exact comparison stays
inside fp32's exact range."""
import ctypes
import os

import pytest
import torch

import conv_route_cases as RC
import test_gpu_conv as TC
from tps_pp_amd import _lib, ops

# kernel, stride, tile, images per tile: the 18 tiles of tpspp_conv.hip
TILES = [(1, "1x1", "4x16", 2), (1, "1x1", "1x128", 1), (1, "1x1", "2x64", 1), (1, "1x1", "4x32", 1), (1, "1x1", "8x16", 1),
         (1, "2x2", "4x16", 2), (1, "2x2", "2x64", 1), (1, "2x2", "4x32", 1), (1, "2x2", "8x16", 1),
         (3, "1x1", "4x16", 2), (3, "1x1", "2x64", 1), (3, "1x1", "4x32", 1), (3, "1x1", "8x16", 1),
         (3, "2x2", "4x16", 2), (3, "2x2", "2x64", 1), (3, "2x2", "4x32", 1), (3, "2x2", "8x16", 1),
         (3, "2x1", "8x16", 1)]
TILED_ROUTES = {f"tiled {k}x{k} s{s} {t} ni{ni} nb{nb}" for k, s, t, ni in TILES for nb in (1, 2)}
OTHER_ROUTES = {"generic 1x1 kc32", "generic 3x3 kc8", "wide", "skinny nw4", "skinny nw16"}


@pytest.fixture
def tuning():
    """Sets tuning bit 0 on request and clears it afterwards."""
    lib = _lib.lib()
    yield lambda on: lib.tpspp_conv_set_tuning(1 if on else 0)
    lib.tpspp_conv_set_tuning(0)


def test_every_case_takes_the_route_it_names(tuning):
    wrong = {c.name: (RC.route_of(c), c.route) for c in RC.CASES if RC.route_of(c) != c.route}
    assert not wrong, wrong
    wrong = {n: (RC.route_of(c), c.route) for n, c in RC.EPILOGUE_SHAPES.items() if RC.route_of(c) != c.route}
    assert not wrong, wrong
    tuning(True)
    wrong = {c.name: (RC.route_of(c), RC.generic_route(c)) for c in RC.CASES if RC.route_of(c) != RC.generic_route(c)}
    assert not wrong, wrong


def test_the_table_reaches_every_kernel():
    assert len(TILED_ROUTES) == 36
    reached = {c.route for c in RC.CASES}
    assert not TILED_ROUTES - reached, sorted(TILED_ROUTES - reached)
    assert not OTHER_ROUTES - reached, sorted(OTHER_ROUTES - reached)
    assert reached - TILED_ROUTES - OTHER_ROUTES == {"generic 3x3 kc4"}           # the multi-source generic 3x3 kernel
    assert len(reached) == 36 + 2 + 1 + 2 + 1
    assert {c.route for c in RC.EPILOGUE_SHAPES.values()} >= {"wide", "skinny nw4", "skinny nw16", "generic 3x3 kc8"}
    # every 1x1 stride-1 tile twice: past the skinny kernel by batch size, and with a small batch through its sources
    small = {c.route.rsplit(" ", 1)[0] for c in RC.TILES_1X1_SMALL_N}
    assert small == {f"tiled 1x1 s1x1 {t} ni{ni}" for k, s, t, ni in TILES if (k, s) == (1, "1x1")}
    assert all(c.N == 3 for c in RC.TILES_1X1_SMALL_N)


def test_the_older_table_alone_reaches_15_of_the_36_tiled_kernels_and_its_ids_name_the_kernel_they_reach():
    routes = {}
    for name, srcs, cout, k, stride, _, _, N in TC.CASES:
        routes[name] = RC.route_of(RC.case(name, srcs, cout, k, stride, N, ""))
    assert len(set(routes.values()) & TILED_ROUTES) == 15
    for name, r in routes.items():
        for word in ("skinny", "wide", "tiled"):                      # an id that claims a kernel reaches it
            assert not name.startswith(word + " ") or r.startswith(word), (name, r)
        assert "two-image tile" not in name or " ni2 " in r, (name, r)


def test_crnn_layers_take_their_tiles_at_both_batch_sizes():
    want = {"crnn conv0": "tiled 3x3 s1x1 2x64 ni1 nb2", "crnn conv1": "tiled 3x3 s1x1 4x32 ni1 nb2",
            "crnn conv2": "tiled 3x3 s1x1 8x16 ni1 nb2", "crnn conv4": "tiled 3x3 s1x1 8x16 ni1 nb2",
            "crnn conv5": "tiled 3x3 s1x1 8x16 ni1 nb2", "crnn conv6": "tiled 3x3 s2x1 8x16 ni1 nb2"}
    assert len(RC.CRNN) == 6
    for c in RC.CRNN:
        key = " ".join(c.name.split()[:2])
        assert c.N == 2 and c.route == want[key]
        assert RC.route_of(c, 2) == want[key] and RC.route_of(c, 512) == want[key], c.name


def test_thresholds_are_held_from_both_sides():
    by = {c.name: c for c in RC.CASES}
    pairs = [("big = 252 < 256: N=63", "big = 256: N=64"),
             ("wide workgroups = 508 < 512: N=127", "wide K=40 HoWo=132 Cout=132 N=128"),
             ("3x3 @1x1 Cout=1028 N=3855 (z = 65535)", "3x3 @1x1 Cout=1028 N=3856 (z would be 65552)")]
    for a, b in pairs:
        a, b = by[a], by[b]
        assert a[1:5] == b[1:5] and b.N == a.N + 1 and a.route != b.route, (a.name, b.name)
    assert 3855 * ((1028 + 63) // 64) == 65535


def test_exact_data_stays_inside_fp32s_integers():
    for c in list(RC.CASES) + list(RC.EPILOGUE_SHAPES.values()):
        assert RC.cin_of(c) * c.k * c.k <= RC.EXACT_MAX_K, c.name
    assert (RC.EXACT_MAX_K * 8 * 4 + 64 + 64) * 2 + 64 < 2 ** 24
    c = RC.EPILOGUE_SHAPES["skinny 4"]
    d = RC.make_inputs(c, True)
    for key, lim in (("w", 4), ("bias", 64), ("res", 64), ("post_shift", 64)):
        t = d[key]
        assert torch.equal(t, t.round()) and t.abs().max() <= lim and t.min() < 0 < t.max(), key
    assert d["w"].max() == 4 and d["w"].min() == -4 and d["res"].max() == 64 and d["res"].min() == -64
    assert d["xs"][0].abs().max() == 8 and torch.equal(d["xs"][0], d["xs"][0].round())
    assert set(d["post_scale"].tolist()) == {-2.0, -1.0, 1.0, 2.0}
    z = RC.make_inputs(RC.CRNN[5], True)["w"]
    assert z.shape[2:] == (3, 3) and not z[:, :, 0].any() and not z[:, :, :, 0].any() and z[:, :, 1:, 1:].any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def query(srcs, cout, k, stride, N, ho, wo, has_wt=1, has_tiled=1):
    dims = (ctypes.c_int * (5 * len(srcs)))(*[v for s in srcs for v in s])
    rc = _lib.lib().tpspp_conv2d_route(ctypes.cast(dims, ctypes.c_void_p), len(srcs), has_wt, has_tiled, N, cout, k, k,
                                       stride[0], stride[1], ho, wo)
    return rc, _lib.lib().tpspp_last_error().decode()


REFUSALS = [
    ([(6, 9, 13, 1, 1), (4, 9, 13, 1, 1)], 40, 3, (1, 1), 2, 9, 13, 1, 1,
     "tpspp_conv2d_fwd: concatenated sources need channel counts that are multiples of 4"),
    ([(32, 9, 13, 1, 1), (16, 9, 13, 1, 1)], 40, 1, (1, 1), 2, 9, 13, 1, 1,
     "tpspp_conv2d_fwd: concatenated sources need channel counts that are multiples of 32"),
    ([(6, 9, 13, 1, 1)], 38, 3, (1, 1), 2, 9, 13, 0, 1, "tpspp_conv2d_fwd: shape needs the generic kernel but weight_t is NULL"),
    ([(6, 9, 13, 1, 1)], 40, 3, (1, 1), 2, 9, 13, 0, 0, "tpspp_conv2d_fwd: null pointer"),
    ([(6, 9, 13, 1, 1)], 40, 3, (1, 1), 65536, 9, 13, 1, 1, "tpspp_conv2d_fwd: grid too large"),
    ([(6, 9, 13, 1, 1)], 40, 5, (1, 1), 2, 9, 13, 1, 1, "tpspp_conv2d_fwd: kernel must be 1x1 or 3x3"),
    ([(6, 9, 13, 1, 1)], 40, 3, (1, 1), 2, 9, 12, 1, 1,
     "tpspp_conv2d_fwd: output size does not match input size / stride ('same' padding)"),
    ([(8, 9, 13, 1, 1), (8, 3, 13, 2, 1)], 40, 3, (1, 1), 2, 9, 13, 1, 1, "tpspp_conv2d_fwd: sources disagree on the logical size"),
    ([(6, 9, 13, 1, 1)] * 4, 40, 3, (1, 1), 2, 9, 13, 1, 1, "tpspp_conv2d_fwd: 1..3 sources"),
]


@pytest.mark.parametrize("args", REFUSALS, ids=[r[-1].split(": ", 1)[1][:40] for r in REFUSALS])
def test_the_query_refuses_what_the_forward_refuses_in_the_forwards_words(args):
    *call, text = args
    rc, msg = query(*call)
    assert rc == -22 and msg == text, (rc, msg)


def test_the_wrappers_refuse_a_source_that_is_no_multiple_of_the_chunk():
    w = torch.empty((40, 10, 3, 3), device="meta")
    cw = ops.prep_conv_weight(w, src_channels=[6, 4])
    assert cw.tiled is None                    # no chunked layout exists for such sources ...
    srcs = [torch.empty((2, 6, 9, 13), device="meta"), torch.empty((2, 4, 9, 13), device="meta")]
    with pytest.raises(_lib.TpsppError, match="concatenated sources need channel counts that are multiples of 4"):
        ops.conv2d_route(srcs, cw)             # ... and the library refuses the call whichever weights it is given
    for chans in ([4, 4], [12, 4, 8]):         # multiples of 4 are the rule: both layouts are built
        cw = ops.prep_conv_weight(torch.empty((40, sum(chans), 3, 3), device="meta"), src_channels=chans)
        assert cw.tiled is not None and cw.tiled.shape == (sum(chans) // 4, 3, 3, 4, 40)


def test_header_argument_check_and_kernels_state_one_rule():
    lib = _lib.lib()
    assert (lib.tpspp_conv_chunk_channels(1), lib.tpspp_conv_chunk_channels(3)) == (32, 4)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = " ".join(open(os.path.join(root, "include", "tpspp.h")).read().replace(" * ", " ").split())
    assert "every C_i must be a multiple of tpspp_conv_chunk_channels(K), 32 (1x1) / 4 (3x3)" in header
    assert "8 (3x3)" not in header


def test_the_generic_3x3_kernel_never_takes_a_chunk_across_two_sources(tuning):
    """Walks the staging addresses of conv_igemm_f32_kernel<3, 3, KC> (chunk c0 reads channels c0 - cbase .. + KC - 1 of the
    source c0 lies in, guarded only by c0 + ci < Cin) for the chunk size the route names: none lies outside its source."""
    tuning(True)
    for chans in ([4, 4], [12, 4], [12, 4, 8], [8, 12], [8, 16, 12], [16, 8], [4, 8, 8], [8, 4, 4], [24, 4, 12]):
        c = RC.case("walk", [(ch, 9, 13, 1, 1) for ch in chans], 40, 3, (1, 1), 2, "")
        kc = int(RC.route_of(c).rsplit("kc", 1)[1])
        assert kc == (8 if all(ch % 8 == 0 for ch in chans[:-1]) else 4)
        outside = walk_generic_chunks(chans, kc)
        assert not outside, (chans, kc, outside)
    assert walk_generic_chunks([4, 4], 8) == [(0, 0, 4), (0, 0, 5), (0, 0, 6), (0, 0, 7)]       # what 8 per chunk would read


def walk_generic_chunks(chans, kc):
    """(chunk's first channel, source, channel inside the source) of every staged channel that its source does not hold."""
    cin, out = sum(chans), []
    cbase, s = 0, 0
    for c0 in range(0, cin, kc):
        while c0 >= cbase + chans[s]:
            cbase += chans[s]
            s += 1
        for ci in range(kc):
            if c0 + ci < cin and c0 - cbase + ci >= chans[s]:
                out.append((c0, s, c0 - cbase + ci))
    return out
