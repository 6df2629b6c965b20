"""Host side of tests/test_gpu_conv_bf16_routes.py (no GPU): `tpspp_conv2d_bf16_route` names, for every case of
tests/conv_bf16_route_cases.py, the kernel the case was written for, with the tuning bits clear and set; a sweep of the query
over shapes, layouts, alignments and batch sizes returns exactly the routes the table holds (a route added later without a case
fails here); the query refuses what the forward refuses, in the forward's words; and it works with no device visible."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest
import torch

import conv_bf16_route_cases as RC
from tps_pp_amd import _lib, ops

ALL = list(RC.CASES) + list(RC.EPILOGUE_SHAPES.values())


@pytest.mark.parametrize("c", ALL, ids=[c.name for c in ALL])
def test_every_case_takes_its_route(c):
    assert RC.route_of(c) == c.route
    for bits, res_mode, post, route in RC.runs_of(c):              # every launch of the exact test, as it asserts it
        assert RC.route_of(c, res_mode=res_mode, bits=bits, post=post) == route, (bits, res_mode, post)
    assert c.route.split()[0] in ("tiled", "tiled-x3") or c.bits, "a specialised case records the bit that disables it"
    if c.bits:
        assert RC.route_of(c, bits=c.bits) == c.fallback and c.fallback.startswith("tiled ")
        assert RC.route_of(c, bits=6) == c.fallback
        # what every specialised kernel declines goes to the tiled kernel as well: GELU, the post-affine
        assert RC.route_of(c, relu=2) == c.fallback and RC.route_of(c, post=True) == c.fallback
    else:
        assert RC.route_of(c, bits=6) == c.route                   # the bits move no tiled case
        assert RC.route_of(c, relu=2) == c.route and RC.route_of(c, post=True) == c.route
    if not c.route.startswith("blk1") and "blk1's" not in c.name:
        assert RC.route_of(c, N=0) == RC.route_of(c, N=8) == c.route  # only blk1's whole-tile rule reads N at these sizes


def test_an_empty_batch_is_judged_as_eight_images():
    by = {c.name: c for c in RC.CASES}
    for name in ("blk1 64->64 @4x8 N=8", "blk1's 64->64 @4x8 with N=7: tiled", "blk1 256->256 @4x8 N=4"):
        c = by[name]
        assert RC.route_of(c, N=0) == RC.route_of(c, N=8) and RC.route_of(c, N=8).startswith("blk1"), name
    c = by["blk1 64->64 @4x8 N=8"]
    assert [RC.route_of(c, N=n).split()[0] for n in (7, 8, 9, 16)] == ["tiled", "blk1", "tiled", "blk1"]
    c = by["blk1 256->256 @4x8 N=4"]                                   # four wavefronts: 128-pixel tiles
    assert [RC.route_of(c, N=n).split()[0] for n in (3, 4, 6, 8)] == ["tiled", "blk1", "tiled", "blk1"]


def test_the_table_holds_what_the_issue_lists():
    routes = [c.route for c in RC.CASES]
    fam = lambda f: [r for r in routes if r.split()[0] == f]      # noqa: E731
    for f in ("wide3", "wide1"):
        assert {(r.split()[3], r.split()[-1]) for r in fam(f)} == {(t, f"epi{e}") for t in ("8x32", "4x16") for e in range(4)}
        modes = {(c.route.split()[3], c.res_mode) for c in RC.CASES if c.route.startswith(f)}
        assert modes >= {(t, m) for t in ("8x32", "4x16") for m in (0, 1, 2)} - {("8x32", 0), ("4x16", 0)} | {("8x32", 0)}
        assert any(c.N % 4 for c in RC.CASES if c.route.startswith(f) and " 4x16 " in c.route)
    assert {(c.srcs[0][0], c.out) for c in RC.STEM} == {(1, "bf16"), (1, "blk"), (3, "bf16"), (3, "blk")}
    p = [r.split() for r in fam("persist")]
    assert {(r[2], r[3]) for r in p} == {("s1x1", "4x64"), ("s1x1", "8x32"), ("s2x2", "2x64"), ("s2x2", "4x32")}
    assert {r[6] for r in p} == {"wres0", "wres1"} and {r[7] for r in p} == {"epi0", "epi1", "epi2"} and {r[8] for r in p} == {"cpb1", "cpb2"}
    assert {c.cout for c in RC.PERSIST} == {32, 64} and any(s[3] == 2 for c in RC.PERSIST for s in c.srcs)
    assert any(len(c.srcs) == 3 and "wres0" in c.route for c in RC.PERSIST)
    assert len(set(fam("blk1"))) == 8 and {r.split()[-1] for r in fam("blk1")} == {"nw4", "nw8"} and any(" sl2 " in r for r in fam("blk1"))
    for f, n in (("tiled", 5 * 8 - 2 * 2 + 8), ("tiled-x3", 2 * (2 * 8 + 3 * 6))):
        assert len(set(fam(f))) == n, (f, len(set(fam(f))))
    assert {c.srcs[0][5] for c in RC.TILED_NOT_WIDE} >= {"f32", "bf16off", "blk"} and all("wide1" in c.route for c in RC.TILED_WIDE)
    assert all(c.N <= 9 for c in RC.CASES)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
BASE = 1 << 20


def query(srcs, cout, k, stride, N, out_code, res_code=0, res_mode=0, relu=1, post=False, x3=0, out_ptr=BASE, wt_ptr=BASE, ho=None, wo=None):
    """`tpspp_conv2d_bf16_route` on made-up addresses: srcs [(C, H, W, uh, uw, layout code, address)] -> (code, message)."""
    lib = _lib.lib()
    dims = (ctypes.c_int * (6 * len(srcs)))(*[v for s in srcs for v in s[:6]])
    ptrs = (ctypes.c_void_p * len(srcs))(*[s[6] for s in srcs])
    hi, wi = srcs[0][1] * srcs[0][3], srcs[0][2] * srcs[0][4]
    p = (k - 1) // 2
    ho = (hi + 2 * p - k) // stride[0] + 1 if ho is None else ho
    wo = (wi + 2 * p - k) // stride[1] + 1 if wo is None else wo
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    args = [vp(ptrs), vp(dims), len(srcs), wt_ptr, BASE, BASE if res_mode else None, res_code, BASE if post else None,
            BASE if post else None, res_mode, relu, N, cout, k, k, stride[0], stride[1], out_ptr, out_code, ho, wo, x3]
    return lib.tpspp_conv2d_bf16_route(*args), args


def test_the_sweep_returns_exactly_the_routes_of_the_table():
    """Shapes x layouts x alignments x N, wide enough for every branch of every `*_route`; layout codes: 0 bf16, 1 fp32, 2 blocked
    bf16, 3 blocked fp32."""
    seen = set()
    maps = [(h, w) for h in (1, 2, 3, 4, 5, 8, 9, 16) for w in (8, 13, 16, 20, 32, 40, 64, 70, 128, 136)]
    maps += [(18, 13), (1, 260)]          # at stride 2: more than 8 rows of at most 16, a row of more than 128 tokens
    forms = ((3, (1, 1)), (3, (2, 2)), (3, (2, 1)), (1, (1, 1)), (1, (2, 2)))
    plain_srcs = [[(1, 1)], [(3, 1)], [(24, 0)], [(24, 0, 2)], [(32, 2)], [(48, 2)], [(64, 2)], [(64, 2)] * 3, [(128, 2)], [(256, 2)],
                  [(512, 2)], [(32, 2, 0, 2)]]
    x3_srcs = [[(24, 1)], [(32, 3)], [(32, 0)]]
    n_calls = 0
    for x3, src_sets, outs in ((0, plain_srcs, (0, 1, 2)), (1, x3_srcs, (1, 3))):
        for (k, stride), (h, w), ss, cout, out_code, res, N in itertools.product(
                forms, maps, src_sets, (24, 32, 64, 128, 256, 512), outs, (0, 1), (3, 4)):
            if cout % 8 and out_code >= 2:
                continue
            srcs = []
            for s in ss:
                ch, lay = s[0], s[1]
                off, up = (s[2] if len(s) > 2 else 0), (s[3] if len(s) > 3 else 1)
                if h % up or w % up:
                    break
                srcs.append((ch, h // up, w // up, up, up, lay, BASE + off))
            else:
                rc, _ = query(srcs, cout, k, stride, N, out_code, res_code=(3 if x3 else 2) if res else 0, res_mode=res, x3=x3)
                assert rc >= 0, (rc, _lib.lib().tpspp_last_error().decode())
                seen.add(rc)
                n_calls += 1
    seen = {ops.conv2d_bf16_route_name(code) for code in seen}
    table = {c.route for c in RC.CASES} | {c.fallback for c in RC.CASES if c.fallback}
    print(f"{n_calls} queries, {len(seen)} routes")
    assert seen - table == set(), sorted(seen - table)
    assert table - seen == set(), sorted(table - seen)


def test_codes_and_names_are_one_to_one():
    """Distinct routes of the table come from distinct codes, and every field survives the packing."""
    lib = _lib.lib()
    assert ops.conv2d_bf16_route_name(5 | 8 | (1 << 4) | (1 << 6) | (8 << 8) | (32 << 13) | (1 << 22) | (1 << 25) | (1 << 27) | (2 << 28) | (1 << 30)) \
        == "persist 3x3 s1x1 8x32 ni1 nf2 wres1 epi2 cpb2"
    assert ops.conv2d_bf16_route_name(6 | (1 << 4) | (1 << 6) | (8 << 8) | (16 << 12) | (2 << 17) | (4 << 19)) == "blk1 1x1 s1x1 nt8 nks16 sl2 nw4"
    assert ops.conv2d_bf16_route_name(1 | 8 | (2 << 4) | (1 << 6) | (1 << 8) | (256 << 13) | (4 << 22) | (3 << 25) | (1 << 27) | (1 << 28)) \
        == "tiled-x3 3x3 s2x1 1x256 ni4 nf4 wide1 nb2"
    assert lib.tpspp_conv_bf16_chunk_channels(3) == 16 and lib.tpspp_conv_bf16_chunk_channels(1) == 32


def test_alignment_of_each_pointer_the_route_reads():
    blk1 = lambda **kw: ops.conv2d_bf16_route_name(query([(64, 4, 8, 1, 1, 2, kw.pop("src", BASE))], 64, 1, (1, 1), 8, 2, **kw)[0])  # noqa: E731
    assert blk1().startswith("blk1")
    for kw in (dict(src=BASE + 8), dict(out_ptr=BASE + 8), dict(wt_ptr=BASE + 8)):
        assert blk1(**kw) == "tiled 1x1 s1x1 4x16 ni2 nf1 wide0 nb2", kw
    stem = lambda **kw: ops.conv2d_bf16_route_name(query([(3, 4, 128, 1, 1, 1, kw.pop("src", BASE))], 32, 3, (1, 1), 2, 0, **kw)[0])  # noqa: E731
    assert stem().startswith("stem") and stem(src=BASE + 4).startswith("stem")          # the fp32 image is read by elements
    for kw in (dict(out_ptr=BASE + 2), dict(wt_ptr=BASE + 8)):
        assert stem(**kw) == "tiled 3x3 s1x1 2x128 ni1 nf2 wide0 nb2", kw
    wide = lambda a, b=BASE: ops.conv2d_bf16_route_name(query([(16, 5, 40, 1, 1, 0, a), (16, 5, 40, 1, 1, 0, b)], 64, 3, (1, 1), 3, 0)[0])  # noqa: E731
    assert wide(BASE) == "tiled 3x3 s1x1 4x64 ni1 nf2 wide1 nb2"
    for a, b in ((BASE + 2, BASE), (BASE, BASE + 2), (BASE + 8, BASE)):
        assert wide(a, b) == "tiled 3x3 s1x1 4x64 ni1 nf2 wide0 nb2"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
S = (24, 9, 13, 1, 1, 0, BASE)
REFUSALS = [
    (dict(srcs=[S], k=5), "tpspp_conv2d_bf16_fwd: kernel must be 1x1 or 3x3"),
    (dict(srcs=[S] * 4), "tpspp_conv2d_bf16_fwd: 1..3 sources"),
    (dict(srcs=[S], wt_ptr=None), "tpspp_conv2d_bf16_fwd: null pointer"),
    (dict(srcs=[S], out_ptr=None), "tpspp_conv2d_bf16_fwd: null pointer"),
    (dict(srcs=[S], N=-1), "tpspp_conv2d_bf16_fwd: bad sizes"),
    (dict(srcs=[S], relu=3), "tpspp_conv2d_bf16_fwd: activation code must be 0 (none), 1 (ReLU) or 2 (GELU)"),
    (dict(srcs=[S], res_mode=3), "tpspp_conv2d_bf16_fwd: residual / res_mode mismatch"),
    (dict(srcs=[(24, 9, 13, 1, 1, 0, None)]), "tpspp_conv2d_bf16_fwd: bad source 0"),
    (dict(srcs=[(24, 3, 13, 3, 1, 0, BASE)]), "tpspp_conv2d_bf16_fwd: upsampling factors must be 1, 2 or 4"),
    (dict(srcs=[(24, 9, 13, 1, 1, 0, BASE), (16, 9, 13, 1, 1, 0, BASE)]),
     "tpspp_conv2d_bf16_fwd: concatenated sources need channel counts that are multiples of 16"),
    (dict(srcs=[(16, 9, 13, 1, 1, 0, BASE), (16, 9, 13, 1, 1, 0, BASE)], k=1),
     "tpspp_conv2d_bf16_fwd: concatenated sources need channel counts that are multiples of 32"),
    (dict(srcs=[(16, 9, 13, 1, 1, 0, BASE), (16, 3, 13, 2, 1, 0, BASE)]), "tpspp_conv2d_bf16_fwd: sources disagree on the logical size"),
    (dict(srcs=[S], wo=12), "tpspp_conv2d_bf16_fwd: output size does not match input size / stride ('same' padding)"),
    (dict(srcs=[(20, 9, 13, 1, 1, 2, BASE)]),
     "tpspp_conv2d_bf16_fwd: source 0: layout code must be 0 / 1 / 2 / 3 (blocked: channels a multiple of 8; 2 bf16 not with split3, 3 fp32 "
     "only with split3)"),
    (dict(srcs=[S], out_code=3),
     "tpspp_conv2d_bf16_fwd: residual / output layout code must be 0 / 1 / 2 / 3 (blocked: Cout a multiple of 8; 2 bf16 not with split3, "
     "3 fp32 only with split3)"),
    (dict(srcs=[S], N=65536), "tpspp_conv2d_bf16_fwd: grid too large"),
    (dict(srcs=[S], stride=(1, 2), wo=7), "tpspp_conv2d_bf16_fwd: no kernel for a 3x3 kernel with stride (1,2)"),
    (dict(srcs=[S], stride=(2, 1), k=1, ho=5), "tpspp_conv2d_bf16_fwd: no kernel for a 1x1 kernel with stride (2,1)"),
    (dict(srcs=[(24, 9, 13, 1, 1, 1, BASE)], stride=(3, 3), x3=1, ho=3, wo=5), "tpspp_conv2d_bf16_fwd: no kernel for a 3x3 kernel with stride (3,3)"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[r[1].split(": ", 1)[1][:40] + f" #{i}" for i, r in enumerate(REFUSALS)])
def test_the_query_refuses_what_the_forward_refuses_in_the_forwards_words(kw, text):
    """The forward checks its arguments and picks its route before it touches a device, so it can be asked here as well."""
    lib = _lib.lib()
    kw = dict(dict(cout=40, k=3, stride=(1, 1), N=2, out_code=0), **kw)
    rc, args = query(**kw)
    assert rc == -22 and lib.tpspp_last_error().decode() == text, (rc, lib.tpspp_last_error().decode())
    assert lib.tpspp_conv2d_bf16_fwd(*args, None) == -22 and lib.tpspp_last_error().decode() == text


def test_the_wrapper_raises_the_librarys_refusal():
    c = RC.case("stride (1,2)", [(24, 9, 13, 1, 1, "bf16")], 40, 3, (1, 2), 2, "")
    with pytest.raises(_lib.TpsppError, match=r"no kernel for a 3x3 kernel with stride \(1,2\)"):
        RC.route_of(c)
    with pytest.raises(ValueError, match="source channels != Cin"):
        ops.conv2d_bf16_route([torch.empty((2, 8, 9, 13), device="meta")], RC.weights_of(c))


def test_the_query_works_with_no_device_visible():
    """A fresh process that sees no GPU (and never imports torch) asks for a persistent-kernel route, whose launch would query the
    CU count, and gets it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = (
        "import ctypes, importlib.util, os\n"
        f"spec = importlib.util.spec_from_file_location('_lib', os.path.join({root!r}, 'tps_pp_amd', '_lib.py'))\n"
        "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)\n"
        "lib = m.lib()\n"
        "dims = (ctypes.c_int * 6)(64, 8, 64, 1, 1, 2)\n"
        "ptrs = (ctypes.c_void_p * 1)(1 << 20)\n"
        "vp = lambda a: ctypes.cast(a, ctypes.c_void_p)\n"
        "print(lib.tpspp_conv2d_bf16_route(vp(ptrs), vp(dims), 1, 1 << 20, None, None, 0, None, None, 0, 1, 3, 64, 3, 3, 1, 1, 1 << 20, 2, 8, 64, 0))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert ops.conv2d_bf16_route_name(int(out.stdout.strip())) == "persist 3x3 s1x1 4x64 ni1 nf2 wres1 epi0 cpb2"


def test_exact_data_stays_inside_fp32s_integers_and_bf16():
    assert (RC.EXACT_MAX_K * 8 * 4 + 64 + 64) * 2 + 64 < 2 ** 24
    c = RC.EPILOGUE_SHAPES["x3 3x3 s1x1"]
    d = RC.make_inputs(c, True)
    for key in ("w", "bias", "res", "post_scale", "post_shift"):
        t = d[key]
        assert torch.equal(t, t.round()) and torch.equal(RC.rb(t), t), key         # a bf16 number: hi = the value, lo = 0
    hi, lo = ops._hi_lo(d["xs"][0])
    assert torch.equal(hi.float(), d["xs"][0]) and not lo.any()
    # in the exact data the three-term restatement IS the plain product
    y3 = RC.conv_sum(c, d["xs"], d["w"])
    y1 = RC.conv_sum(c._replace(x3=False), d["xs"], d["w"])
    assert torch.equal(y3, y1) and y3.abs().max() > 256
    # the real data of a bf16 tensor is what the kernel reads
    r = RC.make_inputs(RC.EPILOGUE_SHAPES["3x3 s1x1"], False)
    assert torch.equal(RC.rb(r["xs"][0]), r["xs"][0]) and not torch.equal(RC.rb(r["w"]), r["w"])
