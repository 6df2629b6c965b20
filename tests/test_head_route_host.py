"""Host side of the recogniser head's decoder (no GPU): the workspace sizes `tpspp_nrtr_encoder_workspace` /
`tpspp_nrtr_decoder_workspace` report and the route `tpspp_nrtr_decoder_route` names, each against a restatement in Python.

The restatements were written from the formulas and the selection conditions of the entry points as they stood BEFORE the
workspace layout and the route became values (`enc_ws_bytes` / `dec_ws_bytes` and the `fast` / `persist` / `kern` lines of
`tpspp_nrtr_decoder_fwd`), not from `EncWorkspace` / `DecWorkspace` / `dec_route()`: a buffer added to the layout, or a
shape that silently changes pipeline, fails here.  The reduced-precision pipelines agree with each other only within 2e-5,
so no tolerance test would notice the latter."""
import itertools
import os
import re

import pytest
import torch

from tps_pp_amd import _lib, build, ops

D_COUNT = 24                      # pointers per decoder layer (include/tpspp.h); the last six are the arranged projections
K_P_MAX_LAYERS = 8                # tpspp_head_persist.h: kPMaxLayers


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


# ---- workspace sizes ---------------------------------------------------------------------------------------------------

def a256(v):
    return (v + 255) & ~255


def enc_bytes(N, C, T, Di):
    M = N * T
    return a256(C * M * 4) * 3 + a256(3 * C * M * 4) + a256(Di * M * 4)


def dec_bytes(N, C, T, Di, n_layers, L, Cc):
    MT = N * T
    s = n_layers * 2 * a256(C * MT * 4)                # Kx, Vx_t per layer
    s += n_layers * 2 * a256(N * C * L * 4)            # self-attention caches
    s += 3 * a256(C * N * 4)                           # x, y, a
    s += a256(3 * C * N * 4)                           # qkv_t
    s += a256(Di * N * 4)                              # hidden
    s += a256(Cc * N * 4)                              # logits
    s += a256(N * (L + 1) * 4)                         # tokens
    s += a256(C * MT * 4)                              # keys before their transposition
    s += a256(((N + 31) // 32 * 32 + 64) * 4)          # cluster counters (128 B apart) + error flag
    return s


NS, CS, TS, DIS = (1, 31, 32, 33, 513), (64, 256, 512), (1, 64, 65, 256), (256, 512, 100)


def test_encoder_workspace_is_the_sum_of_its_five_buffers(lib):
    for N, C, T, Di in itertools.product(NS, CS, TS, DIS):
        assert lib.tpspp_nrtr_encoder_workspace(N, C, T, Di) == enc_bytes(N, C, T, Di), (N, C, T, Di)


def test_decoder_workspace_is_the_sum_of_its_buffers(lib):
    n = 0
    for N, C, T, Di, nl, L, Cc in itertools.product(NS, CS, TS, DIS, (1, 6, 8, 9), (1, 40, 64), (4, 93, 128)):
        assert lib.tpspp_nrtr_decoder_workspace(N, C, T, Di, nl, L, Cc) == dec_bytes(N, C, T, Di, nl, L, Cc), \
            (N, C, T, Di, nl, L, Cc)
        n += 1
    assert n == 6480


def test_workspace_queries_return_zero_for_arguments_that_are_not_positive(lib):
    good = [3, 512, 25, 256]
    for i, bad in itertools.product(range(4), (0, -1)):
        a = list(good)
        a[i] = bad
        assert lib.tpspp_nrtr_encoder_workspace(*a) == 0, a
    good = [3, 512, 25, 256, 6, 40, 93]
    assert lib.tpspp_nrtr_decoder_workspace(*good) == dec_bytes(*good)
    for i, bad in itertools.product(range(7), (0, -1)):
        a = list(good)
        a[i] = bad
        assert lib.tpspp_nrtr_decoder_workspace(*a) == 0, a


# ---- the route -----------------------------------------------------------------------------------------------------------

FLAGS = {"fp32": 0, "bf16": ops.HEAD_BF16, "bf16x3": ops.HEAD_BF16X3, "both": ops.HEAD_BF16 | ops.HEAD_BF16X3}
# DecoderRoute.persist -> dec_step_persist_kernel<KV, d_inner / 128, exact fp32 products, more than 64 encoder tokens>
INSTANTIATION = {
    0: ("fp32", 256, False, False), 1: ("fp32", 512, False, False), 2: ("bf16", 256, False, False),
    3: ("bf16", 512, False, False), 4: ("fp32", 256, True, False), 5: ("fp32", 512, True, False),
    6: ("fp32", 256, False, True), 7: ("fp32", 512, False, True), 8: ("bf16", 256, False, True),
    9: ("bf16", 512, False, True), 10: ("fp32", 256, True, True), 11: ("fp32", 512, True, True),
}
_SOME = torch.zeros(1)            # any non-NULL address: the query reads no pointer's target


def table(n_layers, arranged):
    """A decoder pointer table of which only the null-ness matters: `arranged` = "all" | "one missing" (one arranged
    projection of the middle layer) | "classifier missing"."""
    ptrs = [_SOME] * (n_layers * D_COUNT + 1)
    if arranged == "one missing":
        ptrs[(n_layers // 2) * D_COUNT + 18 + (n_layers % 6)] = None
    elif arranged == "classifier missing":
        ptrs[-1] = None
    return ops.PtrTable(ptrs)


def restated_route(flags, C, T, d_inner, num_out, n_layers, arranged):
    """The selection as `tpspp_nrtr_decoder_fwd` spelled it in line: (pipeline, kv, gemm, cross, persist)."""
    b16 = bool(flags & 1)
    x3 = not b16 and bool(flags & 2)
    gemm_f32 = not (b16 or x3)
    H = C // 64
    fast = arranged == "all" and C in (256, 512) and d_inner in (256, 512) and num_out % 4 == 0
    persist = fast and C == 512 and H == 8 and num_out <= 128 and n_layers <= K_P_MAX_LAYERS
    tbig = T > 64
    which = (6 if tbig else 0) + (2 if b16 else 4 if gemm_f32 else 0) + (0 if d_inner == 256 else 1)
    cross = 2 if fast and T <= 64 and H % 2 == 0 else 1            # (the plain pipeline: one head per wavefront)
    return ("persistent" if persist else "arranged" if fast else "plain", "bf16" if b16 else "fp32",
            "fp32" if gemm_f32 else "x3", cross, which if persist else None)


def test_route_is_the_selection_the_entry_point_made_in_line(lib):
    tables = {(nl, arr): table(nl, arr) for nl in (1, 8, 9) for arr in ("all", "one missing", "classifier missing")}
    seen, n = set(), 0
    for (fname, flags), C, Di, Cc, nl, T, arr in itertools.product(
            FLAGS.items(), (64, 256, 512), (256, 512, 100), (92, 93, 128, 132), (1, 8, 9), (64, 65),
            ("all", "one missing", "classifier missing")):
        got = ops.nrtr_decoder_route(C, T, tables[nl, arr], nl, Di, Cc, flags)
        assert tuple(got) == restated_route(flags, C, T, Di, Cc, nl, arr), (fname, C, Di, Cc, nl, T, arr)
        if got.persist is not None:
            # the index names the instantiation the nested ?: of the entry point named for these sizes and flags
            assert INSTANTIATION[got.persist] == (got.kv, Di, got.gemm == "fp32", T > 64), (fname, C, Di, Cc, nl, T)
        seen.add(got)
        n += 1
    assert n == 2592
    assert {r.persist for r in seen} == set(range(12)) | {None}
    assert {r.pipeline for r in seen} == {"plain", "arranged", "persistent"}
    assert {r.cross for r in seen if r.pipeline == "arranged"} == {1, 2}
    assert {(r.kv, r.gemm) for r in seen} == {("fp32", "fp32"), ("fp32", "x3"), ("bf16", "x3")}


def test_kernel_table_holds_the_instantiation_each_index_names():
    """The source's one table of persistent kernels, entry by entry, against INSTANTIATION."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tps_pp_amd", "csrc",
                            "tpspp_head.hip")).read()
    body = re.search(r"kPersistKernels\[12\] = \{(.*?)\};", src, flags=re.S).group(1)
    entries = re.findall(r"dec_step_persist_kernel<([^>]*)>", body)
    assert len(entries) == 12
    for i, e in enumerate(entries):
        a = [s.strip() for s in e.split(",")]
        kv = {"float": "fp32", "unsigned short": "bf16"}[a[0]]
        assert (kv, 128 * int(a[1]), a[2] == "true", len(a) > 3 and a[3] == "true") == INSTANTIATION[i], (i, e)
    # ... and it is the only place that names an instantiation
    assert len(re.findall(r"dec_step_persist_kernel<", src)) == 12 + 1          # + the comment above the table


def test_route_refuses_what_the_entry_point_refuses(lib):
    t = table(2, "all")
    assert ops.nrtr_decoder_route(512, 25, t, 2, 256, 92).pipeline == "persistent"
    for args in ((512, 25, t, 3, 256, 92), (500, 25, t, 2, 256, 92), (512, 0, t, 2, 256, 92), (512, 25, t, 2, 0, 92),
                 (512, 25, t, 2, 256, 0), (512, 25, t, 0, 256, 92)):
        with pytest.raises(_lib.TpsppError):
            ops.nrtr_decoder_route(*args)
