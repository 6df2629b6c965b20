"""Host side of the memory-safety sweep (no GPU): the guard harness tests itself on the CPU device, every exported entry
point of include/tpspp.h is either named by a sweep case or excluded with a reason, the conv-backward backbone table is
the backbone's own list of convolutions, and the NaN assertion of the conv-backward bar holds."""
import pytest
import torch
import torch.nn as nn

import guarded_alloc as GA
import test_gpu_conv_bwd as TB
import test_gpu_memory_safety as MS
from test_capi_symbols import header_functions

_QUERY = "a size or version query: computes on the host, touches no device memory"
_KNOB = "sets a process-wide host-side switch: touches no device memory"
_HOST = "reads and writes host memory only"
_PLAN = "host-side bookkeeping of a prepared call; its launch is tpspp_warp_plan_run, which is swept"
EXCLUDED = {
    "tpspp_abi_version": _QUERY, "tpspp_last_error": _QUERY, "tpspp_prepared_table_floats": _QUERY,
    "tpspp_conv_chunk_channels": _QUERY, "tpspp_conv_bf16_chunk_channels": _QUERY, "tpspp_conv2d_route": _QUERY,
    "tpspp_conv2d_bwd_weight_workspace_floats": _QUERY, "tpspp_linear_bwd_weight_workspace_floats": _QUERY,
    "tpspp_plane_ln_bwd_workspace_floats": _QUERY, "tpspp_cbam_bwd_workspace_floats": _QUERY,
    "tpspp_bn_stats_workspace_floats": _QUERY, "tpspp_bn_bwd_reduce_workspace_floats": _QUERY,
    "tpspp_warp_bwd_workspace_floats": _QUERY, "tpspp_nrtr_encoder_workspace": _QUERY, "tpspp_nrtr_decoder_workspace": _QUERY,
    "tpspp_nrtr_decoder_route": _QUERY, "tpspp_warp_bwd_route": _QUERY, "tpspp_conv2d_bf16_route": _QUERY,
    "tpspp_conv_set_tuning": _KNOB, "tpspp_warp_set_tuning": _KNOB, "tpspp_warp_set_trace": _KNOB,
    "tpspp_head_set_trace": _KNOB, "tpspp_warp_bwd_set_accumulator": _KNOB,
    "tpspp_table_mirror_symmetry": _HOST,
    "tpspp_warp_plan_create": _PLAN, "tpspp_warp_plan_destroy": _PLAN,
    "tpspp_warp_plan_run_on": "tpspp_warp_plan_run with an explicit stream: the same launch (multi-stream paths are out of "
                              "the sweep's scope)",
    "tpspp_lab_occupy": "a laboratory kernel that only occupies compute units: it has no output",
}


def test_every_exported_entry_point_is_swept_or_excluded_with_a_reason():
    decl = set(header_functions())
    assert decl, "no declarations parsed from include/tpspp.h"
    swept = set(MS.SWEPT)
    assert not swept - decl, f"sweep cases name functions the header does not declare: {sorted(swept - decl)}"
    assert not set(EXCLUDED) - decl, f"exclusions the header does not declare: {sorted(set(EXCLUDED) - decl)}"
    assert not swept & set(EXCLUDED), f"both swept and excluded: {sorted(swept & set(EXCLUDED))}"
    missing = decl - swept - set(EXCLUDED)
    assert not missing, f"no guard case and no exclusion for: {sorted(missing)} (tests/test_gpu_memory_safety.py)"
    assert all(isinstance(r, str) and len(r) > 20 for r in EXCLUDED.values())


def test_partly_written_list_exempts_regions_with_the_headers_own_sentence():
    import os
    header = " ".join(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                                        "tpspp.h")).read().split())
    names = [e[0] for e in MS.PARTLY_WRITTEN]
    assert len(names) == len(set(names)), "at most one entry per entry point"
    for name, region, sentence in MS.PARTLY_WRITTEN:
        assert name in MS.SWEPT and region and " ".join(sentence.split()) in header, name


def test_backbone_table_is_the_backbones_own_list_of_convolutions():
    from tps_pp_amd import ResNetABI_v2_large
    m = ResNetABI_v2_large(strides=[2, 1, 2, 1, 2]).train()
    seen = set()
    for mod in m.modules():
        if isinstance(mod, nn.Conv2d):
            mod.register_forward_hook(lambda c, inp, out: seen.add(
                (c.in_channels, c.out_channels, c.kernel_size[0], tuple(c.stride), inp[0].shape[2], inp[0].shape[3],
                 c.bias is not None)))
    with torch.no_grad():
        m._forward_torch(torch.zeros(1, 3, 32, 128))
    assert seen == {tuple(row[1:]) for row in TB.BACKBONE_LAYERS}
    assert len({row[0] for row in TB.BACKBONE_LAYERS}) == len(TB.BACKBONE_LAYERS)
    # both batch sizes, the backbone's own calling convention (relu = 0, dZ as dY) and the ReLU-masked one, for every row
    # and for the ragged multi-tile case; all of them run under the element-wise bar and in the sweep
    rows = len(TB.BACKBONE_LAYERS) + 1
    assert len(TB.BACKBONE_CASES) == 4 * rows
    assert {(c[7], c[5]) for c in TB.BACKBONE_CASES} == {(3, 0), (3, 1), (5, 0), (5, 1)}
    _, ci, co, k, st, H, W, _ = TB.BACKBONE_RAGGED
    assert ci % 64 and co % 64 and ci > 128 and co > 128 and H % 2 and W % 2 and st == (2, 1)
    assert all(c in MS.BWD_CASES for c in TB.BACKBONE_CASES + TB.RAGGED)


def test_conv_backward_bar_refuses_nan():
    want = torch.ones(4, 4, dtype=torch.float64)
    TB.check("fine", torch.ones(4, 4), want, want)
    bad = torch.ones(4, 4)
    bad[1, 2] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        TB.check("nan", bad, want, want)
    bad[1, 2] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        TB.check("inf", bad, want, want)


# ---- the harness on the CPU device -------------------------------------------------------------------------------------

def test_allocations_are_poisoned_aligned_and_recorded():
    with GA.guarded("cpu") as g:
        a = torch.empty((3, 5))
        b = torch.empty(7, dtype=torch.bfloat16)
        c = torch.empty_like(a)
        d = torch.empty(4, dtype=torch.int32)
        e = torch.empty_like(a, dtype=torch.float64)
        assert len(g.records) == 5
        for x in (a, b, c, d, e):
            assert x.data_ptr() % GA.ALIGN == 0 and x.is_contiguous()
        assert torch.isnan(a).all() and torch.isnan(b.float()).all() and torch.isnan(c).all() and torch.isnan(e).all()
        assert (d == -1).all() and a.shape == (3, 5) and e.dtype == torch.float64
        assert all(GA.poison_count(x) == x.numel() for x in (a, b, c, e)) and GA.poison_count(d) == 0
        # what is not a plain allocation on the guarded device goes to the real functions
        assert torch.empty(0).numel() == 0 and torch.empty((2, 0, 3)).shape == (2, 0, 3)
        torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        torch.empty(3, pin_memory=False)
        torch.empty_like(a, memory_format=torch.contiguous_format)
        torch.empty(3, device="meta")
        assert len(g.records) == 5
        # autograd and matmul work unchanged inside the context
        x = torch.randn(4, 4, requires_grad=True)
        (x @ x).sum().backward()
        assert x.grad is not None
        for r in g.records:
            assert r.off >= GA.GUARD and r.buf.numel() - r.off - r.nbytes >= GA.GUARD and "test_memory_safety_host" in r.where


def test_inputs_sit_between_nan_bands():
    src = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    with GA.guarded("cpu") as g:
        x = g.input(src)
        assert torch.equal(x, src) and x.data_ptr() % GA.ALIGN == 0
        r = g.records[0]
        before = r.buf[r.off - GA.GUARD:r.off].view(torch.float32)
        after = r.buf[r.off + r.nbytes:r.off + r.nbytes + GA.GUARD].view(torch.float32)
        assert torch.isnan(before).all() and torch.isnan(after).all()
        assert (r.buf[:r.off - GA.GUARD] == GA.GUARD_BYTE).all() and (r.buf[r.off + r.nbytes + GA.GUARD:] == GA.GUARD_BYTE).all()
        i = g.input(torch.tensor([3, 1, 2], dtype=torch.int32))
        assert i.tolist() == [3, 1, 2]
        assert g.check(x, require_guarded=True) == 0 and len(g.records) == 2      # inputs are not allocations
        torch.as_strided(x, (1,), (1,), x.storage_offset() - 1).fill_(0.0)      # a store into the leading NaN band
        with pytest.raises(GA.GuardError, match="4 bytes before the payload"):
            g.check(x)


def test_patched_functions_are_restored_after_an_exception():
    with pytest.raises(RuntimeError, match="boom"):
        with GA.guarded("cpu"):
            assert torch.empty is not GA._REAL_EMPTY
            raise RuntimeError("boom")
    assert torch.empty is GA._REAL_EMPTY and torch.empty_like is GA._REAL_EMPTY_LIKE
    assert not torch.isnan(torch.zeros(3) + torch.empty(3).fill_(0)).any()


def test_a_write_one_element_past_a_payload_fails_check():
    """Through as_strided on the harness's own buffer: legal memory, not an out-of-bounds access."""
    with GA.guarded("cpu") as g:
        a = torch.empty((3, 5))
        a.fill_(1.0)
        assert g.check(a) == 1
        torch.as_strided(a, (1,), (1,), a.storage_offset() + a.numel()).fill_(3.0)
        with pytest.raises(GA.GuardError) as ei:
            g.check(a)
        msg = str(ei.value)
        assert "guard after allocation (3, 5) torch.float32" in msg and "0 bytes past its end" in msg
        assert "test_memory_safety_host.py" in msg and "payload offset 60" in msg
    with GA.guarded("cpu") as g:
        a = torch.empty(8, dtype=torch.bfloat16)
        a.fill_(1.0)
        torch.as_strided(a, (1,), (1,), a.storage_offset() - 1).fill_(3.0)
        with pytest.raises(GA.GuardError, match="guard before allocation .* 2 bytes before the payload"):
            g.check(a)


def test_an_unwritten_output_element_fails_check():
    with GA.guarded("cpu") as g:
        a, b = torch.empty((3, 5)), torch.empty(6, dtype=torch.bfloat16)
        a.fill_(0.5)
        b.fill_(0.5)
        a[1, 3] = float("nan")                            # an ordinary NaN is a value, not the poison word
        assert g.check({"a": a, "rest": [(b,)]}) == 2
        a.view(torch.int32)[2, 4] = -1
        with pytest.raises(GA.GuardError, match=r"1 elements never written .* flat index 14"):
            g.check({"a": a, "rest": [(b,)]})
        a.fill_(0.5)
        b.view(torch.int16)[5] = -1
        with pytest.raises(GA.GuardError, match="tensor #1"):
            g.check({"a": a, "rest": [(b,)]})


def test_outputs_outside_the_guards_and_unserved_requests_are_not_silent():
    import numpy as np
    with GA.guarded("cpu") as g:
        a = torch.empty(np.int64(3), np.int32(5))         # dimensions that are no Python ints are served all the same
        b = torch.empty((np.int64(4),))
        assert len(g.records) == 2 and a.shape == (3, 5) and b.shape == (4,) and not g.fallthrough
        a.fill_(1.0)
        b.fill_(1.0)
        assert g.check([a, a[1:], b], require_guarded=True) == 2
        c = a.clone()                                     # a float output that some other allocator made
        g.check([a, c])
        with pytest.raises(GA.GuardError, match="tensor #1 .* lies in no guarded allocation"):
            g.check([a, c], require_guarded=True)
        assert g.check([a, GA.Unguarded(c, "a clone made by a torch op")], require_guarded=True) == 2
        c.view(torch.int32)[0, 0] = -1                    # ... which is still held to the poison test
        with pytest.raises(GA.GuardError, match="never written"):
            g.check(GA.Unguarded(c, "a clone made by a torch op"))
        assert list(GA.tensors_in([GA.Unguarded(c, "a clone made by a torch op"), GA.Unguarded(None, "an absent output")])) == [c]
        # requests on the device that the patch does not serve are listed; empty ones and other devices are not
        torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        torch.empty_like(a.t())
        torch.empty(0)
        torch.empty(3, device="meta")
        assert len(g.fallthrough) == 2 and all("test_memory_safety_host" in w for w, _ in g.fallthrough)
        assert "memory_format" in g.fallthrough[0][1] and "empty_like" in g.fallthrough[1][1]


def test_same_bits_compares_as_integers():
    a = torch.tensor([0.0, float("nan"), 1.0])
    assert GA.same_bits([a, {"k": a}], [a.clone(), {"k": a.clone()}])[0]
    assert not GA.same_bits(a, torch.tensor([-0.0, float("nan"), 1.0]))[0]
    assert not GA.same_bits(torch.tensor([1, 2]), torch.tensor([1, 3]))[0]
    assert not GA.same_bits([a], [a, a])[0]
