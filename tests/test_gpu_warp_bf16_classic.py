"""-m gpu tests of TPSPP_IO_BF16 on the classic rectifier (tpspp_warp_geo_bf16.h): bf16 images in and out with the prepared
table.  The fp32 classic kernels are pinned bit for bit to the CPU oracle on these shapes (test_gpu_warp.py), and the bf16
kernel's arithmetic is theirs with one round-to-nearest-even at the store, so every comparison here is bit for bit:
against the oracle's fp32 result rounded once, and against the fp32 kernel's result rounded once."""
import functools

import numpy as np
import pytest
import torch

import cases
import guarded_alloc as GA
from tps_pp_amd import _lib, constants, ops, synth
from tps_pp_amd.tps_preprocessor import TPSPreprocessor

pytestmark = pytest.mark.gpu

F = 20
# (N, C, H, W, perturb); a perturbation >= 0.3 puts taps on odd and even columns alike (a packed 16-bit read's two halves)
CASES = [
    (1, 1, 32, 100, 0.05),
    (5, 3, 32, 100, 0.3),       # odd batch
    (2, 3, 32, 100, 2.0),       # mostly clamped to the border
    (3, 3, 32, 128, 0.1),       # two quadrant pixels per thread
    (2, 1, 32, 64, 0.3),
    (3, 3, 48, 160, 0.4),       # three quadrant pixels per thread
    (2, 3, 64, 200, 0.45),      # four, two workgroups per image
    (2, 1, 64, 256, 0.45),
    (1, 3, 64, 256, 0.45),      # the largest staged image: 96 KB
    (3, 3, 16, 64, 0.3),
    (2, 1, 128, 256, 0.45),     # four workgroups per image
    (1, 3, 96, 256, 0.45),      # three: the non-power-of-two division of the banded copy-out, 144 KB of LDS
]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def host_inputs(N, C, H, W, perturb):
    """Host tensors of one case (computed once, never modified): constants, control points, the image rounded to bf16."""
    Kc = constants.classic(F, (H, W))
    ctrl = (constants.classic_identity_ctrl(F)[None] + perturb * synth.dyadic((N, F, 2), "b16.ctrl", N)).astype(np.float32)
    img = t(synth.dyadic((N, C, H, W), "b16.img", N + 1)).to(torch.bfloat16)
    return Kc, t(ctrl), img


@functools.lru_cache(maxsize=None)
def oracle_rounded(N, C, H, W, perturb):
    """The CPU oracle's fp32 result on the bf16-valued image, rounded once to bf16."""
    from oracle import tps_oracle
    tps_oracle.build()
    Kc, ctrl, img = host_inputs(N, C, H, W, perturb)
    ref = tps_oracle.warp(img.float().numpy(), ctrl.numpy(), Kc["inv_delta_C"], Kc["P_hat"], (H, W))
    return t(ref["out0"]).to(torch.bfloat16)


def device_inputs(cuda, N, C, H, W, perturb, put=None):
    put = put or (lambda x: x.to(cuda))
    Kc, ctrl, img = host_inputs(N, C, H, W, perturb)
    assert ops.table_mirror_symmetry(Kc["P_hat"], (H, W), F) == 1
    P_hat, inv = put(t(Kc["P_hat"])), put(t(Kc["inv_delta_C"]))
    prep, packed = ops.prepare_mirror_table(P_hat, (H, W))
    assert packed & ops.TABLE_PACKED
    return put(img), put(ctrl), inv, P_hat, prep, ops.TABLE_MIRROR4 | packed


def same_bits(a, b):
    ok, why = GA.same_bits(a.cpu(), b.cpu())
    assert ok, why


@pytest.mark.parametrize("N,C,H,W,perturb", CASES)
def test_bf16_classic_warp_is_the_oracle_rounded_once(cuda, N, C, H, W, perturb):
    img, ctrl, inv, P_hat, prep, flags = device_inputs(cuda, N, C, H, W, perturb)
    out = ops.warp(img, ctrl, inv, P_hat, (H, W), P_hat_t=prep, table_flags=flags)[0]
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (N, C, H, W)
    assert torch.equal(out.cpu(), oracle_rounded(N, C, H, W, perturb))


@pytest.mark.parametrize("N,C,H,W,perturb", CASES)
def test_bf16_classic_warp_is_the_fp32_kernel_rounded_once(cuda, N, C, H, W, perturb):
    img, ctrl, inv, P_hat, prep, flags = device_inputs(cuda, N, C, H, W, perturb)
    out = ops.warp(img, ctrl, inv, P_hat, (H, W), P_hat_t=prep, table_flags=flags)[0]
    f32, _, grid32, idx32 = ops.warp(img.float(), ctrl, inv, P_hat, (H, W), want_grid=True, want_idx=True,
                                     P_hat_t=prep, table_flags=flags)
    same_bits(out, f32.bfloat16())
    # the optional outputs take another instantiation: fp32 / int32 with the fp32 call's bits, the image unchanged
    out_aux, _, grid, idx = ops.warp(img, ctrl, inv, P_hat, (H, W), want_grid=True, want_idx=True,
                                     P_hat_t=prep, table_flags=flags)
    assert grid.dtype == torch.float32 and idx.dtype == torch.int32
    same_bits(grid, grid32)
    assert torch.equal(idx, idx32)
    same_bits(out_aux, out)


def test_bf16_warp_plan(cuda):
    N, C, H, W, perturb = 5, 3, 32, 100, 0.3
    img, ctrl, inv, P_hat, prep, flags = device_inputs(cuda, N, C, H, W, perturb)
    want = ops.warp(img, ctrl, inv, P_hat, (H, W), P_hat_t=prep, table_flags=flags)[0]
    out_p = torch.full((N, C, H, W), float("nan"), device=cuda, dtype=torch.bfloat16)
    plan = ops.WarpPlan(img, ctrl, inv, P_hat, (H, W), out_p, P_hat_t=prep, table_flags=flags)
    plan.run()
    same_bits(out_p, want)
    out_p.fill_(float("nan"))
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    plan.run(side)
    side.synchronize()
    same_bits(out_p, want)
    # mixed dtypes stay refused
    with pytest.raises(TypeError):
        ops.WarpPlan(img, ctrl, inv, P_hat, (H, W), torch.empty((N, C, H, W), device=cuda), P_hat_t=prep, table_flags=flags)
    with pytest.raises(TypeError):
        ops.WarpPlan(img.float(), ctrl, inv, P_hat, (H, W), out_p, P_hat_t=prep, table_flags=flags)


@pytest.mark.parametrize("N,C,H,W,perturb", [(5, 3, 32, 100, 0.3), (2, 3, 64, 200, 0.45)])
def test_bf16_classic_warp_between_guard_bands(cuda, N, C, H, W, perturb):
    """No byte outside out0 is written, every element of out0 is, and guarded and plain runs have the same bits."""
    def fn(put):
        img, ctrl, inv, P_hat, prep, flags = device_inputs(cuda, N, C, H, W, perturb, put)
        return ops.warp(img, ctrl, inv, P_hat, (H, W), P_hat_t=prep, table_flags=flags)[0]
    plain = fn(None)
    torch.cuda.synchronize()
    with GA.guarded(cuda) as g:
        got = fn(g.input)
        n = g.check(got, require_guarded=True)
    assert n > 0 and not g.fallthrough, g.fallthrough
    assert got.dtype == torch.bfloat16
    ok, why = GA.same_bits(got, plain)
    assert ok, "guarded and plain runs differ: " + why


def test_bf16_classic_refusals(cuda):
    N, C, H, W, perturb = 2, 3, 32, 100, 0.3
    img, ctrl, inv, P_hat, prep, flags = device_inputs(cuda, N, C, H, W, perturb)

    def refused(fn):
        with pytest.raises(_lib.TpsppError) as e:
            fn()
        assert "TPSPP_IO_BF16" in str(e.value) and len(str(e.value)) > 40, str(e.value)
        return str(e.value)

    assert "p_hat_t" in refused(lambda: ops.warp(img, ctrl, inv, P_hat, (H, W)))
    msg = refused(lambda: ops.warp(img, ctrl, inv, P_hat, (H, W), P_hat_t=ops.transpose_p_hat(P_hat), table_flags=ops.TABLE_MIRROR4))
    assert "TPSPP_TABLE_PACKED" in msg
    img4 = torch.zeros((N, 4, H, W), device=cuda, dtype=torch.bfloat16)
    assert "C0" in refused(lambda: ops.warp(img4, ctrl, inv, P_hat, (H, W), P_hat_t=prep, table_flags=flags))
    tall = torch.zeros((N, C, 2 * H, W), device=cuda, dtype=torch.bfloat16)
    refused(lambda: ops.warp(tall, ctrl, inv, P_hat, (H, W), P_hat_t=prep, table_flags=flags))
    K10 = constants.classic(10, (H, W))
    P10 = t(K10["P_hat"]).to(cuda)
    prep10, packed10 = ops.prepare_mirror_table(P10, (H, W))
    ctrl10 = t(constants.classic_identity_ctrl(10)[None].repeat(N, 0).astype(np.float32)).to(cuda)
    assert "F" in refused(lambda: ops.warp(img, ctrl10, t(K10["inv_delta_C"]).to(cuda), P10, (H, W), P_hat_t=prep10,
                                           table_flags=ops.TABLE_MIRROR4 | packed10))


def golden_module(cuda):
    m = TPSPreprocessor(num_fiducial=cases.CL_F, img_size=cases.CL_HW,
                        rectified_img_size=cases.CL_HW, num_img_channel=3).eval()
    sd = cases.synth_state(m.state_dict(), 1, cases.g1_state_rule, cases.G1_KEEP)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.to(cuda)


def test_module_unset_keeps_fp32_output(cuda):
    m = golden_module(cuda)
    x = t(cases.g1_inputs()["img"]).to(cuda).to(torch.bfloat16)
    with torch.no_grad():
        got, want = m(x), m(x.float())
    assert got.dtype == torch.float32
    same_bits(got, want)


def test_module_bf16_against_the_golden_run(cuda):
    """The bar of test_gpu_modules.py::test_classic_module_bf16_localisation: the same network in front of the same
    arithmetic."""
    G = cases.load("classic_module")
    m = golden_module(cuda)
    assert m.set_compute_dtype(torch.bfloat16) is m
    img = t(cases.g1_inputs()["img"]).to(cuda)
    with torch.no_grad():
        out = m(img)                        # an fp32 input is cast once
        out_b = m(img.to(torch.bfloat16))
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == G["out"].shape
    same_bits(out, out_b)
    err = np.abs(out.float().cpu().numpy() - G["out"]).mean()
    print(f"mean abs error {err:.3e}, bound {5e-3 * np.abs(G['out']).max():.3e}")
    assert err <= 5e-3 * np.abs(G["out"]).max()


def test_module_bf16_rectify(cuda):
    N, C, H, W, perturb = 5, 3, 32, 100, 0.3
    _, ctrl, img = host_inputs(N, C, H, W, perturb)
    m = TPSPreprocessor(num_fiducial=F, img_size=(H, W), rectified_img_size=(H, W), num_img_channel=C).eval().to(cuda)
    with torch.no_grad():
        out = m.rectify(img.to(cuda), ctrl.to(cuda))
    assert out.dtype == torch.bfloat16
    assert torch.equal(out.cpu(), oracle_rounded(N, C, H, W, perturb))
