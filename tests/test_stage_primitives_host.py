"""CPU checks that tests/test_gpu_stage_primitives.py is itself sound: its case tables reach every branch the launchers of
the stage kernels can take (the selection is restated there and asserted here), the integer cases stay below 2^24 by bounds
computed from the tables and on the operands actually used, every float64 builder agrees with PyTorch's float64
composition written a second way, the weights are non-zero and no reference is flat or behind a dead ReLU layer, the
special DGAB, score and max-pool inputs do what they are for, and the entry points refuse bad sizes before any launch.
No GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tpspp_oracle as TO
from tps_pp_amd import _lib, build
import test_gpu_stage_primitives as SP

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def _is_int(a):
    a = np.asarray(a, np.float64)
    return bool(np.isfinite(a).all() and (a == np.round(a)).all())


def close(a, b, tol=1e-11):
    return torch.allclose(a, b, rtol=tol, atol=tol)


# ---- the tables reach every branch ------------------------------------------------------------------------------------------
def test_front_table_reaches_every_branch():
    assert SP.FRONT_CASES == ((1, 2, 2), (2, 2, 10), (3, 6, 46), (2, 18, 128), (1, 20, 128), (2, 32, 128))
    plan = {c: SP.front_plan(c[1], c[2]) for c in SP.FRONT_CASES}
    assert plan[(1, 2, 2)]["below_tile"] and plan[(1, 2, 2)]["tiles"] == 1
    assert plan[(2, 2, 10)]["below_tile"] and plan[(2, 2, 10)]["odd_half_width"] and plan[(2, 2, 10)]["ragged"]
    p = plan[(3, 6, 46)]
    assert (p["tiles"], p["gx"], p["ragged"], p["odd_half_width"]) == (2, 2, True, True) and 6 * 46 == 276
    p = plan[(2, 18, 128)]
    assert (p["tiles"], p["gx"], p["uneven"], p["ragged"], p["strided"]) == (9, 3, False, False, True)
    p = plan[(1, 20, 128)]
    assert (p["tiles"], p["gx"], p["uneven"], p["ragged"], p["strided"]) == (10, 3, True, False, True)
    p = plan[(2, 32, 128)]
    assert (p["tiles"], p["gx"], p["uneven"], p["strided"]) == (16, 4, False, True)
    for key in ("uneven", "ragged", "below_tile", "odd_half_width", "strided"):
        assert {plan[c][key] for c in SP.FRONT_CASES} == {False, True}, key
    assert any(c[0] > 1 for c in SP.FRONT_CASES) and any(c[0] == 1 for c in SP.FRONT_CASES)
    # the exact cases: below a tile with an odd half width, a ragged second tile, uneven strides
    assert set(SP.FRONT_A_CASES) <= set(SP.FRONT_CASES) and SP.FRONT_A_CASES == ((2, 2, 10), (3, 6, 46), (1, 20, 128))
    assert SP.DOWN_FUSED_CASES == ((3, 2), (2, 6), (1, 32))


def test_score_table_reaches_every_branch():
    ns = [h * w for h, w in SP.SCORE_SHAPES]
    assert ns == [1, 127, 128, 129, 250, 1024] and SP.SCORE_N == 2
    plan = {n: SP.score_plan(n) for n in ns}
    assert [plan[n]["blocks"] for n in ns] == [1, 1, 1, 2, 2, 8]
    assert [plan[n]["ragged"] for n in ns] == [True, True, False, True, True, False]
    assert plan[1]["below_block"] and plan[127]["below_block"] and not plan[128]["below_block"]
    assert SP.SATURATED_SHAPE == (3, 43) and SP.score_plan(129) == dict(blocks=2, ragged=True, below_block=False)


def test_dgab_table_reaches_every_branch():
    assert SP.DGAB_CASES == ((1, 8), (3, 24), (2, 64)) and SP.DGAB_TRIP == (67, 64)
    assert all(c % 8 == 0 for _, c in SP.DGAB_CASES) and {c for _, c in SP.DGAB_CASES} == {8, 24, 64}
    p = SP.dgab_plan(1, 8)
    assert p["wtiles"] == 4 and p["single_short_workgroup"] and p["idle_wavefronts"] and not p["second_trip"]
    p = SP.dgab_plan(3, 24)
    assert (p["wtiles"], p["workgroups"], p["idle_wavefronts"], p["second_trip"]) == (36, 5, True, False)
    p = SP.dgab_plan(2, 64)
    assert (p["wtiles"], p["workgroups"], p["idle_wavefronts"], p["second_trip"]) == (64, 8, False, False)
    # the N = 37 test of tests/test_gpu_dgab.py is a single trip for every chain kernel; (67, 64) is a second trip for all
    p, pb = SP.dgab_plan(37, 64), SP.dgab_plan(37, 64, bf16=True)
    assert (p["workgroups"], p["cap"], p["second_trip"]) == (148, 256, False)
    assert (pb["workgroups"], pb["cap"], pb["second_trip"]) == (296, 512, False)
    p, pb = SP.dgab_plan(*SP.DGAB_TRIP), SP.dgab_plan(*SP.DGAB_TRIP, bf16=True)
    assert (p["wtiles"], p["workgroups"], p["cap"], p["second_trip"]) == (2144, 268, 256, True)
    assert (pb["workgroups"], pb["cap"], pb["second_trip"]) == (536, 512, True)
    assert 64 * 64 == 4096 and not SP.dgab_plan(64, 64)["second_trip"] and SP.dgab_plan(65, 64)["second_trip"]
    for lo, hi in SP.DGAB_TRIP_SLICES:                 # the first image, the last one, and images on both sides of the wrap
        assert 0 <= lo < hi <= SP.DGAB_TRIP[0]
    wrap = 256 * 8 * 2 // 64                           # the image whose first tile opens the second trip (fp32, x3, and bf16)
    assert wrap == 512 * 4 * 2 // 64 == 64 and SP.DGAB_TRIP_SLICES[-1] == (66, 67) and SP.DGAB_TRIP_SLICES[0] == (0, 1)
    assert {(0, 1), (31, 34), (66, 67)} <= set(SP.DGAB_TRIP_SLICES)
    assert any(lo < wrap < hi - 1 for lo, hi in SP.DGAB_TRIP_SLICES)          # one slice holds images 63, 64 and 65
    assert SP.DGAB_KINDS == ("random", "constant-plane", "y-times-30")


def test_points_and_pool_tables_reach_every_branch():
    assert SP.POINTS_A_BATCHES == (1, 2, 3, 513, 515) and SP.POINTS_B_BATCHES == (1, 3, 5)
    plan = {n: SP.points_plan(n) for n in SP.POINTS_A_BATCHES}
    assert plan[1] == dict(pairs=1, second_trip=False, odd_tail=True)
    assert plan[2] == dict(pairs=1, second_trip=False, odd_tail=False)
    assert plan[513] == dict(pairs=257, second_trip=True, odd_tail=True)
    assert plan[515] == dict(pairs=258, second_trip=True, odd_tail=True)
    assert not SP.points_plan(512)["second_trip"]
    assert {(p["second_trip"], p["odd_tail"]) for p in plan.values()} >= {(False, False), (False, True), (True, True)}
    assert SP.AVGPOOL_SHAPES == ((1, 1, 1, 1), (1, 3, 1, 63), (2, 5, 5, 13), (3, 512, 1, 6))
    ap = [SP.avgpool_plan(*s) for s in SP.AVGPOOL_SHAPES]
    assert [p["plane_tail"] for p in ap] == [1, 3, 2, 0] and [p["hw"] for p in ap] == [1, 63, 65, 6]
    assert [p["below_wave"] for p in ap] == [True, True, False, True] and ap[2]["wave_tail"]
    assert SP.MAXPOOL_SHAPES == ((1, 1, 2, 2), (2, 3, 5, 7), (1, 5, 3, 2), (3, 64, 32, 100))
    assert any(h % 2 for _, _, h, _ in SP.MAXPOOL_SHAPES) and any(w % 2 for _, _, _, w in SP.MAXPOOL_SHAPES)
    assert any(n * c * (h // 2) * (w // 2) > 256 for n, c, h, w in SP.MAXPOOL_SHAPES)          # more than one workgroup
    assert any(n * c * (h // 2) * (w // 2) < 64 for n, c, h, w in SP.MAXPOOL_SHAPES)
    assert SP.LINEAR_BATCHES == (1, 3, 77) and SP.LINEAR_LAYERS == ((512, 256, True), (256, 40, False))
    assert SP.CBAM_BATCHES == (1, 2, 5) and len(SP.CBAM_KINDS) == 3


# ---- weights ---------------------------------------------------------------------------------------------------------------
def test_every_weight_and_bias_is_nonzero():
    for m in (SP.stage_module(), SP.int_module(), SP.saturated_module()):
        for name, p in m.named_parameters():
            assert bool((p != 0).all()) and bool(torch.isfinite(p).all()), name
    fresh = SP.TPS_PP()
    assert not fresh.TPE.localization_fc2.weight.any()                  # what a fresh module would have tested: the bias
    assert float(SP.stage_module().TPE.localization_fc2.weight.std()) > 0.05
    m = SP.int_module()
    for name in SP.FRONT_LAYERS:
        conv = getattr(m, name).conv
        assert _is_int(conv.weight) and _is_int(conv.bias)
        assert 1 <= float(conv.weight.abs().min()) and float(conv.weight.abs().max()) == SP.FRONT_A_W
        assert 1 <= float(conv.bias.abs().min()) and float(conv.bias.abs().max()) <= SP.FRONT_A_B
    for name in SP.POINT_LAYERS:
        lin = m.TPE.get_submodule(name)
        assert set(np.unique(lin.weight.numpy())) == {-1.0, 1.0} and set(np.unique(lin.bias.numpy())) <= {-1.0, 1.0}


# ---- the exact cases stay exact --------------------------------------------------------------------------------------------
def test_front_integer_cases_stay_below_2_24():
    layer1, grid = SP.front_a_bounds()
    assert layer1 == 64 * 8 + 4 and grid == 192 * 2 * layer1 + 4 and grid < SP.EXACT
    assert 32 * 8 + SP.FRONT_A_B <= layer1                              # down0 / down1 have 32 inputs, down2 has 64
    for N, H, W in SP.FRONT_A_CASES:
        k = SP.front_a_case(N, H, W)
        for n in ("o0", "o1", "x"):
            assert _is_int(k[n]) and np.abs(k[n]).max() == SP.FRONT_A_IN and k[n].min() < 0 < k[n].max()
        f0, f1, f2, fg = k["want"]
        assert f0.shape == f1.shape == fg.shape == (N, 64, H, W) and f2.shape == (N, 64, H // 2, W // 2)
        assert max(f0.max(), f1.max(), f2.max()) <= layer1 and fg.max() <= grid and min(a.min() for a in k["want"]) == 0
        for name, a in zip(SP.FRONT_NAMES, k["want"]):
            SP.spread(name, a, relu=True)
            assert np.array_equal(a.astype(np.float32).astype(np.int64), a)
        # the same maps from PyTorch's float64 composition of the integer module
        m = SP.copy.deepcopy(SP.int_module()).double()
        ref = SP.front_compose(m, *(torch.from_numpy(k[n]).double() for n in ("o0", "o1", "x")))
        for a, r in zip(k["want"], ref):
            assert np.array_equal(a, r.numpy())


def test_points_integer_cases_stay_below_2_24():
    b = SP.points_a_bounds()
    assert b["hidden"] == 129 and b["v"] == 256 * 129 + 1 and b["ctrl"] == 64 * (256 * 129 + 1) + 1 and b["p"] == 32 * 129 + 1
    assert max(b.values()) < SP.EXACT
    tpe = SP.copy.deepcopy(SP.int_module()).double().TPE
    for N in SP.POINTS_A_BATCHES:
        k = SP.points_a_case(N)
        assert _is_int(k["en"]) and np.abs(k["en"]).max() == SP.POINTS_A_IN
        ctrl, p = k["want"]
        assert ctrl.shape == (N, 32, 2) and p.shape == (N, 32, 128)
        assert np.abs(k["hidden"]).max() <= b["hidden"] and np.abs(k["v"]).max() <= b["v"]
        assert np.abs(ctrl).max() <= b["ctrl"] and np.abs(k["t1"]).max() <= b["t1"] and np.abs(p).max() <= b["p"]
        # neither ReLU layer is dead or wide open, and ctrl is not its bias
        assert 0.2 < (k["hidden"] > 0).mean() < 0.8 and 0.2 < (k["v"] > 0).mean() < 0.8
        SP.spread("ctrl", ctrl)
        SP.spread("p", p)
        assert float(np.std(ctrl - tpe.localization_fc2.bias.numpy().reshape(1, 32, 2))) > 10
        rc, rp = SP.points_compose(tpe, torch.from_numpy(k["en"]).double())
        assert np.array_equal(ctrl, rc.numpy()) and np.array_equal(p, rp.numpy())


def test_max_pool_reference_follows_the_nan_rule():
    """F.max_pool2d on the CPU propagates a NaN from any of the four positions with its bits, uses floor mode, and so never
    sees the NaN in the dropped row or column: what tpspp_pool.hip states."""
    quiet_nan = np.float32(np.nan).view(np.int32)
    for shape in SP.MAXPOOL_SHAPES[:3]:
        N, C, H, W = shape
        x = SP.maxpool_case(shape, "negative-and-inf")
        y = F.max_pool2d(torch.from_numpy(x), 2, 2).numpy()
        assert y.shape == (N, C, H // 2, W // 2) and not np.isnan(y).any()
        assert y[0, 0].max() < 0 and np.isneginf(x).any()
        if W >= 4:
            assert np.isneginf(y[0, 0, 0, 1])
        for variant in SP.MAXPOOL_VARIANTS[1:]:
            x = SP.maxpool_case(shape, variant)
            y = F.max_pool2d(torch.from_numpy(x), 2, 2).numpy()
            nan = np.isnan(y)
            assert nan[:, :, -1, -1].all() and nan.sum() == N * C                 # the last window of every plane, alone
            assert (y.view(np.int32)[nan] == quiet_nan).all()
            assert np.isnan(x).sum() == N * C * (1 + (W if H % 2 else 0) + (H if W % 2 else 0) - (1 if H % 2 and W % 2 else 0))
            # the rule of the kernel, in NumPy
            a, b, c, d = (x[:, :, i:2 * (H // 2):2, j:2 * (W // 2):2] for i in (0, 1) for j in (0, 1))
            m = a.copy()
            for v in (b, c, d):
                m = np.where((v > m) | np.isnan(v), v, m)
            assert np.array_equal(m.view(np.int32), y.view(np.int32))


# ---- the float64 builders, written a second way ----------------------------------------------------------------------------
def _sd64():
    return {k: v for k, v in SP.stage_module64().state_dict().items()}


def test_front_builder_is_the_pointwise_formula():
    m = SP.stage_module64()
    w = {n: (getattr(m, n).conv.weight.view(64, -1), getattr(m, n).conv.bias) for n in SP.FRONT_LAYERS}
    for N, H, W in SP.FRONT_CASES[:5]:
        k = SP.front_case(N, H, W)
        o0, o1, x = (k[n].double() for n in ("o0", "o1", "x"))
        assert o0.min() < 0 < o0.max() and x.min() < 0 < x.max()                 # signed inputs

        def pw(name, t):
            return torch.relu(torch.einsum("oc,nchw->nohw", w[name][0], t) + w[name][1][None, :, None, None])
        f0, f1, f2 = pw("down0", o0), pw("down1", o1), pw("down2", x)
        up = f2[:, :, torch.arange(H) // 2][:, :, :, torch.arange(W) // 2]                  # the parent pixel, by index
        fg = pw("down_feat", torch.cat([f0, f1, up], 1))
        for name, a, b in zip(SP.FRONT_NAMES, k["want"], (f0, f1, f2, fg)):
            assert a.dtype == torch.float64 and close(a, b), name
            SP.spread(name, a, relu=True)


def test_down_fused_builder_is_conv_of_conv():
    sd = _sd64()
    for N, H in SP.DOWN_FUSED_CASES:
        k = SP.down_fused_case(N, H)
        assert k["o"].min() < 0 < k["o"].max()
        for i in (0, 1):
            mid = TO.conv_module(sd, f"down{i}", k["o"].double())
            want = TO.conv_module(sd, f"down{i}_1", mid, stride=2, padding=1)
            assert k["want"][i].shape == (N, 64, H // 2, 64) and close(k["want"][i], want)
            SP.spread(f"down{i}_1", want, relu=True)
        assert float(SP.stage_module().down0_1.conv.bias.abs().min()) > 0


def test_cbam_builder_and_its_special_images():
    sd = _sd64()
    for N in SP.CBAM_BATCHES:
        for kind in SP.CBAM_KINDS:
            k = SP.cbam_case(N, kind)
            x = k["x"]
            assert close(k["want"], TO.cbam(sd, "MSFA.conv.atten", x.double()))
            SP.spread(f"cbam {kind}", k["want"])
            last = x[N - 1].view(64, 32)
            if kind == "signed":
                assert bool(((last > 0).any(1) & (last < 0).any(1)).all())
            elif kind == "one-image-negative":
                assert float(last.max()) < 0                   # a channel max that starts from 0 would be wrong here
            else:
                assert bool(((last > 0).sum(1) == 1).all()) and float((last.max(1).values - last.mean(1)).min()) > 1.0
            # the shared MLP's ReLU is neither dead nor open for the batch: some hidden unit on each side of 0
            w0 = SP.stage_module64().MSFA.conv.atten.channel_attention.shared_MLP[0].weight.view(4, 64)
            pre = torch.cat([x.double().mean((2, 3)) @ w0.t(), x.double().amax((2, 3)) @ w0.t()])
            assert float(pre.max()) > 0 > float(pre.min())


def test_points_builder_is_linear_relu_linear():
    sd = _sd64()
    for N in SP.POINTS_B_BATCHES:
        k = SP.points_case(N)
        en = k["en"].double().flatten(2).transpose(1, 2)
        f1 = F.relu(F.linear(en, sd["TPE.localization_fc1.0.weight"], sd["TPE.localization_fc1.0.bias"]))
        f1 = F.relu(F.linear(f1, sd["TPE.localization_fc1.2.weight"], sd["TPE.localization_fc1.2.bias"]))
        assert 0.1 < float((f1 > 0).double().mean()) < 0.9
        ctrl = F.linear(f1.reshape(N, -1), sd["TPE.localization_fc2.weight"], sd["TPE.localization_fc2.bias"]).view(N, 32, 2)
        p = F.linear(F.linear(en, sd["TPE.p_linear.0.weight"], sd["TPE.p_linear.0.bias"]),
                     sd["TPE.p_linear.1.weight"], sd["TPE.p_linear.1.bias"])
        assert close(k["want"][0], ctrl) and close(k["want"][1], p)
        assert float((ctrl - sd["TPE.localization_fc2.bias"].view(1, 32, 2)).abs().max()) > 0.05      # not the bias
        SP.spread("ctrl", ctrl)
        SP.spread("p", p)


def test_score_builder_and_saturation():
    sd = _sd64()
    for H, W in SP.SCORE_SHAPES:
        k = SP.score_case(H, W)
        de, en = k["de"].double(), k["en"].double()
        feat = de.reshape(SP.SCORE_N, 64, H * W)
        f = torch.einsum("oc,bcn->bno", sd["TPE.feat_linear.0.weight"], feat) + sd["TPE.feat_linear.0.bias"]
        f = f @ sd["TPE.feat_linear.1.weight"].t() + sd["TPE.feat_linear.1.bias"]
        p = (en @ sd["TPE.p_linear.0.weight"].t() + sd["TPE.p_linear.0.bias"]) @ sd["TPE.p_linear.1.weight"].t() \
            + sd["TPE.p_linear.1.bias"]
        want = torch.tanh(torch.einsum("bnc,bmc->bnm", f, p) * 64 ** -0.5)
        assert k["want"].shape == (SP.SCORE_N, H * W, 32) and close(k["want"], want)
        SP.spread("score", want)
    k = SP.saturated_case()
    assert SP.SATURATED_TARGET / 2 ** 0.5 <= k["top"] <= SP.SATURATED_TARGET * 2 ** 0.5
    w32 = k["want"].float()
    assert bool((w32.abs() == 1.0).any()) and float(k["want"].abs().max()) <= 1.0          # some tanh round to +-1 in fp32
    assert float((k["want"].abs() > 0.99).double().mean()) > 0.2
    # at that scale the split's format bound is above the workload's absolute tolerance
    assert SP.X3_SPLIT_BOUND == 3 * 2.0 ** -16 and float(k["x3_bound"].max()) > SP.SCORE_X3_TOL
    assert k["x3_bound"].shape == k["want"].shape
    ratio = SP.saturated_module().TPE.p_linear[1].weight / SP.stage_module().TPE.p_linear[1].weight
    assert float(ratio.min()) == float(ratio.max()) and float(np.log2(float(ratio[0, 0]))).is_integer()


def test_dgab_builder_special_inputs_and_fp32_composition():
    """The float64 builder is the oracle's restatement in double; each special input is finite there and PyTorch's fp32
    composition stays within 1e-4 of it; y-times-30 gives logits beyond the overflow threshold of expf in both softmaxes,
    constant-plane gives LayerNorm 1 a variance of exactly 0."""
    sd = _sd64()
    blk32, blk64 = SP.stage_module().TPE.atten[0], SP.stage_module64().TPE.atten[0]
    for N, C in SP.DGAB_CASES:
        for kind in SP.DGAB_KINDS:
            k = SP.dgab_case(N, C, kind)
            x, y = k["x"], k["y"]
            assert k["want"].dtype == torch.float64 and torch.isfinite(k["want"]).all()
            assert close(k["want"], TO.dgab(sd, "TPE.atten.0", x.double(), y.double().transpose(1, 2)), 1e-10)
            SP.spread(f"dgab {kind}", k["want"])
            e32 = SP.rel(blk32(x, y.transpose(1, 2)), k["want"])
            print(f"dgab ({N}, {C}) {kind}: PyTorch fp32 on the CPU is {e32:.3e} from float64")
            assert e32 <= SP.DGAB_LIB32_LIMIT
            xn = blk64.norm1(x.double())
            w = blk64.attn.mlp_w[0](torch.cat([xn.mean(2), y.double()], 2))[:, :, :-1]
            h = blk64.attn.mlp_h[0](torch.cat([xn.mean(3), y.double()], 2))[:, :, :-1]
            if kind == "y-times-30":
                assert float(w.max()) > 89 and float(h.max()) > 89
                with np.errstate(over="ignore"):
                    assert np.isinf(np.exp(np.float32(w.max()))) and np.isinf(np.exp(np.float32(h.max())))
            else:
                assert float(w.abs().max()) < 40 and float(h.abs().max()) < 40
            if kind == "constant-plane":
                assert float(x[0, 1].var()) == 0 and float(x[0, 1, 0, 0]) == 3.0
                assert torch.equal(xn[0, 1], blk64.norm1.bias)                   # (x - mean) is exactly 0
            # the gated map stays of order one, so the x3 variant's absolute tolerance means what it means at the workload
            assert float(k["want"].abs().max()) < 100


def test_pool_and_linear_builders():
    for shape in SP.AVGPOOL_SHAPES:
        k = SP.avgpool_case(shape)
        assert close(k["want"], F.adaptive_avg_pool2d(k["x"].double(), 1).flatten(1)) and k["want"].shape == shape[:2]
        SP.spread("global_avgpool", k["want"])
    for N in SP.LINEAR_BATCHES:
        for cin, cout, relu in SP.LINEAR_LAYERS:
            k = SP.linear_case(N, cin, cout, relu)
            z = k["x"].double() @ k["w"].double().t() + k["b"].double()
            assert close(k["want"], z.clamp_min(0) if relu else z) and k["want"].shape == (N, cout)
            assert bool((k["w"] != 0).all() and (k["b"] != 0).all())
            SP.spread("linear", k["want"], relu=relu)


# ---- the refusals that return before a launch ---------------------------------------------------------------------------------
def test_entry_points_refuse_bad_sizes_before_any_launch(lib):
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rc, text):
        assert rc == EINVAL and text in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())

    def front(N, H, W):
        return lib.tpspp_front_fwd(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, N, H, W, None)
    refused(front(1, 3, 4), b"need even H, W")
    refused(front(1, 4, 3), b"need even H, W")
    refused(front(65536, 2, 2), b"need even H, W")
    refused(lib.tpspp_score_fwd(p, p, p, p, p, p, 0.125, p, 1, 0, None), b"tpspp_score_fwd: bad sizes")
    refused(lib.tpspp_score_fwd(p, p, p, p, p, p, 0.125, p, 65536, 4, None), b"tpspp_score_fwd: bad sizes")
    refused(lib.tpspp_score_x3_fwd(p, p, p, p, p, p, 0.125, p, 1, 0, None), b"tpspp_score_x3_fwd: bad sizes")
    refused(lib.tpspp_maxpool2x2_fwd(p, 1, 1, 1, 4, p, None), b"tpspp_maxpool2x2_fwd: bad sizes")
    refused(lib.tpspp_dgab_fwd(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 1, 12, None), b"multiple of 8")
    refused(lib.tpspp_dgab_bf16_fwd(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 1, 12, 0, None), b"multiple of 8")
