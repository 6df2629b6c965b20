"""-m gpu: the "hip_all" train backend -- DGAB, the score, CBAM and the localization FCs forward and backward on the HIP
kernels of tpspp_regressor_bwd.hip -- block by block and as a whole TPS_PP / NRTR training step, against float64 PyTorch on
the CPU.

Per-block bar: relative L2 <= max(1e-5, 2 x the relative L2 of PyTorch's fp32 composition of the same block on the same
inputs, run on the GPU as the "torch" train backend runs it), both measured against the float64 composition on the CPU;
every output gradient (inputs and parameters) is checked."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
from freeze_patterns import check_freeze_patterns
from tps_pp_amd import TPS_PP, ops

pytestmark = pytest.mark.gpu


def synth_module(variant):
    m = TPS_PP(variant=variant)
    sd = cases.synth_state(m.state_dict(), 4, cases.tpspp_state_rule, cases.TPSPP_KEEP)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


def rel(got, want):
    want = want.double()
    n = want.norm()
    d = (got.detach().cpu().double() - want).norm()
    return (d / n).item() if n > 0 else d.item()


# ---- float64 / fp32 compositions of each block with the module's own layers --------------------------------------------
def _dgab_ref(blk, x, y):
    return blk(x, y.transpose(1, 2))                         # y (N, C, T) -> the (b t c) tokens DGAB takes


def _score_ref(tpe, de, en):
    n, c = en.shape[:2]
    return tpe.get_score(en.reshape(n, c, -1).transpose(1, 2), de).transpose(1, 2)     # the (N, F, n) buffer


def _points_ref(tpe, en):
    n, c = en.shape[:2]
    tok = en.reshape(n, c, -1).transpose(1, 2)
    return tpe.localization_fc2(tpe.localization_fc1(tok).reshape(n, -1)).view(n, tpe.num_fiducial, 2)


def _cbam_ref(mod, x):
    return mod(x)


REFS = {"dgab": _dgab_ref, "score": _score_ref, "points": _points_ref, "cbam": _cbam_ref}


def reference_grads(kind, mod, inputs, gout, dtype, device="cpu"):
    """(input grads, {param name: grad}) of the PyTorch composition of `mod` in `dtype` on `device`."""
    m = copy.deepcopy(mod).to(device).to(dtype)
    for p in m.parameters():
        p.grad = None
        p.requires_grad_(True)
    xs = [t.detach().to(device).to(dtype).requires_grad_(True) for t in inputs]
    out = REFS[kind](m, *xs)
    out.backward(gout.detach().to(device).to(dtype))
    return [t.grad.cpu() for t in xs], {k: p.grad.cpu() for k, p in m.named_parameters()}


def check_block(kind, mod, inputs, gout, got_inputs, got_params, label=""):
    """Every gradient of the block against float64 (CPU), within max(1e-5, 2 x the error of PyTorch's fp32 composition
    on the GPU -- what the "torch" train backend runs)."""
    gi64, gp64 = reference_grads(kind, mod, inputs, gout, torch.float64)
    gi32, gp32 = reference_grads(kind, mod, inputs, gout, torch.float32, "cuda")
    bad = {}
    names = [f"input{i}" for i in range(len(inputs))] + list(gp64)
    got = list(got_inputs) + [got_params[k] for k in gp64]
    want = list(gi64) + [gp64[k] for k in gp64]
    lib32 = list(gi32) + [gp32[k] for k in gp64]
    for name, g, w, t in zip(names, got, want, lib32):
        if w is None:
            continue
        assert g is not None, f"{kind}{label}: no gradient for {name}"
        assert torch.isfinite(g).all(), f"{kind}{label}: {name} not finite"
        if w.norm() == 0:
            assert g.abs().max() == 0, f"{kind}{label}: {name} should be zero"
            continue
        bar = max(1e-5, 2 * rel(t, w))
        e = rel(g, w)
        if e > bar:
            bad[name] = (e, bar)
    assert not bad, f"{kind}{label}: {bad}"


# ---- 1. per block, as seen inside a real training step ------------------------------------------------------------------
def head_grads():
    g = torch.Generator().manual_seed(17)
    return (torch.randn((cases.G4_N, 64, 16, 64), generator=g), torch.randn((cases.G4_N, 64, 16, 64), generator=g))


def module_step(cuda, variant, mode="hip_all", m=None):
    g0, g1 = head_grads()
    m = (m or synth_module(variant)).to(cuda).train().set_train_backend(mode)
    inp = cases.g4_inputs(variant)
    x = torch.from_numpy(inp["x"]).to(cuda).requires_grad_(True)
    outs = [torch.from_numpy(o).to(cuda).requires_grad_(True) for o in inp["outs"]]
    res = m(x, outs)
    ((res["output"] * g0.to(cuda)).sum() + (res["mp_img"] * g1.to(cuda)).sum()).backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads.update({"x": x.grad, "outs[0]": outs[0].grad, "outs[1]": outs[1].grad})
    return m, x.detach(), [o.detach() for o in outs], res, grads


def install_spies(monkeypatch):
    recs = []

    def wrap(kind, real, nin):
        def spy(*args):
            views = [a.view_as(a) for a in args[:nin]]
            out = real(*views, *args[nin:])
            r = dict(kind=kind, mod=args[nin], inputs=[v.detach().clone() for v in views], gout=None,
                     gin=[None] * nin)
            out.register_hook(lambda g: r.__setitem__("gout", g.detach().clone()))
            for i, v in enumerate(views):
                if v.requires_grad:
                    v.register_hook(lambda g, i=i: r["gin"].__setitem__(i, g.detach().clone()))
            recs.append(r)
            return out
        return spy

    monkeypatch.setattr(ops, "dgab_autograd", wrap("dgab", ops.dgab_autograd, 2))
    monkeypatch.setattr(ops, "score_autograd", wrap("score", ops.score_autograd, 2))
    monkeypatch.setattr(ops, "cbam_autograd", wrap("cbam", ops.cbam_autograd, 1))
    monkeypatch.setattr(ops, "tpe_points_autograd", wrap("points", ops.tpe_points_autograd, 1))
    return recs


@pytest.mark.parametrize("variant", ["ResNet45v2", "ResNet45"])
def test_blocks_inside_a_training_step_against_float64(cuda, variant, monkeypatch):
    recs = install_spies(monkeypatch)
    m, *_ = module_step(cuda, variant)
    torch.cuda.synchronize()
    assert sorted(r["kind"] for r in recs) == ["cbam", "dgab", "points", "score"]
    for r in recs:
        mod = r["mod"]
        got_params = {k: p.grad for k, p in mod.named_parameters()}
        if r["kind"] in ("score", "points"):
            # TPE is shared by the score, the points and DGAB: compare the parameters this block owns
            own = ("feat_linear", "p_linear") if r["kind"] == "score" else ("localization_fc",)
            mod = FilteredTPE(mod, own)
            got_params = {k: p.grad for k, p in mod.named_parameters()}
        check_block(r["kind"], mod, r["inputs"], r["gout"], r["gin"], got_params, f" ({variant})")


class FilteredTPE(nn.Module):
    """A view of Transformation_Parameter_Estimation whose named_parameters() are only those of the listed children."""

    def __init__(self, tpe, own):
        super().__init__()
        self.tpe = tpe
        self.own = own

    def named_parameters(self, *a, **k):
        return [(n, p) for n, p in self.tpe.named_parameters() if n.startswith(self.own)]

    def __deepcopy__(self, memo):
        return FilteredTPE(copy.deepcopy(self.tpe, memo), self.own)

    def to(self, *a, **k):
        self.tpe.to(*a, **k)
        return self

    def cpu(self):
        self.tpe.cpu()
        return self

    def parameters(self):
        return [p for _, p in self.named_parameters()]

    def get_score(self, *a):
        return self.tpe.get_score(*a)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.tpe, name)


# ---- 1b. the blocks on their own: ragged batches and edge cases ----------------------------------------------------------
def run_block(cuda, kind, mod, inputs, seed=0):
    """HIP gradients of one block for random incoming gradients: (gout, input grads, param grads)."""
    mod = mod.to(cuda)
    for p in mod.parameters():
        p.grad = None
    xs = [t.to(cuda).requires_grad_(True) for t in inputs]
    if kind == "dgab":
        out = ops.dgab_autograd(xs[0], xs[1], mod)
    elif kind == "score":
        out = ops.score_autograd(xs[0], xs[1], mod)
    elif kind == "cbam":
        out = ops.cbam_autograd(xs[0], mod)
    else:
        out = ops.tpe_points_autograd(xs[0], mod)
    g = torch.Generator().manual_seed(100 + seed)
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout.to(cuda))
    torch.cuda.synchronize()
    return gout, [t.grad for t in xs], {k: p.grad for k, p in mod.named_parameters()}


def block_inputs(kind, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "dgab":
        return [torch.randn((N, 64, 16, 64), generator=g), torch.randn((N, 64, 32), generator=g)]
    if kind == "score":
        return [torch.randn((N, 64, 16, 64), generator=g), torch.randn((N, 64, 2, 16), generator=g)]
    return [torch.randn((N, 64, 2, 16), generator=g).abs()]


def block_module(kind, variant="ResNet45v2"):
    m = synth_module(variant)
    if kind == "dgab":
        return m.TPE.atten[0]
    if kind == "cbam":
        return m.MSFA.conv.atten
    own = ("feat_linear", "p_linear") if kind == "score" else ("localization_fc",)
    return FilteredTPE(m.TPE, own)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("kind", ["dgab", "score", "cbam", "points"])
def test_block_ragged_batches(cuda, kind, N):
    mod = block_module(kind)
    inputs = block_inputs(kind, N, seed=N)
    gout, gin, gp = run_block(cuda, kind, mod, inputs, seed=N)
    check_block(kind, mod, inputs, gout, gin, gp, f" N={N}")


def test_dgab_constant_plane(cuda):
    """One (n, c) plane of x constant: norm1's variance is 0 there (rstd = 1 / sqrt(eps))."""
    mod = block_module("dgab")
    x, y = block_inputs("dgab", 3, seed=5)
    x[1, 7] = 0.25
    gout, gin, gp = run_block(cuda, "dgab", mod, [x, y], seed=5)
    check_block("dgab", mod, [x, y], gout, gin, gp, " constant plane")


def test_score_saturated_tanh(cuda):
    """Inputs scaled so that most of the score's tanh arguments are far in saturation."""
    mod = block_module("score")
    de, en = block_inputs("score", 2, seed=6)
    de, en = de * 30.0, en * 30.0
    gout, gin, gp = run_block(cuda, "score", mod, [de, en], seed=6)
    with torch.no_grad():
        s = ops.score_autograd(de.to(cuda), en.to(cuda), mod)
    assert (s.abs() > 0.999).float().mean() > 0.5
    check_block("score", mod, [de, en], gout, gin, gp, " saturated")


# ---- 2. whole module ------------------------------------------------------------------------------------------------------
GROUP_BARS = [
    (lambda k: k.startswith("MSFA.conv.atten."), 2e-2),
    (lambda k: k.startswith("MSFA.conv.k_decoder."), 3e-3),
    (lambda k: k.startswith("TPE.") and not k.startswith("TPE.localization_"), 6e-3),
    (lambda k: True, 3e-4),          # down*, k_encoder.*, TPE.localization_*, x, outs
]


def group_bar(name):
    return next(b for match, b in GROUP_BARS if match(name))


def grid64(at, ctrl, score):
    N, n, _ = score.shape
    P = torch.from_numpy(np.asarray(at.P)).to(score.dtype)[None].expand(N, -1, -1)
    ph = at.P_hat[None] * (score * at.thela + 1)
    ph = torch.cat([torch.ones((N, n, 1), dtype=score.dtype), P, ph], dim=2)
    T = torch.bmm(at.hat_C[None].expand(N, -1, -1), torch.cat([ctrl, torch.zeros((N, 3, 2), dtype=ctrl.dtype)], 1))
    return torch.bmm(ph, T)


def forward64(m64, x, outs, hw):
    cp, sc, fg = m64._regress_torch(x, outs)
    g = grid64(m64.atten_tps, cp, sc).reshape(x.shape[0], hw[0], hw[1], 2)
    o0 = F.grid_sample(fg, g, padding_mode="border", align_corners=True)
    o1 = F.grid_sample(x, g, padding_mode="border", align_corners=True)
    return o0, o1


@pytest.mark.parametrize("variant", ["ResNet45v2", "ResNet45"])
def test_module_gradients_against_float64(cuda, variant):
    g0, g1 = head_grads()
    m, x, outs, res, gh = module_step(cuda, variant)
    m64 = synth_module(variant).double().train()
    inp = cases.g4_inputs(variant)
    x64 = torch.from_numpy(inp["x"]).double().requires_grad_(True)
    outs64 = [torch.from_numpy(o).double().requires_grad_(True) for o in inp["outs"]]
    o0, o1 = forward64(m64, x64, outs64, m.rectified_img_size)
    ((o0 * g0.double()).sum() + (o1 * g1.double()).sum()).backward()
    g64 = {k: p.grad for k, p in m64.named_parameters()}
    g64.update({"x": x64.grad, "outs[0]": outs64[0].grad, "outs[1]": outs64[1].grad})
    bad = {}
    for k, want in g64.items():
        assert gh[k] is not None and torch.isfinite(gh[k]).all(), k
        if want.norm() == 0:
            continue
        e = rel(gh[k], want)
        if e > group_bar(k):
            bad[k] = (e, group_bar(k))
    assert not bad, bad
    with torch.no_grad():
        ref = m.eval()(x, outs)
    assert (ref["output"] - res["output"].detach()).abs().max() <= 1e-4
    assert (ref["mp_img"] - res["mp_img"].detach()).abs().max() <= 1e-4


# ---- 3. no library layer runs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["ResNet45v2", "ResNet45"])
def test_no_library_layer_runs(cuda, variant, monkeypatch):
    m = synth_module(variant).to(cuda)

    def refuse(self, *a, **k):
        raise AssertionError(f"{type(self).__name__}.forward ran in the hip_all training graph")

    for cls in (nn.Linear, nn.LayerNorm, nn.GELU, nn.Conv2d, nn.Sigmoid, nn.AdaptiveAvgPool2d, nn.AdaptiveMaxPool2d,
                nn.ReLU, nn.Upsample):
        monkeypatch.setattr(cls, "forward", refuse)
    _, _, _, res, grads = module_step(cuda, variant, m=m)
    assert torch.isfinite(res["output"]).all()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


# ---- 4. reproducible -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dgab", "score", "cbam", "points"])
def test_bitwise_reproducible_across_calls_and_streams(cuda, kind):
    mod = block_module(kind).to(cuda)
    inputs = [t.to(cuda).requires_grad_(True) for t in block_inputs(kind, 3, seed=9)]
    params = [p for p in mod.parameters()]
    fn = {"dgab": ops.dgab_autograd, "score": ops.score_autograd, "cbam": ops.cbam_autograd,
          "points": ops.tpe_points_autograd}[kind]

    def grads():
        out = fn(*inputs, mod)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(cuda)
        return [g.clone() for g in torch.autograd.grad(out, inputs + params, gout)]

    a = grads()
    b = grads()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = grads()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ---- 5. frozen layers ----------------------------------------------------------------------------------------------------
def test_frozen_dgab_gives_input_gradients_only(cuda):
    mod = block_module("dgab").to(cuda)
    for p in mod.parameters():
        p.requires_grad_(False)
    inputs = block_inputs("dgab", 3, seed=11)
    gout, gin, gp = run_block(cuda, "dgab", mod, inputs, seed=11)
    assert all(p.grad is None for p in mod.parameters())
    gi64, _ = reference_grads("dgab", mod, inputs, gout, torch.float64)
    gi32, _ = reference_grads("dgab", mod, inputs, gout, torch.float32, "cuda")
    for g, w, t in zip(gin, gi64, gi32):
        assert g is not None and rel(g, w) <= max(1e-5, 2 * rel(t, w))


@pytest.mark.parametrize("kind", ["dgab", "score", "points"])
def test_freeze_patterns_return_none_and_keep_the_bits(cuda, kind, monkeypatch):
    fn_cls, fn, last = {"dgab": (ops._DgabFunction, ops.dgab_autograd, "mlp.fc2."),
                        "score": (ops._ScoreFunction, ops.score_autograd, "p_linear.1."),
                        "points": (ops._TpePointsFunction, ops.tpe_points_autograd, "localization_fc2.")}[kind]
    mod = block_module(kind).to(cuda)
    inputs = [t.to(cuda) for t in block_inputs(kind, 3, seed=12)]
    check_freeze_patterns(monkeypatch, fn_cls, lambda *xs: fn(*xs, mod), inputs, dict(mod.named_parameters()), last)


# ---- 6. training tracks torch --------------------------------------------------------------------------------------------
def test_sgd_steps_track_the_torch_backend(cuda):
    inp = cases.g4_inputs("ResNet45v2")
    x = torch.from_numpy(inp["x"]).to(cuda)
    outs = [torch.from_numpy(o).to(cuda) for o in inp["outs"]]
    losses = {}
    for mode in ("torch", "hip_all"):
        m = synth_module("ResNet45v2").to(cuda).train().set_train_backend(mode)
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        seq = []
        for _ in range(3):
            opt.zero_grad()
            res = m(x, outs)
            loss = res["output"].square().mean() + res["mp_img"].square().mean()
            loss.backward()
            opt.step()
            seq.append(loss.item())
        losses[mode] = seq
    t, h = np.array(losses["torch"]), np.array(losses["hip_all"])
    assert np.all(np.abs(h - t) <= 1e-3 * np.abs(t)), losses
    assert t[-1] != t[0]


# ---- 7. recogniser -------------------------------------------------------------------------------------------------------
def test_nrtr_forward_train_with_hip_all(cuda):
    import tps_pp_amd as P
    torch.manual_seed(0)
    m = P.build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                         strides=[2, 1, 2, 1, 2]),
                              tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                              decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                              label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
                              max_seq_len=8))
    m = m.to(cuda).train().set_train_backend("hip_all")
    assert m.tpsnet.train_backend == "hip_all"
    img = torch.randn((2, 3, 32, 128), device=cuda)
    metas = [dict(resize_shape=(32, 128, 3), text="ab"), dict(resize_shape=(32, 100, 3), text="tps")]
    losses = m.forward_train(img, metas)
    loss = sum(v.mean() for v in losses.values())
    loss.backward()
    for k, p in m.tpsnet.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    for k, p in m.tpsnet.named_parameters():
        if k.startswith(("TPE.atten.", "TPE.feat_linear.", "TPE.p_linear.")):
            assert p.grad.abs().max() > 0, k
