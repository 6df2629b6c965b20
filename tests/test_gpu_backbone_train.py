"""-m gpu: the backbone's "hip" train backend -- ResNetABI_v2_large's stem and BasicBlocks forward and backward on the
convolution kernels and the BatchNorm training kernels of tpspp_bn_train.hip -- kernel by kernel, block by block inside a
real training step, and as a whole backbone, against float64 PyTorch on the CPU.

Bar: relative L2 <= max(1e-5, 2 x the relative L2 of PyTorch's fp32 composition of the same thing on the same inputs, run
on the GPU as the "torch" train backend runs it), both measured against the float64 composition on the CPU."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tps_pp_amd import ResNetABI_v2_large, ops

pytestmark = pytest.mark.gpu


def rel(got, want):
    want = want.double().cpu()
    n = want.norm()
    d = (got.detach().cpu().double() - want).norm()
    return (d / n).item() if n > 0 else d.item()


def bar(lib32, want):
    return max(1e-5, 2 * rel(lib32, want))


def randomize_bn(m, seed):
    """Non-trivial affine parameters and running statistics for every BatchNorm of `m`."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in m.modules():
            if isinstance(bn, nn.BatchNorm2d):
                c = bn.num_features
                bn.weight.copy_(1 + 0.3 * torch.randn(c, generator=g))
                bn.bias.copy_(0.2 * torch.randn(c, generator=g))
                bn.running_mean.copy_(0.1 * torch.randn(c, generator=g))
                bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
                bn.num_batches_tracked.fill_(3)
    return m


def backbone(arch=(1, 1, 1, 1, 1), seed=0):
    torch.manual_seed(seed)
    return randomize_bn(ResNetABI_v2_large(arch_settings=list(arch), strides=[2, 1, 2, 1, 2]), seed + 100)


def check(label, got, want, lib32):
    """{name: tensor} dicts; every entry of `want` within the bar."""
    bad = {}
    for k, w in want.items():
        g = got[k]
        assert g is not None, f"{label}: no value for {k}"
        assert torch.isfinite(g).all(), f"{label}: {k} not finite"
        e, b = rel(g, w), bar(lib32[k], w)
        if e > b:
            bad[k] = (e, b)
    assert not bad, f"{label}: {bad}"


# ---- 1. the BatchNorm kernels alone --------------------------------------------------------------------------------------
def bn_inputs(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    za = 1.5 * torch.randn((N, C, H, W), generator=g) + 0.3
    zb = torch.randn((N, C, H, W), generator=g) - 0.2
    za[:, 0] = 0.75                                                  # a constant channel: variance 0
    za[:, 1] = 1e3 + torch.randn((N, H, W), generator=g)            # large mean, unit spread: E[z^2] - E[z]^2 cancels
    gy = torch.randn((N, C, H, W), generator=g)
    return za, zb, gy


def bn_ref(za, zb, gy, bns, mode, dtype, device, relu=True):
    """relu(bn_a(za) + r) with PyTorch's layers; returns (y, grads, buffers)."""
    bns = [copy.deepcopy(b).to(device).to(dtype) for b in bns]
    za = za.to(device).to(dtype).requires_grad_(True)
    zb = zb.to(device).to(dtype).requires_grad_(True)
    out = bns[0](za)
    if mode == "residual":
        out = out + zb
    elif mode == "branch":
        out = out + bns[1](zb)
    y = F.relu(out) if relu else out
    y.backward(gy.to(device).to(dtype))
    grads = {"za": za.grad, "ga": bns[0].weight.grad, "ba": bns[0].bias.grad}
    if mode != "none":
        grads["zb"] = zb.grad
    if mode == "branch":
        grads.update(gb=bns[1].weight.grad, bb=bns[1].bias.grad)
    bufs = {f"{i}.{k}": v for i, b in enumerate(bns) for k, v in (("rm", b.running_mean), ("rv", b.running_var))}
    return y.detach(), {k: v.cpu() for k, v in grads.items()}, {k: v.cpu() for k, v in bufs.items()}


def bn_hip(za, zb, gy, bns, mode, cuda, relu=True):
    """The same on the HIP kernels through the ops wrappers."""
    bns = [copy.deepcopy(b).to(cuda) for b in bns]
    za, zb, gy = za.to(cuda), zb.to(cuda), gy.to(cuda)

    def stats(b, z):
        if b.training:
            return ops.bn_train_stats(z, b.eps, b.momentum, b.running_mean, b.running_var, b.num_batches_tracked)
        return ops.bn_eval_stats(b.running_mean, b.running_var, b.eps)

    a = bns[0]
    sa = stats(a, za)
    kw = {}
    if mode == "residual":
        kw = dict(residual=zb)
    elif mode == "branch":
        sb = stats(bns[1], zb)
        kw = dict(zb=zb, stats_b=sb, gamma_b=bns[1].weight, beta_b=bns[1].bias)
    y = ops.bn_apply(za, sa, a.weight, a.bias, relu=relu, **kw)
    two = mode == "branch"
    sums = ops.bn_bwd_reduce(gy, y, za, sa, zb if two else None, sb if two else None, relu=relu)
    dres = torch.empty_like(gy) if mode == "residual" else None
    dza, dzb = ops.bn_bwd_data(gy, y, za, sa, a.weight, sums, a.training, zb=zb if two else None,
                               stats_b=sb if two else None, gamma_b=bns[1].weight if two else None,
                               train_b=bns[1].training if two else True, relu=relu, dres=dres,
                               dres_mode=1 if mode == "residual" else 0)
    grads = {"za": dza, "ga": sums[1], "ba": sums[0]}
    if mode == "residual":
        grads["zb"] = dres
    if two:
        grads.update(zb=dzb, gb=sums[2], bb=sums[0])
    bufs = {f"{i}.{k}": v for i, b in enumerate(bns) for k, v in (("rm", b.running_mean), ("rv", b.running_var))}
    return y, sa, grads, bufs, bns


def make_bns(C, seed, momentum=0.1, train=(True, True)):
    bns = [nn.BatchNorm2d(C, momentum=momentum), nn.BatchNorm2d(C, momentum=momentum)]
    for b in bns:
        randomize_bn(b, seed)
        seed += 1
    for b, t in zip(bns, train):
        b.train(t)
    return bns


def run_bn_case(cuda, N, C, H, W, mode, seed, momentum=0.1, train=(True, True), relu=True):
    za, zb, gy = bn_inputs(N, C, H, W, seed)
    bns = make_bns(C, seed, momentum, train)
    y64, g64, b64 = bn_ref(za, zb, gy, bns, mode, torch.float64, "cpu", relu)
    y32, g32, b32 = bn_ref(za, zb, gy, bns, mode, torch.float32, cuda, relu)
    y, (mean, rstd), g, b, hb = bn_hip(za, zb, gy, bns, mode, cuda, relu)
    label = f"{mode} N={N} C={C} {H}x{W}"
    check(label + " y", {"y": y}, {"y": y64}, {"y": y32})
    check(label, g, g64, g32)
    if train[0]:
        # the statistics themselves: mean and rstd of every channel against float64
        z64 = za.double()
        m64 = z64.mean((0, 2, 3))
        r64 = 1 / torch.sqrt(z64.var((0, 2, 3), unbiased=False) + bns[0].eps)
        assert (mean.cpu().double() - m64).abs().max() <= 1e-6 * (m64.abs() + 1).max(), label
        assert ((rstd.cpu().double() - r64).abs() / r64).max() <= 1e-5, label
        check(label + " running", b, b64, b32)
        assert int(hb[0].num_batches_tracked) == 4
    else:
        for k in ("0.rm", "0.rv"):
            assert torch.equal(b[k].cpu(), bns[0].running_mean if k == "0.rm" else bns[0].running_var), label
        assert int(hb[0].num_batches_tracked) == 3


@pytest.mark.parametrize("C", [32, 64, 128, 256, 512])
@pytest.mark.parametrize("N,H,W", [(1, 5, 7), (3, 37, 41), (3, 40, 40)])
@pytest.mark.parametrize("mode", ["none", "residual", "branch"])
def test_bn_kernels_against_float64(cuda, C, N, H, W, mode):
    """Ragged M (35, 4551 = one slice and a bit; 4800 with the float4 path), the constant and the large-mean channel in
    every case."""
    run_bn_case(cuda, N, C, H, W, mode, seed=C + N + H)


def test_bn_momentum_none_is_the_cumulative_average(cuda):
    run_bn_case(cuda, 3, 64, 9, 20, "branch", seed=5, momentum=None)


@pytest.mark.parametrize("mode", ["none", "residual", "branch"])
def test_eval_mode_bn_uses_running_statistics(cuda, mode):
    run_bn_case(cuda, 3, 64, 9, 20, mode, seed=6, train=(False, False))
    run_bn_case(cuda, 2, 32, 8, 16, mode, seed=7, train=(False, True))


def test_bn_without_relu(cuda):
    run_bn_case(cuda, 2, 64, 8, 16, "branch", seed=8, relu=False)


def test_bn_apply_reads_unaligned_views(cuda):
    """A view that does not start on a 16-byte boundary takes the scalar form: same values."""
    za, zb, gy = bn_inputs(2, 32, 8, 16, 9)
    a = make_bns(32, 9)[0].to(cuda)
    big = torch.empty(za.numel() + 1, device=cuda)
    big[1:] = za.to(cuda).flatten()
    view = big[1:].view_as(za)
    st = ops.bn_eval_stats(a.running_mean, a.running_var, a.eps)
    y0 = ops.bn_apply(za.to(cuda), st, a.weight, a.bias)
    y1 = ops.bn_apply(view, st, a.weight, a.bias)
    assert torch.equal(y0, y1)


# ---- 2. every distinct block shape inside a real training step -------------------------------------------------------------
def install_block_spy(monkeypatch):
    recs = []
    real = ops.bn_block_autograd

    def spy(x, blk, cws=None, name="block"):
        rec = dict(name=name, blk=blk, x=x.detach().clone(), pre=copy.deepcopy(blk))
        out = real(x, blk, cws, name=name)
        if x.requires_grad:
            x.register_hook(lambda g: rec.__setitem__("gin", g.clone()))
        out.register_hook(lambda g: rec.__setitem__("gout", g.clone()))
        recs.append(rec)
        return out

    monkeypatch.setattr(ops, "bn_block_autograd", spy)
    return recs


def block_ref(rec, dtype, device):
    blk = copy.deepcopy(rec["pre"]).to(device).to(dtype).train()
    x = rec["x"].to(device).to(dtype).requires_grad_(True)
    out = blk._forward_torch(x)
    out.backward(rec["gout"].to(device).to(dtype))
    grads = {k: p.grad.cpu() for k, p in blk.named_parameters()}
    grads["x"] = x.grad.cpu()
    bufs = {k: v.cpu() for k, v in blk.named_buffers() if not k.endswith("num_batches_tracked")}
    return out.detach().cpu(), grads, bufs


def image(N, seed, hw=(32, 128)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, 3) + hw, generator=g)


def gout_like(out, seed):
    return torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)


def test_every_block_shape_inside_a_training_step(cuda, monkeypatch):
    recs = install_block_spy(monkeypatch)
    m = backbone(arch=(2, 1, 1, 1, 1)).to(cuda).train().set_train_backend("hip")
    res = m(image(3, 1).to(cuda))
    res["output"].backward(gout_like(res["output"], 2))
    names = [r["name"] for r in recs]
    assert names == ["layer1.0", "layer1.1", "layer2.0", "layer3.0", "layer4.0", "layer5.0"]
    for rec in recs:
        blk = rec["blk"]
        _, g64, b64 = block_ref(rec, torch.float64, "cpu")
        _, g32, b32 = block_ref(rec, torch.float32, cuda)
        got = {k: p.grad for k, p in blk.named_parameters()}
        got["x"] = rec["gin"]
        check(rec["name"], got, g64, g32)
        bufs = {k: v for k, v in blk.named_buffers() if not k.endswith("num_batches_tracked")}
        check(rec["name"] + " running", bufs, b64, b32)
        for k, v in blk.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(v) == 4, (rec["name"], k)
    assert int(m.bn1.num_batches_tracked) == 4


def stem_ref(m, x, gout, dtype, device):
    mm = copy.deepcopy(m).to(device).to(dtype).train()
    z = mm.conv1(x.to(device).to(dtype))
    z.retain_grad()
    y = mm.relu1(mm.bn1(z))
    y.backward(gout.to(device).to(dtype))
    return mm, z.grad.cpu()


def test_stem_conv_bias_gradient_is_zero_to_rounding(cuda):
    """d(stem conv bias) = sum of dz over the channel = 0 under a training-mode BN: an absolute bar, scaled by the sum of
    |dz| of the channel (float64), not a relative one."""
    m = backbone()
    x = image(4, 3)
    mh = copy.deepcopy(m).to(cuda).train()
    y = ops.bn_stem_autograd(x.to(cuda), mh.conv1, mh.bn1)
    gout = gout_like(y, 4).cpu()
    y.backward(gout.to(cuda))
    m64, dz64 = stem_ref(m, x, gout, torch.float64, "cpu")
    scale = dz64.abs().sum((0, 2, 3))
    db = mh.conv1.bias.grad.cpu().double()
    assert (db.abs() <= 1e-5 * scale).all(), (db.abs() / scale).max()
    m32, _ = stem_ref(m, x, gout, torch.float32, cuda)
    for k in ("conv1.weight", "bn1.weight", "bn1.bias"):
        got = dict(mh.named_parameters())[k].grad
        want = dict(m64.named_parameters())[k].grad
        lib = dict(m32.named_parameters())[k].grad
        assert rel(got, want) <= bar(lib, want), k


# ---- 3. the whole backbone -------------------------------------------------------------------------------------------------
def backbone_step(m, x, gout):
    """PyTorch's composition of the backbone (CPU float64 or GPU fp32): output, parameter gradients, running statistics,
    and the gradient reaching the stem convolution's output."""
    keep = {}

    def hook(mod, inp, out):
        out.retain_grad()
        keep["z"] = out

    h = m.conv1.register_forward_hook(hook)
    out = m._forward_torch(x)["output"]
    h.remove()
    out.backward(gout)
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    bufs = {k: v.clone() for k, v in m.named_buffers() if not k.endswith("num_batches_tracked")}
    return out.detach(), grads, bufs, keep["z"].grad


def test_whole_backbone_against_float64(cuda):
    m = backbone(arch=(3, 4, 6, 6, 3))
    x = image(8, 5)
    mh = copy.deepcopy(m).to(cuda).train().set_train_backend("hip")
    res = mh(x.to(cuda))["output"]
    gout = gout_like(res, 6)
    res.backward(gout)
    gh = {k: p.grad for k, p in mh.named_parameters()}
    bh = {k: v for k, v in mh.named_buffers() if not k.endswith("num_batches_tracked")}
    o64, g64, b64, dz64 = backbone_step(copy.deepcopy(m).double().train(), x.double(), gout.cpu().double())
    o32, g32, b32, _ = backbone_step(copy.deepcopy(m).to(cuda).train(), x.to(cuda), gout)
    check("output", {"y": res}, {"y": o64}, {"y": o32})
    g64.pop("conv1.bias")                     # zero but for rounding: the absolute bar below
    assert len(g64) == len(list(m.parameters())) - 1
    check("backbone grads", gh, g64, g32)
    check("backbone running", bh, b64, b32)
    scale = dz64.abs().sum((0, 2, 3))
    assert (gh["conv1.bias"].cpu().double().abs() <= 1e-5 * scale).all()
    for k, v in mh.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 4, k


def test_no_library_layer_runs(cuda, monkeypatch):
    m = backbone().to(cuda).train().set_train_backend("hip")

    def refuse(*a, **k):
        raise AssertionError("a library layer ran in the backbone's hip training graph")

    for cls in (nn.Conv2d, nn.BatchNorm2d, nn.ReLU):
        monkeypatch.setattr(cls, "forward", refuse)
    monkeypatch.setattr(F, "conv2d", refuse)
    monkeypatch.setattr(F, "batch_norm", refuse)
    res = m(image(2, 7).to(cuda))["output"]
    res.square().mean().backward()
    assert torch.isfinite(res).all()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_bitwise_reproducible_across_calls_and_streams(cuda):
    m0 = backbone(arch=(2, 1, 1, 1, 1)).to(cuda).train()
    x = image(3, 8).to(cuda)

    def run():
        m = copy.deepcopy(m0).set_train_backend("hip")
        out = m(x)["output"]
        out.backward(gout_like(out, 9))
        return [p.grad.clone() for p in m.parameters()] + [b.clone() for b in m.buffers()] + [out.detach()]

    a = run()
    b = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)


def test_frozen_stage_and_needs_input_grad(cuda, monkeypatch):
    """A frozen stage passes input gradients on and gets no parameter gradients; the stem launches no data gradient
    (the image needs none); a frozen convolution launches no weight gradient."""
    calls = {"data": 0, "weight": 0}
    real_data, real_weight = ops.conv2d_bwd_data, ops.conv2d_bwd_weight

    def data(*a, **k):
        calls["data"] += 1
        return real_data(*a, **k)

    def weight(*a, **k):
        calls["weight"] += 1
        return real_weight(*a, **k)

    monkeypatch.setattr(ops, "conv2d_bwd_data", data)
    monkeypatch.setattr(ops, "conv2d_bwd_weight", weight)
    m = backbone().to(cuda).train().set_train_backend("hip")
    for p in m.layer2.parameters():
        p.requires_grad_(False)
    out = m(image(2, 10).to(cuda))["output"]
    out.square().mean().backward()
    assert all(p.grad is None for p in m.layer2.parameters())
    for k, p in m.named_parameters():
        if not k.startswith("layer2."):
            assert p.grad is not None and p.grad.abs().max() > 0, k
    # 5 blocks, each with a downsample: 3 data gradients per block (conv2, conv1, downsample), none for the stem;
    # weight gradients: the stem + 3 per trainable block
    assert calls == {"data": 15, "weight": 1 + 4 * 3}, calls
    # freezing changes no other gradient: the same step with nothing frozen gives the same bits (the data-gradient path
    # runs the same kernels on the same tensors)
    full = backbone().to(cuda).train().set_train_backend("hip")
    full(image(2, 10).to(cuda))["output"].square().mean().backward()
    for k, p in full.named_parameters():
        if not k.startswith("layer2."):
            assert torch.equal(p.grad, dict(m.named_parameters())[k].grad), k


def test_eval_mode_bn_inside_a_training_backbone(cuda):
    """Frozen-BN fine-tuning: BNs in .eval() normalise with their running statistics, leave them alone, and the gradients
    match PyTorch's."""
    m = backbone(arch=(2, 1, 1, 1, 1))
    m.train()
    for mod in list(m.layer1.modules()) + [m.bn1, m.layer3[0].downsample[1]]:
        if isinstance(mod, nn.BatchNorm2d):
            mod.eval()
    x = image(3, 11)
    mh = copy.deepcopy(m).to(cuda).set_train_backend("hip")
    frozen = {k: v.clone() for k, v in mh.named_buffers() if k.startswith(("layer1.", "bn1.", "layer3.0.downsample.1."))}
    res = mh(x.to(cuda))["output"]
    gout = gout_like(res, 12)
    res.backward(gout)
    for k, v in mh.named_buffers():
        if k in frozen:
            assert torch.equal(v, frozen[k]), k
    o64, g64, b64, _ = backbone_step(copy.deepcopy(m).double(), x.double(), gout.cpu().double())
    o32, g32, b32, _ = backbone_step(copy.deepcopy(m).to(cuda), x.to(cuda), gout)
    gh = {k: p.grad for k, p in mh.named_parameters()}
    # the stem bias sees an eval-mode BN: its gradient is not zero and takes the relative bar like the others
    check("frozen-BN grads", gh, g64, g32)
    check("frozen-BN running", {k: v for k, v in mh.named_buffers() if not k.endswith("num_batches_tracked")}, b64, b32)


def test_sgd_steps_track_the_torch_backend(cuda):
    x = image(4, 13).to(cuda)
    final = {}
    for mode in ("torch", "hip"):
        m = backbone().to(cuda).train().set_train_backend(mode)
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        for _ in range(3):
            opt.zero_grad()
            m(x)["output"].square().mean().backward()
            opt.step()
        final[mode] = {k: v.detach().clone() for k, v in list(m.named_parameters()) + list(m.named_buffers())}
    for k, t in final["torch"].items():
        h = final["hip"][k]
        if t.dtype == torch.int64:
            assert torch.equal(t, h), k
        else:
            assert rel(h, t) <= 1e-3, (k, rel(h, t))


def test_nrtr_forward_train_with_the_hip_backbone(cuda):
    import tps_pp_amd as P
    torch.manual_seed(0)
    m = P.build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                         strides=[2, 1, 2, 1, 2]),
                              tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                              decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                              label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
                              max_seq_len=8))
    m = m.to(cuda).train().set_train_backend("hip_all", backbone="hip")
    assert m.tpsnet.train_backend == "hip_all" and m.backbone.train_backend == "hip"
    img = torch.randn((2, 3, 32, 128), device=cuda)
    metas = [dict(resize_shape=(32, 128, 3), text="ab"), dict(resize_shape=(32, 100, 3), text="tps")]
    losses = m.forward_train(img, metas)
    sum(v.mean() for v in losses.values()).backward()
    for k, p in list(m.backbone.named_parameters()) + list(m.tpsnet.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    # stages 0 and 1 feed TPS++ as well: their gradients include what flows back from it
    assert m.backbone.layer1[0].conv1.weight.grad.abs().max() > 0


def test_eval_path_unaffected_by_the_switch(cuda):
    m = backbone(arch=(2, 1, 1, 1, 1)).to(cuda).eval()
    x = image(3, 14).to(cuda)
    with torch.no_grad():
        before = m(x)["output"].clone()
        m.set_train_backend("hip")
        after = m(x)["output"]
    assert torch.equal(before, after)
    assert np.isfinite(after.cpu().numpy()).all()


# ---- 8. frozen-BN fine-tuning: eval-mode BatchNorms whose gamma and beta do not train ----------------------------------
def freeze_bn(bn):
    bn.eval()
    bn.weight.requires_grad_(False)
    bn.bias.requires_grad_(False)


def frozen_bn_step_against_float64(cuda, m, seed):
    x = image(3, seed)
    mh = copy.deepcopy(m).to(cuda).set_train_backend("hip")
    bufs = {k: v.clone() for k, v in mh.named_buffers()}
    res = mh(x.to(cuda))["output"]
    gout = gout_like(res, seed + 1)
    res.backward(gout)
    o64, g64, b64, _ = backbone_step(copy.deepcopy(m).double(), x.double(), gout.cpu().double())
    o32, g32, b32, _ = backbone_step(copy.deepcopy(m).to(cuda), x.to(cuda), gout)
    gh = {k: p.grad for k, p in mh.named_parameters()}
    for k, p in mh.named_parameters():
        assert (p.grad is None) == (not p.requires_grad), k
    check("frozen-BN output", {"y": res}, {"y": o64}, {"y": o32})
    check("frozen-BN grads", gh, g64, g32)
    return mh, bufs


def test_eval_stem_bn_with_frozen_affine_and_trainable_conv(cuda):
    """The stem's BatchNorm in .eval() with gamma and beta frozen, its convolution training: the backward runs no
    reduction for it (no gamma / beta gradient, running statistics) and must pass the data gradient on all the same."""
    m = backbone(arch=(2, 1, 1, 1, 1)).train()
    freeze_bn(m.bn1)
    mh, bufs = frozen_bn_step_against_float64(cuda, m, 15)
    assert mh.conv1.weight.grad is not None and mh.conv1.bias.grad is not None
    assert mh.bn1.weight.grad is None and mh.bn1.bias.grad is None
    for k in ("bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked"):
        assert torch.equal(dict(mh.named_buffers())[k], bufs[k]), k


def test_frozen_bn_fine_tuning_of_the_whole_backbone(cuda):
    """Every BatchNorm in .eval() with frozen gamma and beta (the usual frozen-BN fine-tuning): convolution gradients
    against PyTorch's, no running statistic touched."""
    m = backbone(arch=(2, 1, 1, 1, 1)).train()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            freeze_bn(mod)
    mh, bufs = frozen_bn_step_against_float64(cuda, m, 17)
    for k, v in mh.named_buffers():
        assert torch.equal(v, bufs[k]), k


def test_bn_bwd_data_without_sums_for_an_eval_mode_branch(cuda):
    """ops.bn_bwd_data with no reduction (sums=None) for eval-mode branches: dz = gamma rstd dr, exactly what the kernel
    forms, for one branch and for two with the shortcut's gradient added."""
    za, zb, gy = bn_inputs(3, 64, 8, 16, 19)
    a, b = (bn.to(cuda) for bn in make_bns(64, 19, train=(False, False)))
    za, zb, gy = za.to(cuda), zb.to(cuda), gy.to(cuda)
    sa = ops.bn_eval_stats(a.running_mean, a.running_var, a.eps)
    sb = ops.bn_eval_stats(b.running_mean, b.running_var, b.eps)
    y = ops.bn_apply(za, sa, a.weight, a.bias, zb=zb, stats_b=sb, gamma_b=b.weight, beta_b=b.bias)
    dr64 = gy.double().cpu() * (y.cpu() > 0).double()
    want_a = (a.weight.double() * sa[1].double()).cpu()[None, :, None, None] * dr64
    want_b = (b.weight.double() * sb[1].double()).cpu()[None, :, None, None] * dr64
    dza, _ = ops.bn_bwd_data(gy, y, za, sa, a.weight, None, False, relu=True)
    assert rel(dza, want_a) <= 1e-6
    base = torch.randn(gy.shape, generator=torch.Generator().manual_seed(20)).to(cuda)
    dres = base.clone()
    dza, dzb = ops.bn_bwd_data(gy, y, za, sa, a.weight, None, False, zb=zb, stats_b=sb, gamma_b=b.weight, train_b=False,
                               relu=True, dres=dres, dres_mode=2)
    assert rel(dza, want_a) <= 1e-6 and rel(dzb, want_b) <= 1e-6
    assert torch.equal(dres, base + gy * (y > 0))
    # a training-mode branch without its sums is refused before anything is launched
    with pytest.raises(ValueError):
        ops.bn_bwd_data(gy, y, za, sa, a.weight, None, True, relu=True)
    # the shortcut's gradient is written in place: a non-contiguous dres is refused, not silently copied
    with pytest.raises(ValueError, match="contiguous"):
        ops.bn_bwd_data(gy, y, relu=True, dres=base.transpose(2, 3).contiguous().transpose(2, 3), dres_mode=2,
                        want_a=False, want_b=False)
