"""-m gpu, two devices: a wrapper's launch lands on the device of its tensors, not on the current one.

Each wrapper runs on cuda:0 tensors with device 0 current and on cuda:1 tensors while device 0 is still current; the
inputs are copies of one seeded CPU set and the kernels are documented as bitwise reproducible, so the two results must
have the same bits.  The reference is the code's own device-0 result: this is about where `ops._call` launches -- the
library keys its per-device state on the current device -- not about arithmetic."""
import pytest
import torch

from tps_pp_amd import ops

gpu = pytest.mark.gpu


def _inputs():
    g = torch.Generator().manual_seed(20)
    r = lambda *shape: torch.randn(shape, generator=g)                     # noqa: E731
    return {
        "lin": (r(5, 7), r(3, 7), r(3)),                                      # rows 5, K 7, O 3
        "act": (r(37), r(37)),                                                # GELU, 37 elements
        "ln": (r(3, 8), r(8), r(8)),                                          # rows 3, P 8
        "attn": (r(1, 3, 64), r(1, 3, 64), r(1, 3, 64), r(1, 3, 64)),         # q, k, v, d out: N 1, T 3, C 64
        "ce": (r(2, 3, 5), torch.randint(0, 5, (2, 3), generator=g), r(6)),   # N 2, L 3, 5 classes
    }


def _run(inp, dev):
    """Every wrapper of the case table on copies of `inp` on `dev` -> its results on the host."""
    put = lambda t: t.to(dev)                                               # noqa: E731
    out = {}
    x, w, b = map(put, inp["lin"])
    out["linear_fwd"] = ops.linear_fwd(x, ops._dense(5, 7), w, b)
    gy, u = map(put, inp["act"])
    out["act_bwd"] = ops.act_bwd(ops.ACT_GELU, gy, u)
    x, w, b = map(put, inp["ln"])
    out["plane_ln_fwd"] = ops.plane_ln_fwd(x, w, b, 1e-5)
    q, k, v, go = map(put, inp["attn"])
    qkv = [t.requires_grad_() for t in (q, k, v)]
    a = ops.attn_train_autograd(*qkv, drop_p=0.0)
    a.backward(go)
    out["attn_train_autograd"] = (a.detach(), *(t.grad for t in qkv))
    logits, tgt, gl = map(put, inp["ce"])
    logits.requires_grad_()
    loss = ops.seq_cross_entropy_autograd(logits, tgt)
    loss.backward(gl)
    out["seq_cross_entropy_autograd"] = (loss.detach(), logits.grad)
    torch.cuda.synchronize(dev)
    return {k: [t.cpu() for t in (v if isinstance(v, (tuple, list)) else (v,))] for k, v in out.items()}


@gpu
def test_launch_lands_on_the_tensors_device_not_the_current_one(cuda):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: the second device's tensors are used while the first device is current")
    inp = _inputs()
    with torch.cuda.device(0):
        ref = _run(inp, torch.device("cuda:0"))
        got = _run(inp, torch.device("cuda:1"))
        assert torch.cuda.current_device() == 0
    for name, tensors in ref.items():
        assert len(tensors) == len(got[name])
        for i, (r, g) in enumerate(zip(tensors, got[name])):
            assert r.dtype == g.dtype and r.shape == g.shape, (name, i)
            assert torch.equal(r.view(torch.int32), g.view(torch.int32)), f"{name}[{i}]: cuda:1 differs from cuda:0"
