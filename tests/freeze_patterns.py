"""Freeze patterns for the autograd Functions of the HIP training graph (a helper module of the -m gpu tests, not a
conftest): which gradients a Function's backward returns when some of its inputs and parameters want none."""
import torch


def check_freeze_patterns(monkeypatch, fn_cls, call, inputs, params, last, more=None):
    """The backward of the autograd Function `fn_cls` inside `call(*inputs)`, once with every input and every parameter
    of `params` ({name: Parameter}) trainable and once per freeze pattern.  What the backward itself returns (recorded
    around it, before autograd drops anything) is None for exactly the tensors that want no gradient, and every gradient
    that is wanted has the bits of the all-trainable run: the kernels' split-K is fixed by the shapes, so a frozen
    neighbour changes no summation order.  `last`: the name prefix of the block's last Linear layer; `more`: further
    patterns {label: the names that stay trainable} (the inputs are "input0", "input1", ...)."""
    seen = []
    real = fn_cls.backward

    def spy(ctx, *g):
        res = real(ctx, *g)
        seen.append((tuple(ctx.needs_input_grad), [None if t is None else t.detach().clone() for t in res]))
        return res

    monkeypatch.setattr(fn_cls, "backward", staticmethod(spy))
    tensors = {f"input{i}": t for i, t in enumerate(inputs)}
    tensors.update(params)
    patterns = {
        "everything trainable": set(tensors),
        "inputs frozen": set(params),
        "LayerNorm parameters frozen": {k for k in tensors if "norm" not in k},
        "biases frozen": {k for k in tensors if not k.endswith(".bias")},
        "only the last Linear trainable": {k for k in params if k.startswith(last)},
        "parameters frozen": set(tensors) - set(params),
    }
    patterns.update(more or {})
    base = gout = None
    for label, live in patterns.items():
        assert live and live <= set(tensors), label
        for k, t in tensors.items():
            t.requires_grad_(k in live)
            t.grad = None
        out = call(*inputs)
        if gout is None:
            gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
        out.backward(gout)
        torch.cuda.synchronize()
        (need, res), = seen
        seen.clear()
        assert sum(need) == len(live), f"{label}: {len(live)} tensors trainable, the Function sees {sum(need)}"
        for i, (n, g) in enumerate(zip(need, res)):
            assert (g is not None) == n, f"{label}: argument {i} {'wants a' if n else 'got an unwanted'} gradient"
        if base is None:
            base = res
        for i, (n, g, b) in enumerate(zip(need, res, base)):
            assert not n or torch.equal(g, b), f"{label}: the gradient of argument {i} differs from the all-trainable run"
