"""The one cache of prepared kernel weights.

Every HIP forward first turns PyTorch parameters into a kernel layout (BatchNorm folded, K-major, bf16 hi / lo slabs,
pointer tables, transposed tables) and keeps the result on the module until its sources change.  "Changed" means: the
`(data_ptr(), _version)` of a source tensor moved (an optimiser step, an in-place op, `load_state_dict`, `.to()`, a
replaced parameter), its device did, or the arithmetic configuration the caller passes as `config` did.

Blind spot: an edit through `param.data` bumps the version counter of a different tensor and is NOT seen.  After one,
call `invalidate_prepared(module)` (`TPS_PP.invalidate_train_cache()` / `ResNetABI_v2_large.invalidate_train_cache()`
do); otherwise a forward would keep using the stale layout.  A kernel that writes parameters through raw pointers is the
same blind spot; the one that exists, the multi-tensor Adam of `optim.py`, closes it itself: after its launch `step()`
calls `torch.autograd.graph.increment_version` on every parameter it updated, so the key above moves and the next
forward rebuilds (tests/test_gpu_optim.py shows it).

All slots of a module live in one private dict in the module's `__dict__`: never a registered buffer or submodule, so
`state_dict()`, `parameters()` and `buffers()` do not see them.
"""
import torch

_SLOTS = "_tpspp_prepared"


def _tensors(sources):
    for s in sources:
        if isinstance(s, torch.nn.Module):
            yield from s.parameters()
            yield from s.buffers()
        elif s is not None:
            yield s


def prepared(owner, slot, sources, build, config=()):
    """What `build()` returned for `slot` of the module `owner`, rebuilt only when stale.  sources: modules (all their
    parameters and buffers) and / or tensors (None entries are skipped) the prepared object is made from; config: whatever
    else selects its form (x3, bf16, source channel counts ...)."""
    key = (tuple((t.data_ptr(), t._version, t.device) for t in _tensors(sources)), config)
    slots = owner.__dict__.get(_SLOTS)
    if slots is None:
        slots = owner.__dict__[_SLOTS] = {}
    ent = slots.get(slot)
    if ent is None or ent[0] != key:
        ent = slots[slot] = (key, build())
    return ent[1]


def invalidate_prepared(module):
    """Drop every slot on `module` and its submodules; the next forward rebuilds what it needs.  Returns `module`."""
    for m in module.modules():
        m.__dict__.pop(_SLOTS, None)
    return module
