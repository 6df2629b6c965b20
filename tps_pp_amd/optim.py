"""The optimiser stage of a training iteration on HIP kernels (include/tpspp_train_opt.h, csrc/tpspp_optim.hip).

`Adam` and `AdamW` subclass `torch.optim.Optimizer`: `param_groups`, LR schedulers, `state_dict()` and
`load_state_dict()` are PyTorch's, and the per-parameter state uses torch's keys and types (`step`: a 0-dim fp32 CPU
tensor -- all of them views of one tensor, so that they advance in one operation --, `exp_avg`, `exp_avg_sq`), so a `state_dict()` loads into `torch.optim.Adam` and back, and the `optimizer` entry of
a checkpoint written by the reference's runner resumes here.

replaces: torch.optim.Adam / AdamW (amsgrad=False, maximize=False) as `tools/train.py` builds them from
`optimizer = dict(type='Adam', lr=1e-4)` (configs/_base_/schedules/schedule_adam_step_12e.py), mmcv's
`DefaultOptimizerConstructor` for the `paramwise_cfg.custom_keys` of schedule_adam_custom_key_step_10e.py
(`build_optimizer`), and the gradient clipping of mmcv's `OptimizerHook` (`grad_clip`).

`step()` is ONE launch for all parameters (three with clipping) and never synchronises with the host: the kernels read a
tensor table and a chunk map from device memory, which are rebuilt only when a parameter, gradient or state tensor
moved; the per-tensor scalars (`lr / (1 - beta1^t)`, `sqrt(1 - beta2^t)`, `weight_decay`, `1 - lr * weight_decay`) are
computed on the host in double and uploaded asynchronously from a fresh pinned tensor whenever one of them changed.
The kernels write parameters through raw pointers, which bumps no version counter; `step()` therefore increments the
version of every parameter it updated, so that the prepared-weight cache (`_prepared.py`) rebuilds.

Differences from PyTorch, all deliberate: clipping leaves the gradients unscaled (`clip_grad_norm_` scales them in
place; here the coefficient goes to the update kernel by device pointer) and `last_grad_norm` is a 0-dim device tensor
that nobody has to read; all groups share `betas` and `eps` (they travel by value in the one launch); no `amsgrad`,
`maximize`, `foreach`, `fused`, `capturable` or `differentiable` modes; no CPU or eager fallback.
"""
import math

import torch

from . import _lib
from .ops import _call

CHUNK = 4096      # elements per workgroup and THREADS per workgroup: scripts/bench_optimizer.py's sweep
THREADS = 1024
VECTOR = 4        # elements of a 128-bit access: CHUNK must be a multiple

_MODES = {"Adam": 0, "AdamW": 1}


def build_chunk_map(numels, chunk=CHUNK):
    """[(tensor index, first element)] covering every element of every tensor exactly once, tensors and elements
    ascending, `chunk` elements per row (the last row of a tensor may be shorter); a tensor without elements gets no row."""
    if chunk <= 0 or chunk % VECTOR:
        raise ValueError(f"build_chunk_map: chunk must be a positive multiple of {VECTOR}, got {chunk}")
    rows = []
    for ti, n in enumerate(numels):
        rows.extend((ti, first) for first in range(0, int(n), chunk))
    return rows


def _scalar_row(lr, beta1, beta2, wd, t):
    """{step_size, bc2_sqrt, wd, decay} of include/tpspp_train_opt.h in double; the upload rounds each once to fp32."""
    return (lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), wd, 1.0 - lr * wd)


class _MultiTensorAdam(torch.optim.Optimizer):
    _MODE = "Adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, grad_clip=None,
                 chunk=CHUNK, threads=THREADS):
        if isinstance(lr, torch.Tensor) or not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr!r} (a float, not negative)")
        if not eps >= 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not weight_decay >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise NotImplementedError("amsgrad: the HIP optimiser implements amsgrad=False only")
        if chunk <= 0 or chunk % VECTOR or threads not in (64, 128, 256, 512, 1024):
            raise ValueError(f"chunk must be a positive multiple of {VECTOR} and threads one of 64 .. 1024, got "
                             f"{chunk}, {threads}")
        self.max_norm = None
        if grad_clip is not None:
            extra = set(grad_clip) - {"max_norm", "norm_type"}
            if extra or "max_norm" not in grad_clip:
                raise ValueError(f"grad_clip: dict(max_norm=..., norm_type=2), got {grad_clip!r}")
            if grad_clip.get("norm_type", 2) not in (2, 2.0):
                raise NotImplementedError(f"grad_clip: norm_type {grad_clip['norm_type']!r}; the HIP norm is L2 only")
            if not float(grad_clip["max_norm"]) > 0.0:
                raise ValueError(f"grad_clip: max_norm must be positive, got {grad_clip['max_norm']!r}")
            self.max_norm = float(grad_clip["max_norm"])
        # torch.optim.Adam's own keys, so that a state_dict moves between the two classes in both directions
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.chunk, self.threads = int(chunk), int(threads)
        self.table_builds = 0          # how often the tensor table and the chunk map were (re)built
        self.scalar_uploads = 0        # how often the per-tensor scalar rows went to the device
        self.last_grad_norm = None     # 0-dim device tensor after a step() with grad_clip
        self.param_names = {}          # id(parameter) -> name, for error messages (build_optimizer fills it)
        self._key = self._table = self._map = self._scalars = self._rows = self._partials = self._norm = None
        self._n_tensors = self._n_chunks = 0
        self._step_all = self._step_views = None

    # ---- what the kernels work from ----------------------------------------------------------------------------------
    def _name(self, p, gi, pi):
        return self.param_names.get(id(p), f"parameter {pi} of group {gi} {tuple(p.shape)}")

    def _refuse(self, p, gi, pi):
        """Why parameter `pi` of group `gi` cannot go to the kernels (raises)."""
        who, st = self._name(p, gi, pi), self.state.get(p, {})
        for what, t in (("", p), ("the gradient of ", p.grad), ("the state exp_avg of ", st.get("exp_avg")),
                        ("the state exp_avg_sq of ", st.get("exp_avg_sq"))):
            if t is None:
                continue
            if not t.is_cuda:
                raise _lib.TpsppError(f"{self._MODE}: {what}{who} is on {t.device}; the HIP optimiser needs GPU tensors "
                                      "(no CPU fallback)")
            if t.dtype != torch.float32 or t.is_sparse or not t.is_contiguous() or t.shape != p.shape:
                raise _lib.TpsppError(f"{self._MODE}: {what}{who} must be a dense contiguous fp32 tensor of the "
                                      f"parameter's shape, got {t.dtype} {tuple(t.shape)}, "
                                      f"{'sparse' if t.is_sparse else f'strides {t.stride()}'}")
        raise _lib.TpsppError(f"{self._MODE}: {who}, its gradient and its state must be on one device, the one all "
                              "parameters of this optimiser share")

    def _active(self, need_state):
        """(parameters that have a gradient, where they sit, their groups, key, their step counters).  key: the tuple of
        (p, g, numel, m, v) addresses that the table is built from (m = v = 0 without state).  Per call only what can
        change behind an unchanged key is checked here (fp32, contiguous); `_prepare` checks devices and shapes whenever
        the key moved, and an address names its device.  With need_state the state of every such parameter exists."""
        f32, params, where, groups, key, steps = torch.float32, [], [], [], [], []
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                if not (p.dtype is f32 and g.dtype is f32 and p.is_contiguous() and g.is_contiguous()):
                    self._refuse(p, gi, pi)
                m = v = 0
                if need_state:
                    st = self.state[p]
                    if not st:
                        st["step"] = torch.tensor(0.0, dtype=f32)
                        st["exp_avg"] = torch.empty_like(p.detach()).zero_()
                        st["exp_avg_sq"] = torch.empty_like(p.detach()).zero_()
                    m, v = st["exp_avg"], st["exp_avg_sq"]
                    if not (m.dtype is f32 and v.dtype is f32 and m.is_contiguous() and v.is_contiguous()):
                        self._refuse(p, gi, pi)
                    m, v = m.data_ptr(), v.data_ptr()
                    steps.append(st["step"])
                params.append(p)
                where.append((gi, pi))
                groups.append(group)
                key.append((p.data_ptr(), g.data_ptr(), p.numel(), m, v))
        return params, where, groups, tuple(key), steps

    def _count(self, params, steps):
        """Advance the step counters of `params` by one and return them as floats.  The counters stay what torch keeps
        (0-dim fp32 CPU tensors under state[p]["step"]), but as views of ONE tensor, so that 390 of them advance in one
        operation; counters that came from elsewhere (load_state_dict, a changed set of parameters with gradients) are
        adopted with their values first."""
        views = self._step_views
        if views is None or len(views) != len(steps) or any(a is not b for a, b in zip(steps, views)):
            self._step_all = torch.tensor([float(t) for t in steps], dtype=torch.float32)
            views = self._step_views = list(self._step_all.unbind(0))
            for p, view in zip(params, views):
                self.state[p]["step"] = view
        self._step_all += 1
        return self._step_all.tolist()

    def _upload(self, values, dtype, shape, device, into=None):
        """Host values -> a fresh pinned tensor -> an asynchronous copy into a device tensor (`into` if it fits, else a new
        one).  PyTorch's pinned-memory allocator does not hand the block out again before the copy that reads it has
        finished, and the copy is ordered on the stream behind the kernels that still read `into`."""
        host = torch.empty(shape, dtype=dtype, pin_memory=True)
        host.copy_(torch.tensor(values, dtype=torch.float64 if dtype == torch.float32 else dtype).view(shape))
        dev = into if into is not None and into.shape == shape and into.device == device else \
            torch.empty(shape, dtype=dtype, device=device)
        dev.copy_(host, non_blocking=True)
        return dev

    def _prepare(self, key, params, where):
        """(Re)build the table and the chunk map if a tensor moved; every tensor is then checked in full -- on one GPU, dense,
        of the parameter's shape -- before anything is launched."""
        if key == self._key:
            return
        device = params[0].device
        for p, (gi, pi) in zip(params, where):
            st = self.state.get(p, {})
            for t in (p, p.grad, st.get("exp_avg"), st.get("exp_avg_sq")):
                if t is not None and not (t.is_cuda and t.device == device and t.layout is torch.strided
                                          and t.shape == p.shape):
                    self._refuse(p, gi, pi)
        live = [k for k in key if k[2] > 0]
        self._n_tensors, self._key, self._rows = len(live), key, None
        if not live:
            self._n_chunks = 0
            return
        chunks = build_chunk_map([k[2] for k in live], self.chunk)
        self._n_chunks = len(chunks)
        self._table = self._upload([[k[0], k[1], k[3], k[4], k[2]] for k in live], torch.int64, (len(live), 5), device)
        self._map = self._upload(chunks, torch.int64, (len(chunks), 2), device)
        if self.max_norm is not None:
            self._partials = torch.empty((len(chunks),), dtype=torch.float32, device=device)
            self._norm = torch.empty((3,), dtype=torch.float32, device=device)
        self.table_builds += 1

    # ---- torch.optim.Optimizer ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params, where, groups, key, steps = self._active(need_state=True)
        if not params:
            return loss
        shared = {(tuple(g["betas"]), g["eps"]) for g in self.param_groups}
        if len(shared) != 1:
            raise NotImplementedError(f"{self._MODE}.step: param groups differ in betas / eps {sorted(shared)}; the one "
                                      "launch takes them by value")
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError(f"{self._MODE}.step: amsgrad / maximize are not implemented on HIP")
        (beta1, beta2), eps = next(iter(shared))
        device = params[0].device
        self._prepare(key, params, where)
        counts = self._count(params, steps)
        rows, memo = [], {}
        for k, group, t in zip(key, groups, counts):
            if k[2] == 0:
                continue
            q = (group["lr"], group["weight_decay"], t)
            row = memo.get(q)
            if row is None:
                row = memo[q] = _scalar_row(float(q[0]), beta1, beta2, float(q[1]), t)
            rows.append(row)
        if self._n_chunks == 0:
            return loss
        if rows != self._rows:                        # warm-up changes lr, the step count changes the bias corrections
            self._scalars = self._upload(rows, torch.float32, (len(rows), 4), device, into=self._scalars)
            self._rows = rows
            self.scalar_uploads += 1
        coef = 0
        if self.max_norm is not None:
            _call("tpspp_mt_sumsq", device, self._table, self._n_tensors, self._map, self._n_chunks, self.chunk, self.threads,
                  self._partials, self._partials.numel())
            _call("tpspp_mt_norm_finish", device, self._partials, self._n_chunks, self.max_norm, self._norm)
            self.last_grad_norm = self._norm[0]
            coef = self._norm.data_ptr() + 4
        _call("tpspp_mt_adam", device, self._table, self._scalars, self._n_tensors, self._map, self._n_chunks, self.chunk,
              self.threads, beta1, beta2, eps, _MODES[self._MODE], coef)
        # the kernel wrote through raw pointers: tell autograd and the prepared-weight cache that the parameters changed
        torch.autograd.graph.increment_version([p for p, k in zip(params, key) if k[2]])
        return loss

    @property
    def grad_clip_state(self):
        """The (3,) device tensor {norm, coefficient, non-finite flag} of the last clipped step(), or None."""
        return self._norm

    def zero_grad(self, set_to_none=True):
        """set_to_none=True (torch's default): drops the gradients, no kernel.  False: one launch writes +0.0 over all."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        need_state = all(len(self.state.get(p, ())) for g in self.param_groups for p in g["params"] if p.grad is not None)
        params, where, _, key, _ = self._active(need_state)   # with the state in the key, step() shares the table
        if not params:
            return
        device = params[0].device
        self._prepare(key, params, where)
        if self._n_chunks == 0:
            return
        _call("tpspp_mt_zero", device, self._table, self._n_tensors, self._map, self._n_chunks, self.chunk, self.threads)
        torch.autograd.graph.increment_version([p.grad for p, k in zip(params, key) if k[2]])


class Adam(_MultiTensorAdam):
    """torch.optim.Adam(amsgrad=False) in one HIP launch: weight decay joins the gradient (g += wd * p)."""
    _MODE = "Adam"


class AdamW(_MultiTensorAdam):
    """torch.optim.AdamW(amsgrad=False) in one HIP launch: decoupled weight decay (p *= 1 - lr * wd)."""
    _MODE = "AdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)


_HIP = {"Adam": Adam, "AdamW": AdamW}
_TORCH = {"Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW}


def build_optimizer(model, cfg, backend="hip", grad_clip=None):
    """The optimiser of `cfg = dict(type='Adam' | 'AdamW', lr=..., betas=..., eps=..., weight_decay=...,
    paramwise_cfg=dict(custom_keys={substring: dict(lr_mult=..., decay_mult=...)}))` over `model`'s parameters: the part of
    mmcv 1.x's `DefaultOptimizerConstructor` that the reference's schedules use.  Without `paramwise_cfg` all parameters
    form one group.  With it every parameter is a group of its own; the keys are sorted alphabetically, then by length
    descending, and the first one that is a substring of the parameter's name sets `lr = lr * lr_mult` and (if the config
    has a weight decay) `weight_decay = weight_decay * decay_mult`; a parameter that does not require a gradient keeps the
    defaults.  backend "hip": this module's class (grad_clip: mmcv's `optimizer_config.grad_clip`); "torch": the
    `torch.optim` class of that name with the same groups (clipping is then the caller's `clip_grad_norm_`)."""
    if backend not in ("hip", "torch"):
        raise ValueError(f'build_optimizer: backend "hip" or "torch", got {backend!r}')
    if backend == "torch" and grad_clip is not None:
        raise ValueError('build_optimizer: grad_clip belongs to the "hip" backend; with "torch" call clip_grad_norm_')
    cfg = dict(cfg)
    kind = cfg.pop("type", None)
    if kind not in _HIP:
        raise NotImplementedError(f"build_optimizer: optimizer type {kind!r}; the TPS++ configs train with 'Adam' "
                                  "('AdamW' is implemented as well)")
    paramwise = cfg.pop("paramwise_cfg", None)
    cfg.pop("constructor", None)
    unknown = set(cfg) - {"lr", "betas", "eps", "weight_decay", "amsgrad"}
    if unknown:
        raise NotImplementedError(f"build_optimizer: optimizer fields {sorted(unknown)} are not implemented")
    named = [(n, p) for n, p in model.named_parameters()]
    if paramwise is None:
        params = [p for _, p in named]
    else:
        other = set(paramwise) - {"custom_keys"}
        if other:
            raise NotImplementedError(f"build_optimizer: paramwise_cfg fields {sorted(other)} are not implemented "
                                      "(custom_keys only)")
        custom = paramwise.get("custom_keys", {})
        for key, mult in custom.items():
            bad = set(mult) - {"lr_mult", "decay_mult"}
            if bad:
                raise NotImplementedError(f"build_optimizer: custom_keys[{key!r}] fields {sorted(bad)} are not implemented")
        base_lr = cfg.get("lr", 1e-3)
        base_wd = cfg.get("weight_decay")
        keys = sorted(sorted(custom), key=len, reverse=True)
        params = []
        for name, p in named:
            group = {"params": [p]}
            if p.requires_grad:
                for key in keys:
                    if key in name:
                        group["lr"] = base_lr * custom[key].get("lr_mult", 1.0)
                        if base_wd is not None:
                            group["weight_decay"] = base_wd * custom[key].get("decay_mult", 1.0)
                        break
            params.append(group)
    if backend == "torch":
        return _TORCH[kind](params, **cfg)
    opt = _HIP[kind](params, grad_clip=grad_clip, **cfg)
    opt.param_names = {id(p): n for n, p in named}
    return opt
