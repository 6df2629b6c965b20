"""Tensor-level wrappers of the C ABI (the headers under include/, bound by `_lib`).

Each function mirrors one PyTorch call site of the reference (cited in the docstring) and hands raw
device pointers + the current HIP stream to libtpspp_hip.so.  Inputs must be CUDA(HIP) tensors of the
dtype each wrapper names -- float32, bfloat16 on the bf16 paths, integer tokens and lengths; anything
else raises -- there is no eager / CPU fallback on purpose.

Every launch goes through `_call(name, on, *args)`: the device guard and the stream both come from `on`,
so a wrapper works on a tensor of a device that is not the current one.  The function is looked up by
name on every call (nothing is cached), so whatever stands in for the library sees each call.
"""
import collections
import ctypes

import torch
import torch.nn.functional as Fn

from . import _lib


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _marshal(args):
    """The arguments as ctypes takes them: a tensor becomes its device pointer, everything else (None: NULL) stays."""
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def _call(name, on, *args):
    """One launch of the entry point `name` on the device of `on` (a tensor or a torch.device), which is made current
    for the call, and on that device's current stream, appended as the last argument; raises on a non-zero status."""
    dev = on.device if isinstance(on, torch.Tensor) else on
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), name)(*_marshal(args), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, name)


def _query(name, *ints):
    """A host-side query of integers (`*_workspace_floats`, `*_chunk_channels`, ...): no tensors, no stream, no device."""
    return int(getattr(_lib.lib(), name)(*map(int, ints)))


def _vp(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


def _ptr_array(objs):
    """Host array of the device pointers of `objs` (None: NULL); `_vp` of it is what a `T* const*` argument takes."""
    return (ctypes.c_void_p * len(objs))(*[None if o is None else o.data_ptr() for o in objs])


def _int_array(values, ctype=ctypes.c_int):
    return (ctype * len(values))(*values)


def _ws(n, device):
    """The float32 workspace of a `*_workspace_floats` query (at least one element, so that its pointer is never NULL)."""
    return torch.empty((max(n, 1),), device=device, dtype=torch.float32)


def _ws_n(n, device):
    """(`_ws(n, device)`, n): the two arguments a kernel with a workspace takes."""
    return _ws(n, device), n


def _chk_gpu(who, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: expected a torch.Tensor")
    if not t.is_cuda:
        raise _lib.TpsppError(f"{who}: tensor is on {t.device}; the HIP path needs a GPU tensor (no CPU fallback)")


_F32 = (torch.float32,)
_F32_BF16 = (torch.float32, torch.bfloat16)         # what the bf16 paths take


def _chk(name, t, ndim=None, dtypes=_F32, gpu=True):
    """(`gpu=False`: a host-side query reads shapes and addresses only, so a CPU tensor will do.)"""
    if gpu:
        _chk_gpu(name, t)
    elif not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{name}: expected {' or '.join(str(d)[6:] for d in dtypes)}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got {tuple(t.shape)}")
    return t.contiguous()


def require_gpu(t, who, training=False):
    """Module forwards call this first: the product has no CPU path and no library-kernel path."""
    _chk_gpu(who, t)
    if training:
        raise NotImplementedError(f"{who} (HIP path) is forward-only: call .eval() and run under "
                                  "torch.no_grad() (SURVEY.md section 8f, row F2)")


def warn_detached_once(module, who):
    """Eval mode with autograd enabled and trainable parameters (the usual frozen-BatchNorm fine-tuning set-up): the HIP
    inference path records no graph, so a loss computed from its output has no grad_fn.  Said once per module instead of
    failing silently; `.train()` (or an input that requires grad) selects the PyTorch training graph."""
    if not torch.is_grad_enabled() or getattr(module, "_warned_detached", False):
        return
    if any(p.requires_grad for p in module.parameters()):
        import logging
        logging.getLogger("tps_pp_amd").warning(
            "%s in eval mode with autograd enabled: the HIP inference path records no graph, so no gradient will reach "
            "this module's parameters (call .train() -- forward_train needs it --, or wrap inference in torch.no_grad())", who)
    module._warned_detached = True


def solve_T(inv_delta_C, ctrl):
    """torch.bmm(inv_delta_C.repeat(N,1,1), cat(ctrl, zeros(N,3,2)))  -> (N, F+3, 2)
    (tps_preprocessor.py:273-280, tps_pp.py:484-494)."""
    inv_delta_C, ctrl = _chk("inv_delta_C", inv_delta_C, 2), _chk("ctrl", ctrl, 3)
    N, F, two = ctrl.shape
    if two != 2 or tuple(inv_delta_C.shape) != (F + 3, F + 3):
        raise ValueError("solve_T: shape mismatch")
    T = torch.empty((N, F + 3, 2), device=ctrl.device, dtype=torch.float32)
    _call("tpspp_solve_T", ctrl, inv_delta_C, ctrl, N, F, T)
    return T


def build_grid(P_hat, T, P_xy=None, score=None):
    """torch.bmm(batch_P_hat, T) -> (N, n, 2); with P_xy/score the TPS_PP form
    `cat[1, P, P_hat*(score*0.5+1)] @ T` (tps_preprocessor.py:281, tps_pp.py:467-479,495)."""
    P_hat, T = _chk("P_hat", P_hat, 2), _chk("T", T, 3)
    N, K, _ = T.shape
    F, n = K - 3, P_hat.shape[0]
    if P_xy is not None:
        P_xy = _chk("P_xy", P_xy, 2)
    if score is not None:
        score = _chk("score", score, 3)
        if tuple(score.shape) != (N, n, F):
            raise ValueError("build_grid: score must be (N, n, F)")
    if P_hat.shape[1] != (F if P_xy is not None else F + 3):
        raise ValueError("build_grid: P_hat has the wrong number of columns")
    grid = torch.empty((N, n, 2), device=T.device, dtype=torch.float32)
    _call("tpspp_build_grid", T, P_hat, P_hat.shape[1], P_xy, score, T, N, n, F, grid)
    return grid


def grid_sample(inp, grid, return_idx=False):
    """F.grid_sample(inp, grid, mode='bilinear', padding_mode='border', align_corners=True)
    (tps_preprocessor.py:79-83, tps_pp.py:606-615).  grid: (N, Ho, Wo, 2)."""
    inp, grid = _chk("input", inp, 4), _chk("grid", grid, 4)
    N, C, H, W = inp.shape
    if grid.shape[0] != N or grid.shape[3] != 2:
        raise ValueError("grid_sample: grid must be (N, Ho, Wo, 2)")
    Ho, Wo = int(grid.shape[1]), int(grid.shape[2])
    out = torch.empty((N, C, Ho, Wo), device=inp.device, dtype=torch.float32)
    idx = torch.empty((N, Ho * Wo, 2), device=inp.device, dtype=torch.int32) if return_idx else None
    _call("tpspp_grid_sample", inp, inp, grid, N, C, H, W, Ho, Wo, out, idx)
    return (out, idx) if return_idx else out


def transpose_p_hat(P_hat):
    """(n, cols) -> (cols, n) device copy for the coalesced kernels (one-off, per module buffer)."""
    P_hat = _chk("P_hat", P_hat, 2)
    n, cols = P_hat.shape
    out = torch.empty((cols, n), device=P_hat.device, dtype=torch.float32)
    _call("tpspp_transpose_p_hat", P_hat, P_hat, cols, n, cols, out)
    return out


TABLE_MIRROR4 = 1
SCORE_TRANSPOSED = 2
IO_BF16 = 4              # TPSPP_IO_BF16: in0 / in1 / out0 / out1 are bfloat16
BWD_FIXED_POINT = 16     # TPSPP_BWD_FIXED_POINT: tpspp_warp_bwd accumulates dL/d input in 64-bit fixed point (this call only)
BWD_TWO_KERNELS = 64     # TPSPP_BWD_TWO_KERNELS: tpspp_warp_bwd never takes the classic one-launch form (this call only)
TABLE_PACKED = 8         # TPSPP_TABLE_PACKED: P_hat_t is the head of a prepare_mirror_table() buffer
TABLE_SPAN = 32          # TPSPP_TABLE_SPAN: ... of the current three-section layout (the span-staging kernel reads the third)


def prepare_mirror_table(P_hat, out_hw):
    """One-off preparation of a classic-layout table for the image-pair kernel (`tpspp_prepare_mirror_table`):
    returns `(P_hat_t, flags)` where `P_hat_t` is the usual (F+3, n) transposed table -- a view of the head of a
    larger buffer whose tail is the packed copy -- and `flags` is `TABLE_PACKED`; for a geometry without a
    prepared form: `(transpose_p_hat(P_hat), 0)`.  OR `TABLE_MIRROR4` in once the symmetry has been verified.
    `flags` is `TABLE_PACKED | TABLE_SPAN`: the buffer has the current three-section layout."""
    P_hat = _chk("P_hat", P_hat, 2)
    n, cols = P_hat.shape
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    if n != Ho * Wo:
        raise ValueError("prepare_mirror_table: P_hat must have Ho * Wo rows")
    total = _query("tpspp_prepared_table_floats", Ho, Wo, cols - 3) if cols > 3 else 0
    if total == 0:
        return transpose_p_hat(P_hat), 0
    buf = torch.empty((total,), device=P_hat.device, dtype=torch.float32)
    _call("tpspp_prepare_mirror_table", P_hat, P_hat, cols, Ho, Wo, cols - 3, buf)
    return buf[:cols * n].view(cols, n), TABLE_PACKED | TABLE_SPAN


def _chk_table(who, P_hat, P_hat_t, n, out_hw, table_flags):
    """P_hat_t must be P_hat transposed; with TABLE_PACKED it must be the head of a prepare_mirror_table buffer
    (the kernel reads the packed copy behind it: anything else would be an out-of-bounds read)."""
    P_hat_t = _chk("P_hat_t", P_hat_t, 2)
    if tuple(P_hat_t.shape) != (P_hat.shape[1], n) or P_hat_t.device != P_hat.device:
        raise ValueError(f"{who}: P_hat_t must be P_hat transposed, on the same device")
    if int(table_flags) & TABLE_PACKED:
        need = _query("tpspp_prepared_table_floats", out_hw[0], out_hw[1], P_hat.shape[1] - 3)
        base = P_hat_t._base
        if need == 0 or base is None or base.numel() < need or base.data_ptr() != P_hat_t.data_ptr():
            raise ValueError(f"{who}: TABLE_PACKED needs the P_hat_t that prepare_mirror_table() returned")
    return P_hat_t


def _chk_out(who, name, o, shape, dtype, device):
    """Caller-supplied output buffers reach the kernels as raw pointers: everything is checked here."""
    if not isinstance(o, torch.Tensor) or tuple(o.shape) != tuple(shape) or o.dtype != dtype \
            or o.device != device or not o.is_contiguous():
        got = (tuple(o.shape), o.dtype, str(o.device)) if isinstance(o, torch.Tensor) else type(o)
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got {got}")
    return o


def table_mirror_symmetry(P_hat_host, out_hw, F):
    """1 if the HOST tensor/array `P_hat_host` (n, F+3) has the exact 4-fold mirror symmetry of the
    reference's GridGenerator table (then `table_flags=TABLE_MIRROR4` may be passed to warp)."""
    import numpy as np
    a = np.ascontiguousarray(P_hat_host.detach().cpu().numpy() if isinstance(P_hat_host, torch.Tensor)
                             else P_hat_host, dtype=np.float32)
    if a.ndim != 2 or a.shape[0] != out_hw[0] * out_hw[1]:
        return 0
    return _query("tpspp_table_mirror_symmetry", a.ctypes.data, a.shape[1], out_hw[0], out_hw[1], F)


def _chk_score(who, score, N, n, F, gpu=True):
    """(N, n, F) as the reference produces it, or a transposed VIEW of an (N, F, n) buffer: the latter is what lets lanes
    that own consecutive pixels read the score coalesced.  -> (the contiguous buffer, SCORE_TRANSPOSED | 0)."""
    if not isinstance(score, torch.Tensor) or tuple(score.shape) != (N, n, F):
        raise ValueError(f"{who}: score must be (N, n, F)")
    if score.stride() == (F * n, 1, n) and n > 1 and F > 1:
        return _chk("score", score.transpose(1, 2), 3, gpu=gpu), SCORE_TRANSPOSED      # the underlying (N, F, n) buffer
    return _chk("score", score, 3, gpu=gpu), 0


def _warp_call(who, in0, ctrl, inv_delta_C, P_hat, out_hw, P_xy, score, in1, out0, out1, P_hat_t, table_flags,
               want_grid=False, want_idx=False):
    """The checks of one `tpspp_warp_fwd` call, for `warp` and `WarpPlan` (who): -> (the checked tensors, in argument
    order, that must outlive the launch; the final table_flags; the argument tuple).  `warp` takes bfloat16 images
    (TPSPP_IO_BF16: T, grid and interpolation stay fp32) and allocates the outputs it is not given; a plan works on its
    caller's buffers and is bfloat16 when in0 (and in1) and out0 (and out1) all are -- mixed dtypes raise before anything
    else is looked at."""
    plan = who == "WarpPlan"
    table_flags = int(table_flags)
    io_dtype = torch.float32
    if plan and isinstance(in0, torch.Tensor):
        for nm, t in (("in1", in1), ("out0", out0), ("out1", out1)):
            if isinstance(t, torch.Tensor) and t.dtype != in0.dtype:
                raise TypeError(f"WarpPlan: in0 / in1 / out0 / out1 must share their dtype (all float32 or all bfloat16); "
                                f"in0 is {in0.dtype}, {nm} is {t.dtype}")
    if isinstance(in0, torch.Tensor) and in0.dtype == torch.bfloat16:
        if in1 is not None and in1.dtype != torch.bfloat16:
            raise TypeError("warp: in0 and in1 must share their dtype")
        io_dtype = torch.bfloat16
        table_flags |= IO_BF16
    io = _F32_BF16 if io_dtype == torch.bfloat16 else _F32
    in0, ctrl = _chk("in0", in0, 4, io), _chk("ctrl", ctrl, 3)
    inv_delta_C, P_hat = _chk("inv_delta_C", inv_delta_C, 2), _chk("P_hat", P_hat, 2)
    N, C0, H0, W0 = in0.shape
    F = int(ctrl.shape[1])
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    n = Ho * Wo
    bad_ctrl, bad_inv = ctrl.shape[0] != N or ctrl.shape[2] != 2, tuple(inv_delta_C.shape) != (F + 3, F + 3)
    if plan and (bad_ctrl or bad_inv):
        raise ValueError("WarpPlan: ctrl must be (N, F, 2), inv_delta_C (F+3, F+3)")
    if bad_ctrl:
        raise ValueError("warp: ctrl must be (N, F, 2)")
    if bad_inv:
        raise ValueError("warp: inv_delta_C must be (F+3, F+3)")
    if P_xy is not None:
        P_xy = _chk("P_xy", P_xy, 2)
        if tuple(P_xy.shape) != (n, 2):
            raise ValueError(f"{who}: P_xy must be (n, 2)")
    if tuple(P_hat.shape) != (n, F if P_xy is not None else F + 3):
        raise ValueError(f"{who}: P_hat has shape {tuple(P_hat.shape)}")
    if score is not None:
        score, transposed = _chk_score(who, score, N, n, F)
        table_flags |= transposed
    if P_hat_t is not None:
        P_hat_t = _chk_table(who, P_hat, P_hat_t, n, (Ho, Wo), table_flags)
    elif table_flags & TABLE_PACKED:
        raise ValueError(f"{who}: TABLE_PACKED without P_hat_t")
    dev = in0.device
    if out0 is None and not plan:
        out0 = torch.empty((N, C0, Ho, Wo), device=dev, dtype=io_dtype)
    C1 = H1 = W1 = 0
    if in1 is not None:
        in1 = _chk("in1", in1, 4, io)
        _, C1, H1, W1 = in1.shape
        if plan and (in1.shape[0] != N or in1.device != dev):
            raise ValueError("WarpPlan: in1 must have in0's batch size and device")
        if in1.shape[0] != N:
            raise ValueError("warp: in1 batch mismatch")
        if in1.device != dev:
            raise ValueError("warp: in1 must be on in0's device")
        if out1 is None and not plan:
            out1 = torch.empty((N, C1, Ho, Wo), device=dev, dtype=io_dtype)
        _chk_out(who, "out1", out1, (N, C1, Ho, Wo), io_dtype, dev)
    elif out1 is not None:
        raise ValueError(f"{who}: out1 given without in1")
    _chk_out(who, "out0", out0, (N, C0, Ho, Wo), io_dtype, dev)
    for nm, t in (("ctrl", ctrl), ("inv_delta_C", inv_delta_C), ("P_hat", P_hat), ("P_xy", P_xy), ("score", score)):
        if t is not None and t.device != dev:
            raise ValueError(f"{who}: {nm} must be on in0's device")
    grid = torch.empty((N, n, 2), device=dev, dtype=torch.float32) if want_grid else None
    idx = torch.empty((N, n, 2), device=dev, dtype=torch.int32) if want_idx else None
    args = (_ptr(in0), C0, H0, W0, _ptr(in1), C1, H1, W1, _ptr(ctrl), _ptr(score), _ptr(inv_delta_C), _ptr(P_hat),
            P_hat.shape[1], _ptr(P_xy), _ptr(P_hat_t), table_flags, N, F, Ho, Wo, _ptr(out0), _ptr(out1), _ptr(grid),
            _ptr(idx), _stream(in0))
    return (in0, in1, ctrl, score, inv_delta_C, P_hat, P_xy, P_hat_t, out0, out1, grid, idx), table_flags, args


def warp(in0, ctrl, inv_delta_C, P_hat, out_hw, P_xy=None, score=None, in1=None,
         want_grid=False, want_idx=False, out0=None, out1=None, P_hat_t=None, table_flags=0):
    """Fused build_P_prime + grid_sample(s): one kernel, T in LDS, grid in registers.

    Returns (out0, out1 | None, grid | None, idx | None).
    classic:  in0 = image, P_hat = GridGenerator.P_hat (n, F+3)     (tps_preprocessor.py:71-83)
    TPS_PP :  in0 = feat_grid, in1 = x, P_hat (n, F) + P_xy (n, 2) + score (N, n, F)
                                                                     (tps_pp.py:597-615)
    bfloat16 in0 / in1 give bfloat16 outputs (TPSPP_IO_BF16)."""
    keep, _, args = _warp_call("warp", in0, ctrl, inv_delta_C, P_hat, out_hw, P_xy, score, in1, out0, out1, P_hat_t,
                               table_flags, want_grid, want_idx)
    with torch.cuda.device(keep[0].device):
        rc = _lib.lib().tpspp_warp_fwd(*args)
    _lib.check(rc, "tpspp_warp_fwd")
    return keep[8:]


class WarpPlan:
    """A validated, pre-marshalled `tpspp_warp_fwd` call on fixed buffers: `ops.warp` checks its tensors and
    marshals 25 arguments on every call (~12 us of Python, about one launch period of the classic geometry);
    a caller that rectifies batch after batch into the same buffers (a serving loop, bench.py) builds the
    plan once and pays one foreign call per batch.  The tensors are kept alive by the plan; the launch goes to
    the stream that was current on `in0.device` when the plan was built, and that device must be the
    thread's current device when `run()` is called (one process per GPU: always true)."""

    def __init__(self, in0, ctrl, inv_delta_C, P_hat, out_hw, out0, P_xy=None, score=None, in1=None, out1=None,
                 P_hat_t=None, table_flags=0):
        self._keep, _, self._args = _warp_call("WarpPlan", in0, ctrl, inv_delta_C, P_hat, out_hw, P_xy, score, in1, out0,
                                               out1, P_hat_t, table_flags)
        self.out0, self.out1 = out0, out1
        self._dev = self._keep[0].device
        # round 6: the arguments live on the library's side (tpspp_warp_plan_create); run() hands over one pointer instead of
        # marshalling 25 arguments per launch (1.6 of ~4.3 us of host time per call)
        L = _lib.lib()
        handle = ctypes.c_void_p()
        _lib.check(L.tpspp_warp_plan_create(*self._args, ctypes.byref(handle)), "tpspp_warp_plan_create")
        self._handle, self._run, self._run_on, self._destroy = handle, L.tpspp_warp_plan_run, L.tpspp_warp_plan_run_on, L.tpspp_warp_plan_destroy

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None and getattr(self, "_destroy", None) is not None:
            try:
                self._destroy(h)
            except Exception:                                  # noqa: BLE001  (interpreter shutdown)
                pass

    def run(self, stream=None):
        """One launch on the stream that was current when the plan was built; pass `stream` (a torch.cuda.Stream)
        to launch on another one (the caller orders the buffers' producers / consumers on it)."""
        if stream is not None:
            rc = self._run_on(self._handle, ctypes.c_void_p(stream.cuda_stream))
        else:
            rc = self._run(self._handle)
        if rc != 0:
            _lib.check(rc, "tpspp_warp_fwd")
        return self.out0, self.out1


class ConvWeight:
    """Device-side weights of one fused convolution, prepared once: `wt` (K, Cout) for the generic
    kernel, `tiled` [chunk][tap][channel-in-chunk][Cout] for the tiled kernel, `bias` (Cout) | None."""

    def __init__(self, wt, tiled, bias, kernel, post_scale=None, post_shift=None):
        self.wt, self.tiled, self.bias, self.kernel = wt, tiled, bias, kernel
        self.post_scale, self.post_shift = post_scale, post_shift


def bn_tensors(bn):
    """(gamma, beta, mean, var) of an nn.BatchNorm2d, as the `bn` / `post_bn` arguments of `prep_conv_weight[_bf16]`."""
    return bn.weight, bn.bias, bn.running_mean, bn.running_var


def _fold_bn(weight, bn, conv_bias, eps, post_bn):
    """fp32 (w, b | None, post_scale | None, post_shift | None): an eval-mode BatchNorm (gamma, beta, mean, var) folded
    into the convolution, y = gamma * (conv(x) + b - mean) / sqrt(var + eps) + beta; `post_bn`: a BatchNorm that FOLLOWS
    the activation, as the per-channel affine of the epilogue."""
    w = weight.detach().float()
    b = None if conv_bias is None else conv_bias.detach().float()
    if bn is not None:
        gamma, beta, mean, var = (t.detach().float() for t in bn)
        scale = gamma / torch.sqrt(var + eps)
        w = w * scale.view(-1, 1, 1, 1)
        b = beta - mean * scale if b is None else beta + (b - mean) * scale
    ps = pb = None
    if post_bn is not None:
        gamma, beta, mean, var = (t.detach().float() for t in post_bn)
        ps = (gamma / torch.sqrt(var + eps)).contiguous()
        pb = (beta - mean * ps).contiguous()
    return w, None if b is None else b.contiguous(), ps, pb


def _hi_lo(w):
    """The two bf16 terms of the three-term split ("bf16x3") of an fp32 weight: hi = bf16(w), lo = bf16(w - hi)."""
    hi = w.to(torch.bfloat16)
    return hi, (w - hi.float()).to(torch.bfloat16)


def prep_conv_weight(weight, bn=None, conv_bias=None, eps=1e-5, src_channels=None, post_bn=None):
    """PyTorch conv weight (Cout, Cin, KH, KW) [+ eval-mode BatchNorm (gamma, beta, mean, var), folded: `_fold_bn`]
    -> ConvWeight.
    `src_channels`: channel counts of the concatenated sources (chunks never straddle a source).
    `post_bn`: a BatchNorm that FOLLOWS the activation (applied as a per-channel affine in the epilogue)."""
    w, b, ps, pb = _fold_bn(weight, bn, conv_bias, eps, post_bn)
    cout, cin, kh, kw = w.shape
    wt = w.reshape(cout, -1).t().contiguous()
    kc = _query("tpspp_conv_chunk_channels", kh)
    tiled = None
    if src_channels is None or len(src_channels) == 1 or all(c % kc == 0 for c in src_channels):
        nch = (cin + kc - 1) // kc
        wp = torch.zeros((cout, nch * kc, kh, kw), device=w.device, dtype=torch.float32)
        wp[:, :cin] = w
        # (cout, chunk, ci, ky, kx) -> (chunk, ky, kx, ci, cout)
        tiled = wp.view(cout, nch, kc, kh, kw).permute(1, 3, 4, 2, 0).contiguous()
    return ConvWeight(wt, tiled, b, kh, ps, pb)


def _split_sources(srcs):
    """srcs entries `map` or `(map, uh, uw)` -> [(map, uh, uw)]."""
    return [tuple(e) if isinstance(e, (tuple, list)) else (e, 1, 1) for e in srcs]


def _conv_sources(who, srcs, label="conv source", layouts=False):
    """The sources of one convolution -> (contiguous tensors, flat src_dims, N, device, Hi, Wi).  src_dims holds
    {C, H, W, uh, uw} per source; layouts (the bf16 form): float32 / bfloat16 NCHW tensors and `Blocked` maps, with the
    layout code as a sixth entry.  Every source reaches the kernel as a raw pointer with only those numbers: batch size,
    device and the shared logical size (H*uh, W*uw) are checked here."""
    ts, dims = [], []
    for t, uh, uw in _split_sources(srcs):
        code = [_layout_code(t)] if layouts else []
        t = _BlkView(t) if layouts and isinstance(t, Blocked) else _chk(label, t, 4, _F32_BF16 if layouts else _F32)
        ts.append(t)
        dims += [t.shape[1], t.shape[2], t.shape[3], int(uh), int(uw)] + code
    per = 6 if layouts else 5
    N, dev = ts[0].shape[0], ts[0].device
    Hi, Wi = ts[0].shape[2] * dims[3], ts[0].shape[3] * dims[4]
    for i, t in enumerate(ts):
        uh, uw = dims[per * i + 3], dims[per * i + 4]
        if t.shape[0] != N or t.device != dev:
            raise ValueError(f"{who}: source {i} must have the first source's batch size and device")
        if uh < 1 or uw < 1 or (t.shape[2] * uh, t.shape[3] * uw) != (Hi, Wi):
            raise ValueError(f"{who}: source {i} does not have the shared logical size {(Hi, Wi)}")
    if not 1 <= len(ts) <= 3:
        raise ValueError(f"{who}: 1..3 sources")
    return ts, dims, N, dev, Hi, Wi


def _conv_out_size(Hi, Wi, kernel, stride):
    """(sh, sw, Ho, Wo) of a "same"-padded convolution."""
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    pad = (kernel - 1) // 2
    return sh, sw, (Hi + 2 * pad - kernel) // sh + 1, (Wi + 2 * pad - kernel) // sw + 1


def conv2d(srcs, cw, stride=(1, 1), relu=True, residual=None, res_mode=0, out=None):
    """Fused conv on the fp32 matrix cores (`tpspp_conv2d_fwd`).

    srcs: list of 1..3 entries `tensor` or `(tensor, uh, uw)`: channel-concatenated, each nearest-
    upsampled by (uh, uw) on the fly.  cw: ConvWeight from `prep_conv_weight` ("same" padding).
    residual/res_mode: 1 = act(conv)+res, 2 = act(conv+res).  relu: False/0 none, True/1 ReLU, 2 GELU (erf)."""
    weight_t, bias, kernel = cw.wt, cw.bias, cw.kernel
    ts, dims, N, dev, Hi, Wi = _conv_sources("conv2d", srcs)
    sh, sw, Ho, Wo = _conv_out_size(Hi, Wi, kernel, stride)
    weight_t = _chk("weight_t", weight_t, 2)
    Cout = weight_t.shape[1]
    if weight_t.shape[0] != sum(t.shape[1] for t in ts) * kernel * kernel:
        raise ValueError("conv2d: weight_t rows != Cin*KH*KW")
    if bias is not None:
        bias = _chk("bias", bias, 1)
    if residual is not None:
        residual = _chk("residual", residual, 4)
        if tuple(residual.shape) != (N, Cout, Ho, Wo) or res_mode not in (1, 2) or residual.device != dev:
            raise ValueError("conv2d: residual shape / device / res_mode")
    elif res_mode != 0:
        raise ValueError("conv2d: res_mode without residual")
    if out is None:
        out = torch.empty((N, Cout, Ho, Wo), device=dev, dtype=torch.float32)
    else:
        _chk_out("conv2d", "out", out, (N, Cout, Ho, Wo), torch.float32, dev)
    if N == 0:          # an empty batch has no device pointer to hand over
        return out
    ptrs, dim_arr = _ptr_array(ts), _int_array(dims)
    _call("tpspp_conv2d_fwd", ts[0], _vp(ptrs), _vp(dim_arr), len(ts), weight_t, cw.tiled, bias, residual, cw.post_scale,
          cw.post_shift, int(res_mode), int(relu), N, Cout, kernel, kernel, sh, sw, out, Ho, Wo)
    return out


def conv2d_route(srcs, cw, stride=(1, 1)):
    """The kernel `conv2d(srcs, cw, stride)` launches (`tpspp_conv2d_route`), as a string: `tiled 3x3 s2x2 4x32 ni1 nb2`
    (output tile, images per tile, accumulators), `generic 3x3 kc8` (channels per chunk), `wide` or `skinny nw16`
    (wavefronts that split K).  A host-side query: only shapes are read, so the maps and the weights may live on any
    device, "meta" included; sizes `conv2d` refuses raise the same error."""
    dims = []
    for t, uh, uw in _split_sources(srcs):
        dims += [t.shape[1], t.shape[2], t.shape[3], int(uh), int(uw)]
    if not 1 <= len(dims) // 5 <= 3:
        raise ValueError("conv2d_route: 1..3 sources")
    N = _split_sources(srcs)[0][0].shape[0]
    k = cw.kernel
    sh, sw, Ho, Wo = _conv_out_size(dims[1] * dims[3], dims[2] * dims[4], k, stride)
    code = _lib.lib().tpspp_conv2d_route(_vp(_int_array(dims)), len(dims) // 5, int(cw.wt is not None),
                                         int(cw.tiled is not None), N, cw.wt.shape[1], k, k, sh, sw, Ho, Wo)
    if code < 0:
        _lib.check(code, "tpspp_conv2d_route")
    family, kk = code & 15, (code >> 4) & 15
    if family == 0:
        return f"generic {kk}x{kk} kc{(code >> 8) & 255}"
    if family == 1:
        return (f"tiled {kk}x{kk} s{(code >> 8) & 15}x{(code >> 12) & 15} {(code >> 16) & 15}x{(code >> 20) & 255} "
                f"ni{((code >> 28) & 1) + 1} nb{((code >> 29) & 1) + 1}")
    return "wide" if family == 2 else f"skinny nw{(code >> 8) & 255}"


# ---- backward of the fused convolution (tpspp_conv_bwd.hip): training the regressor on the HIP kernels -------------
def _bwd_out_size(who, Hi, Wi, kernel, stride):
    """`_conv_out_size` under the rule of the backward kernels: stride 1 or 2, kernel 1x1 or 3x3."""
    sh, sw = (stride, stride) if isinstance(stride, int) else (int(stride[0]), int(stride[1]))
    if sh not in (1, 2) or sw not in (1, 2):
        raise ValueError(f"{who}: stride must be 1 or 2 along each axis, got {(sh, sw)}")
    if kernel not in (1, 3):
        raise ValueError(f"{who}: kernel must be 1x1 or 3x3")
    return _conv_out_size(Hi, Wi, kernel, (sh, sw))


def _chk_grad_out(who, dy, y, relu, shape, dev):
    dy = _chk("dy", dy, 4)
    if tuple(dy.shape) != shape or dy.device != dev:
        raise ValueError(f"{who}: dy must be {shape} on {dev}, got {tuple(dy.shape)} on {dy.device}")
    if relu:
        if y is None:
            raise ValueError(f"{who}: relu=True needs the forward's output y (the mask is y > 0)")
        y = _chk("y", y, 4)
        if tuple(y.shape) != shape or y.device != dev:
            raise ValueError(f"{who}: y must have dy's shape and device")
    else:
        y = None
    return dy, y


def prep_conv_weight_device(weight, bias=None, src_channels=None):
    """ConvWeight for `conv2d` built on the device by `tpspp_conv2d_prep_weight` from PyTorch's (Cout, Cin, KH, KW)
    weight: the training step's form of `prep_conv_weight` (no host-side rearrangement; bias is used as it is)."""
    w = _chk("weight", weight.detach(), 4)
    cout, cin, kh, kw = w.shape
    if kh != kw or kh not in (1, 3):
        raise ValueError("prep_conv_weight_device: kernel must be 1x1 or 3x3")
    kc = _query("tpspp_conv_chunk_channels", kh)
    wt = torch.empty((cin * kh * kw, cout), device=w.device, dtype=torch.float32)
    tiled = None
    if src_channels is None or len(src_channels) == 1 or all(c % kc == 0 for c in src_channels):
        tiled = torch.empty(((cin + kc - 1) // kc, kh * kw, kc, cout), device=w.device, dtype=torch.float32)
    _call("tpspp_conv2d_prep_weight", w, w, cout, cin, kh, kw, wt, tiled)
    b = None if bias is None else _chk("bias", bias.detach(), 1)
    return ConvWeight(wt, tiled, b, kh)


def conv2d_bwd_data(dy, weight, srcs, stride=(1, 1), y=None, relu=True, need=None):
    """Gradients of `conv2d(srcs, ..., relu)` (res_mode 0) with respect to its sources (`tpspp_conv2d_bwd_data`).

    dy (N, Cout, Ho, Wo); weight (Cout, Cin, KH, KW) as PyTorch holds it; srcs as `conv2d` takes them (only their
    shapes and upsampling factors are used); y the forward's output (needed with relu: the mask is y > 0).
    need: per-source flags (default all).  Returns a list with one (N, C_i, H_i, W_i) tensor or None per source."""
    ts, dims, N, dev, Hi, Wi = _conv_sources("conv2d_bwd_data", srcs, "conv2d_bwd_data source")
    w = _chk("weight", weight.detach(), 4)
    cout, cin, kh, kw = w.shape
    if kh != kw or cin != sum(t.shape[1] for t in ts) or w.device != dev:
        raise ValueError("conv2d_bwd_data: weight must be (Cout, sum C_i, K, K) on the sources' device")
    sh, sw, Ho, Wo = _bwd_out_size("conv2d_bwd_data", Hi, Wi, kh, stride)
    dy, y = _chk_grad_out("conv2d_bwd_data", dy, y, relu, (N, cout, Ho, Wo), dev)
    need = [True] * len(ts) if need is None else [bool(v) for v in need]
    outs = [torch.empty_like(t) if nd else None for t, nd in zip(ts, need)]
    if N == 0 or not any(need):
        return outs
    ptrs, dim_arr = _ptr_array(outs), _int_array(dims)
    _call("tpspp_conv2d_bwd_data", dy, _vp(ptrs), _vp(dim_arr), len(ts), w, dy, y, int(bool(relu)), N, cout, kh, kw, sh, sw,
          Ho, Wo)
    return outs


def conv2d_bwd_weight_workspace_floats(srcs_dims, N, Cout, kernel, Ho, Wo):
    """Floats of workspace `conv2d_bwd_weight` needs (`tpspp_conv2d_bwd_weight_workspace_floats`): srcs_dims the flat
    {C, H, W, uh, uw} per source; 0 for N = 0.  The split-K slice count behind it depends on the shapes only."""
    dim_arr = _int_array(srcs_dims)
    return _query("tpspp_conv2d_bwd_weight_workspace_floats", ctypes.addressof(dim_arr), len(srcs_dims) // 5, N, Cout,
                  kernel, kernel, Ho, Wo)


def conv2d_bwd_weight(srcs, dy, kernel, stride=(1, 1), y=None, relu=True, want_weight=True, want_bias=True):
    """Weight and bias gradients of `conv2d(srcs, ..., relu)` (res_mode 0) (`tpspp_conv2d_bwd_weight`): a fixed
    split-K without atomics, bitwise reproducible.  Returns (dW (Cout, Cin, K, K) | None, db (Cout) | None)."""
    ts, dims, N, dev, Hi, Wi = _conv_sources("conv2d_bwd_weight", srcs, "conv2d_bwd_weight source")
    sh, sw, Ho, Wo = _bwd_out_size("conv2d_bwd_weight", Hi, Wi, int(kernel), stride)
    if dy.dim() != 4:
        raise ValueError("conv2d_bwd_weight: dy must be (N, Cout, Ho, Wo)")
    cout, cin = dy.shape[1], sum(t.shape[1] for t in ts)
    dy, y = _chk_grad_out("conv2d_bwd_weight", dy, y, relu, (N, cout, Ho, Wo), dev)
    dw = torch.empty((cout, cin, kernel, kernel), device=dev, dtype=torch.float32) if want_weight else None
    db = torch.empty((cout,), device=dev, dtype=torch.float32) if want_bias else None
    if N == 0:
        if dw is not None:
            dw.zero_()
        if db is not None:
            db.zero_()
        return dw, db
    if dw is None and db is None:
        return dw, db
    nws = conv2d_bwd_weight_workspace_floats(dims, N, cout, int(kernel), Ho, Wo)
    ws = torch.empty((nws,), device=dev, dtype=torch.float32)
    ptrs, dim_arr = _ptr_array(ts), _int_array(dims)
    _call("tpspp_conv2d_bwd_weight", dy, _vp(ptrs), _vp(dim_arr), len(ts), dy, y, int(bool(relu)), N, cout, int(kernel),
          int(kernel), sh, sw, Ho, Wo, dw, db, ws, nws)
    return dw, db


class _ConvFunction(torch.autograd.Function):
    """Differentiable `conv2d` (res_mode 0): HIP forward (`tpspp_conv2d_fwd`), HIP backward (`tpspp_conv2d_bwd_data`,
    `tpspp_conv2d_bwd_weight`).  Saves the sources, the weight and the output y (the ReLU mask is y > 0)."""

    @staticmethod
    def forward(ctx, weight, bias, cfg, *ts):
        ups, stride, relu, cw = cfg
        if cw is None:
            cw = prep_conv_weight_device(weight, bias, [t.shape[1] for t in ts])
        entries = [(t, uh, uw) for t, (uh, uw) in zip(ts, ups)]
        y = conv2d(entries, cw, stride, relu=relu)
        ctx.cfg = (ups, stride, relu, weight.shape[-1], bias is not None)
        ctx.save_for_backward(weight, y, *ts)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        ups, stride, relu, kernel, has_bias = ctx.cfg
        weight, y, *ts = ctx.saved_tensors
        need = ctx.needs_input_grad
        gy = gy.float().contiguous()
        entries = [(t, uh, uw) for t, (uh, uw) in zip(ts, ups)]
        dsrc = [None] * len(ts)
        if any(need[3:]):
            dsrc = conv2d_bwd_data(gy, weight, entries, stride, y=y, relu=relu, need=need[3:])
        dw = db = None
        if need[0] or (has_bias and need[1]):
            dw, db = conv2d_bwd_weight(entries, gy, kernel, stride, y=y, relu=relu, want_weight=need[0],
                                       want_bias=has_bias and need[1])
        return (dw, db, None, *dsrc)


def conv2d_autograd(srcs, weight, bias, stride=(1, 1), relu=True, cw=None):
    """`conv2d` inside an autograd graph: y = act(conv(cat_c(up(src_i)), weight) + bias), act ReLU or none.

    srcs as `conv2d` takes them (tensors or (tensor, uh, uw)); weight (Cout, Cin, K, K) and bias (Cout) | None are the
    layer's parameters (gradients reach them); cw: the forward's ConvWeight prepared from them (a cache the caller keys on
    the parameters' versions), built on the device here if None.  The backward honours `needs_input_grad`: no data-gradient
    launch when no source needs one, no weight-gradient launch for a frozen layer."""
    if not 1 <= len(srcs) <= 3:
        raise ValueError("conv2d_autograd: 1..3 sources")
    ts, ups = [], []
    for t, uh, uw in _split_sources(srcs):
        if not isinstance(t, torch.Tensor):
            raise TypeError("conv2d_autograd: expected tensors")
        _chk_gpu("conv2d_autograd", t)
        ts.append(t)
        ups.append((int(uh), int(uw)))
    _chk("weight", weight, 4)
    if bias is not None:
        _chk("bias", bias, 1)
    if relu not in (0, 1, False, True):
        raise ValueError("conv2d_autograd: relu must be True (ReLU) or False (none)")
    st = (stride, stride) if isinstance(stride, int) else (int(stride[0]), int(stride[1]))
    return _ConvFunction.apply(weight, bias, (tuple(ups), st, int(bool(relu)), cw), *ts)


class ConvWeightBf16:
    """Device-side weights of one fused bf16 convolution: `arranged` bf16
    [Cout/64][Cin/KC][taps][KC/8][64][8] (include/tpspp.h, tpspp_conv2d_bf16_fwd), fp32 `bias` | None."""

    def __init__(self, arranged, bias, kernel, cin, cout, post_scale=None, post_shift=None, x3=False):
        self.arranged, self.bias, self.kernel, self.cin, self.cout = arranged, bias, kernel, cin, cout
        self.post_scale, self.post_shift, self.x3 = post_scale, post_shift, x3


def prep_conv_weight_bf16(weight, bn=None, conv_bias=None, eps=1e-5, post_bn=None, x3=False):
    """PyTorch conv weight (Cout, Cin, KH, KW) [+ eval-mode BatchNorm folded in fp32, then rounded] ->
    ConvWeightBf16.  Same folding rules as `prep_conv_weight`.  x3: the "bf16x3" split (hi and lo slabs per chunk)."""
    w, b, ps, pb = _fold_bn(weight, bn, conv_bias, eps, post_bn)
    cout, cin, kh, kw = w.shape
    kc = _query("tpspp_conv_bf16_chunk_channels", kh)
    ct, nch = (cout + 63) // 64, (cin + kc - 1) // kc
    wp = torch.zeros((ct * 64, nch * kc, kh, kw), device=w.device, dtype=torch.float32)
    wp[:cout, :cin] = w
    # (ctile, co, chunk, kgroup, k8, ky, kx) -> (ctile, chunk, ky, kx, kgroup, co, k8)
    arranged = wp.view(ct, 64, nch, kc // 8, 8, kh, kw).permute(0, 2, 5, 6, 3, 1, 4).contiguous()
    if x3:          # [ctile][chunk][hi|lo][tap...]
        arranged = torch.stack(_hi_lo(arranged), dim=2).contiguous()
    else:
        arranged = arranged.to(torch.bfloat16)
    return ConvWeightBf16(arranged, b, kh, cin, cout, ps, pb, x3)


class Blocked:
    """A bf16 feature map in the blocked layout (N, C/8, H, W, 8) -- the eight channels of a group next to each other
    per pixel -- that the bf16 convolutions exchange among themselves (`tpspp_conv2d_bf16_fwd`, layout code 2: a
    16-byte unit of it is a unit of the kernel's LDS patch).  `shape` is the logical (N, C, H, W)."""

    _dtype = torch.bfloat16

    def __init__(self, t):
        if t.dtype != self._dtype or t.dim() != 5 or t.shape[4] != 8 or not t.is_contiguous():
            raise ValueError(f"{type(self).__name__}: needs a contiguous {str(self._dtype)[6:]} (N, C/8, H, W, 8) tensor")
        self.t = t
        self.shape = (t.shape[0], t.shape[1] * 8, t.shape[2], t.shape[3])
        self.dtype, self.device = t.dtype, t.device
        self.requires_grad, self.is_cuda = False, t.is_cuda      # (a product of the HIP inference kernels: no autograd graph)

    @classmethod
    def from_nchw(cls, x):
        n, c, h, w = x.shape
        return cls(x.to(cls._dtype).reshape(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous())

    def nchw(self):
        n, c, h, w = self.shape
        return self.t.permute(0, 1, 4, 2, 3).reshape(n, c, h, w).contiguous()

    def nchw_hip(self):
        """`tpspp_blocked_to_nchw_bf16`: the same tensor as `nchw()` by a HIP kernel (the product path; `nchw()` is a
        PyTorch composition for tests and edges); the result remembers its blocked twin (`_tpspp_blocked`) so that a
        convolution further on can take the cheaper source."""
        n, c, h, w = self.shape
        if not self.t.is_cuda or (h * w) % 64:
            raise _lib.TpsppError("Blocked.nchw_hip: needs a GPU tensor with H * W a multiple of 64 (no CPU fallback)")
        out = torch.empty((n, c, h, w), device=self.t.device, dtype=torch.bfloat16)
        _call("tpspp_blocked_to_nchw_bf16", self.t, self.t, n, c, h * w, out)
        out._tpspp_blocked = self
        return out

    def data_ptr(self):
        return self.t.data_ptr()


class Blocked32(Blocked):
    """The blocked layout in float32, (N, C/8, H, W, 8) fp32 -- what the maps of the three-term-split ("bf16x3") configuration
    use between convolutions (layout code 3: a patch position's 8 channels are two 16-byte loads instead of eight 4-byte
    loads from eight planes)."""

    _dtype = torch.float32


def _layout_code(t):
    if isinstance(t, Blocked32):
        return 3
    return 2 if isinstance(t, Blocked) else int(t.dtype == torch.float32)


def conv2d_bf16(srcs, cw, stride=(1, 1), relu=True, residual=None, res_mode=0, out_dtype=torch.bfloat16, out_blocked=False):
    """Fused conv on the bf16 matrix cores (`tpspp_conv2d_bf16_fwd`): same call shape as `conv2d`; every
    source / the residual may be float32 or bfloat16 NCHW or a `Blocked` bf16 map, the output is `out_dtype`
    (`out_blocked`: a `Blocked` bf16 map, for layers that only feed other convolutions)."""
    ts, dims, N, dev, Hi, Wi = _conv_sources("conv2d_bf16", srcs, layouts=True)
    if sum(t.shape[1] for t in ts) != cw.cin:
        raise ValueError("conv2d_bf16: source channels != Cin of the weight")
    kernel, Cout = cw.kernel, cw.cout
    sh, sw, Ho, Wo = _conv_out_size(Hi, Wi, kernel, stride)
    res_code = 0
    if residual is not None:
        if not isinstance(residual, Blocked):
            residual = _chk("residual", residual, 4, _F32_BF16)
        if tuple(residual.shape) != (N, Cout, Ho, Wo) or res_mode not in (1, 2) or residual.device != dev:
            raise ValueError("conv2d_bf16: residual shape / device / res_mode")
        res_code = _layout_code(residual)
    elif res_mode != 0:
        raise ValueError("conv2d_bf16: res_mode without residual")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("conv2d_bf16: out_dtype must be float32 or bfloat16")
    if out_blocked:
        if Cout % 8:
            raise ValueError("conv2d_bf16: a blocked output needs a multiple of 8 channels")
        if cw.x3:                                   # the three-term split: fp32 maps, fp32 blocked
            if out_dtype != torch.float32:
                raise ValueError("conv2d_bf16: with x3 weights a blocked output is float32 (Blocked32)")
            out = Blocked32(torch.empty((N, Cout // 8, Ho, Wo, 8), device=dev, dtype=torch.float32))
        else:
            if out_dtype != torch.bfloat16:
                raise ValueError("conv2d_bf16: a blocked output is bfloat16 (float32 with x3 weights)")
            out = Blocked(torch.empty((N, Cout // 8, Ho, Wo, 8), device=dev, dtype=torch.bfloat16))
    else:
        out = torch.empty((N, Cout, Ho, Wo), device=dev, dtype=out_dtype)
    codes = list(dims[5::6]) + [res_code]
    if (cw.x3 and 2 in codes) or (not cw.x3 and 3 in codes):
        raise ValueError("conv2d_bf16: Blocked (bfloat16) maps go with plain bf16 weights, Blocked32 (float32) maps with x3 weights")
    if N == 0:          # an empty batch has no device pointer to hand over
        return out
    ptrs, dim_arr = _ptr_array(ts), _int_array(dims)
    first = ts[0].keep if isinstance(ts[0], _BlkView) else ts[0]
    _call("tpspp_conv2d_bf16_fwd", first, _vp(ptrs), _vp(dim_arr), len(ts), cw.arranged, cw.bias,
          residual.data_ptr() if residual is not None else None, res_code, cw.post_scale, cw.post_shift, int(res_mode),
          int(relu), N, Cout, kernel, kernel, sh, sw, out.data_ptr(),
          (3 if cw.x3 else 2) if out_blocked else int(out_dtype == torch.float32), Ho, Wo, int(cw.x3))
    return out


_ROUTE_BASE = 1 << 20         # stands for the (512-byte aligned) start of an allocation where a tensor has no memory


def _route_ptr(t):
    """The address `conv2d_bf16_route` judges a tensor by: its own, or, for a tensor without memory ("meta"), its offset
    from an aligned allocation.  None stays NULL."""
    if t is None:
        return None
    t = t.t if isinstance(t, Blocked) else t
    return t.data_ptr() or _ROUTE_BASE + t.storage_offset() * t.element_size()


_BF16_FAMILIES = ("tiled", "tiled-x3", "wide3", "wide1", "stem", "persist", "blk1")


def conv2d_bf16_route_name(code):
    """The packed code of `tpspp_conv2d_bf16_route` (include/tpspp.h) as a string: `tiled 3x3 s1x1 4x64 ni1 nf2 wide1 nb2`,
    `tiled-x3 1x1 s2x2 4x16 ni2 nf1 wide0 nb1`, `persist 3x3 s2x2 2x64 ni1 nf1 wres1 epi0 cpb2`, `wide3 3x3 s1x1 8x32 ni1 nf4
    epi1`, `wide1 1x1 s1x1 4x16 ni4 nf4 epi3`, `stem 3x3 s1x1 4x128 ni1 nf4 blocked0`, `blk1 1x1 s1x1 nt2 nks4 sl1 nw8`."""
    fam = _BF16_FAMILIES[code & 7]
    k = 3 if (code >> 3) & 1 else 1
    head = f"{fam} {k}x{k} s{(code >> 4) & 3}x{(code >> 6) & 3}"
    if fam == "blk1":
        return f"{head} nt{(code >> 8) & 15} nks{(code >> 12) & 31} sl{(code >> 17) & 3} nw{(code >> 19) & 15}"
    head += f" {(code >> 8) & 31}x{(code >> 13) & 511} ni{(code >> 22) & 7} nf{((code >> 25) & 3) + 1}"
    if fam in ("tiled", "tiled-x3"):
        return f"{head} wide{(code >> 27) & 1} nb{((code >> 28) & 1) + 1}"
    if fam == "persist":
        return f"{head} wres{(code >> 27) & 1} epi{(code >> 28) & 3} cpb{((code >> 30) & 1) + 1}"
    if fam == "stem":
        return f"{head} blocked{(code >> 27) & 1}"
    return f"{head} epi{(code >> 27) & 3}"


def conv2d_bf16_route(srcs, cw, stride=(1, 1), relu=True, residual=None, res_mode=0, out_dtype=torch.bfloat16, out_blocked=False):
    """The kernel `conv2d_bf16` launches for the same arguments (`tpspp_conv2d_bf16_route`), as a string
    (`conv2d_bf16_route_name`).  A host-side query: shapes, layouts and the 16-byte alignment of sources and weight are all
    it reads, so the tensors may live on any device, "meta" included (judged as their offset into an aligned allocation);
    the output is judged as `conv2d_bf16` allocates it, aligned.  What `conv2d_bf16` refuses raises the same error."""
    ents = _split_sources(srcs)
    if not 1 <= len(ents) <= 3:
        raise ValueError("conv2d_bf16_route: 1..3 sources")
    dims = []
    for t, uh, uw in ents:
        dims += [t.shape[1], t.shape[2], t.shape[3], int(uh), int(uw), _layout_code(t)]
    N = ents[0][0].shape[0]
    if sum(dims[0::6]) != cw.cin:
        raise ValueError("conv2d_bf16_route: source channels != Cin of the weight")
    sh, sw, Ho, Wo = _conv_out_size(dims[1] * dims[3], dims[2] * dims[4], cw.kernel, stride)
    if (residual is None) != (res_mode == 0):
        raise ValueError("conv2d_bf16_route: residual / res_mode")
    res_code = 0 if residual is None else _layout_code(residual)
    out_code = (3 if cw.x3 else 2) if out_blocked else int(out_dtype == torch.float32)
    ptrs = (ctypes.c_void_p * len(ents))(*[_route_ptr(t) for t, _, _ in ents])
    code = _lib.lib().tpspp_conv2d_bf16_route(
        _vp(ptrs), _vp(_int_array(dims)), len(ents), _route_ptr(cw.arranged), _route_ptr(cw.bias), _route_ptr(residual), res_code,
        _route_ptr(cw.post_scale), _route_ptr(cw.post_shift), int(res_mode), int(relu), N, cw.cout, cw.kernel, cw.kernel, sh, sw,
        _ROUTE_BASE, out_code, Ho, Wo, int(cw.x3))
    if code < 0:
        _lib.check(code, "tpspp_conv2d_bf16_route")
    return conv2d_bf16_route_name(code)


class _BlkView:
    """What the shared source checks look at (logical shape, device, is_cuda, dtype, data_ptr) for a `Blocked` map."""

    def __init__(self, b):
        self.shape, self.device, self.dtype, self.is_cuda = b.shape, b.device, b.dtype, b.t.is_cuda
        self.keep = b.t

    def data_ptr(self):
        return self.keep.data_ptr()


def _mfma_feature_perm(device):
    """slot 2*ks + half -> input feature held by (accumulator register ks, half-wavefront `half`) in the
    C/D layout of v_mfma_f32_32x32x2_f32 (see tpspp_dgab.hip)."""
    perm = []
    for ks in range(32):
        for half in range(2):
            perm.append(32 * (ks >> 4) + (ks & 3) + 8 * ((ks & 15) >> 2) + 4 * half)
    return torch.tensor(perm, device=device, dtype=torch.long)


class DgabWeights:
    def __init__(self, blk):
        """blk: the DGAB module (norm1, attn.{mlp_h,mlp_w,proj}, norm2, mlp.{fc1,fc2})."""
        f = lambda t: t.detach().float().contiguous()
        dev = blk.norm1.weight.device
        perm = _mfma_feature_perm(dev)
        self.ln1_w, self.ln1_b = f(blk.norm1.weight), f(blk.norm1.bias)
        self.ln2_w, self.ln2_b = f(blk.norm2.weight), f(blk.norm2.bias)
        self.mw_t = f(blk.attn.mlp_w[0].weight.t())              # (96, 65)
        self.mh_t = f(blk.attn.mlp_h[0].weight.t())              # (48, 17)
        self.proj_slab = f(blk.attn.proj.weight[:, perm].t())    # [slot][out]
        self.proj_b = f(blk.attn.proj.bias)
        w1, w2 = blk.mlp.fc1.weight.detach().float(), blk.mlp.fc2.weight.detach().float()
        self.fc1_slab = torch.stack([w1[hb * 64:(hb + 1) * 64][:, perm].t() for hb in range(4)]).contiguous()
        self.fc2_slab = torch.stack([w2[:, hb * 64 + perm].t() for hb in range(4)]).contiguous()
        self.fc1_b, self.fc2_b = f(blk.mlp.fc1.bias), f(blk.mlp.fc2.bias)


def dgab(x, y, dw):
    """DGAB.forward (DGAB.py:74-77) fused: x (N, C, 16, 64), y (N, C, 32) -> (N, C, 16, 64)."""
    x, y = _chk("x", x, 4), _chk("y", y, 3)
    N, C, H, W = x.shape
    if (H, W) != (16, 64) or tuple(y.shape) != (N, C, 32):
        raise ValueError("dgab: needs x (N, C, 16, 64) and y (N, C, 32)")
    out = torch.empty_like(x)
    scratch = torch.empty_like(x)
    _call("tpspp_dgab_fwd", x, x, y, dw.ln1_w, dw.ln1_b, dw.mw_t, dw.mh_t, dw.proj_slab, dw.proj_b, dw.ln2_w, dw.ln2_b,
          dw.fc1_slab, dw.fc1_b, dw.fc2_slab, dw.fc2_b, scratch, out, N, C)
    return out


_PERM16 = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


def _bf16_slab(w, chain, x3=False):
    """(out 64, K) fp32 -> [K/16][2][64][8] bf16 A-operand slab of v_mfma_f32_32x32x16_bf16; `chain`: k-slots in the
    order in which the previous layer's result registers come back as operands (include/tpspp.h).  x3: the hi and lo
    halves of the three-term split, stacked [hi|lo][K/16][2][64][8]."""
    cout, cin = w.shape
    idx = torch.arange(cin, device=w.device).view(cin // 16, 16)
    if chain:
        idx = idx[:, torch.tensor(_PERM16, device=w.device)]
    a = w[:, idx.reshape(-1)].view(cout, cin // 16, 2, 8).permute(1, 2, 0, 3).contiguous()
    return torch.stack(_hi_lo(a)).contiguous() if x3 else a.to(torch.bfloat16)


class DgabWeightsBf16:
    def __init__(self, blk, x3=False):
        """blk: the DGAB module.  Slabs for tpspp_dgab_bf16_fwd (x3: hi + lo halves, split3)."""
        self.x3 = x3
        f = lambda t: t.detach().float().contiguous()          # noqa: E731
        self.ln1_w, self.ln1_b = f(blk.norm1.weight), f(blk.norm1.bias)
        self.ln2_w, self.ln2_b = f(blk.norm2.weight), f(blk.norm2.bias)
        self.mw_t = f(blk.attn.mlp_w[0].weight.t())
        self.mh_t = f(blk.attn.mlp_h[0].weight.t())
        self.proj_slab = _bf16_slab(f(blk.attn.proj.weight), False, x3)
        self.proj_b = f(blk.attn.proj.bias)
        w1, w2 = f(blk.mlp.fc1.weight), f(blk.mlp.fc2.weight)
        self.fc1_slab = torch.stack([_bf16_slab(w1[hb * 64:(hb + 1) * 64], True, x3) for hb in range(4)]).contiguous()
        self.fc2_slab = torch.stack([_bf16_slab(w2[:, hb * 64:(hb + 1) * 64], True, x3) for hb in range(4)]).contiguous()
        self.fc1_b, self.fc2_b = f(blk.mlp.fc1.bias), f(blk.mlp.fc2.bias)


def dgab_bf16(x, y, dw):
    """`dgab` with proj / fc1 / fc2 on the bf16 matrix cores (fp32 in, fp32 out)."""
    x, y = _chk("x", x, 4), _chk("y", y, 3)
    N, C, H, W = x.shape
    if (H, W) != (16, 64) or tuple(y.shape) != (N, C, 32):
        raise ValueError("dgab_bf16: needs x (N, C, 16, 64) and y (N, C, 32)")
    out = torch.empty_like(x)
    scratch = torch.empty(x.shape, device=x.device, dtype=torch.float32 if dw.x3 else torch.bfloat16)
    _call("tpspp_dgab_bf16_fwd", x, x, y, dw.ln1_w, dw.ln1_b, dw.mw_t, dw.mh_t, dw.proj_slab, dw.proj_b, dw.ln2_w, dw.ln2_b,
          dw.fc1_slab, dw.fc1_b, dw.fc2_slab, dw.fc2_b, scratch, out, N, C, int(dw.x3))
    return out


class ScoreWeights:
    def __init__(self, feat_linear):
        """feat_linear: nn.Sequential(Linear(64, 32), Linear(32, 128)) (tps_pp.py:257-260)."""
        l1, l2 = feat_linear[0], feat_linear[1]
        dev = l1.weight.device
        perm16 = torch.tensor([(ks & 3) + 8 * (ks >> 2) + 4 * half for ks in range(16) for half in range(2)],
                              device=dev, dtype=torch.long)
        self.w1_slab = l1.weight.detach().float().t().contiguous()              # [64][32]
        self.w2_slab = l2.weight.detach().float()[:, perm16].t().contiguous()   # [32 slots][128]
        self.b1 = l1.bias.detach().float().contiguous()
        self.b2 = l2.bias.detach().float().contiguous()
        # hi / lo slabs of the three-term split (tpspp_score_x3_fwd)
        self.w1_x3 = _bf16_slab(l1.weight.detach().float(), False, True)
        self.w2_x3 = _bf16_slab(l2.weight.detach().float(), True, True)


def score(de_feat, p, sw, scale, x3=False):
    """get_score (tps_pp.py:303-312) fused: de_feat (N, 64, H, W), p (N, 32, 128) -> (N, H*W, 32) as
    the transposed VIEW of an (N, 32, H*W) buffer.  x3: the three-term bf16 split in the three products."""
    de_feat, p = _chk("de_feat", de_feat, 4), _chk("p", p, 3)
    N, C, H, W = de_feat.shape
    if C != 64 or tuple(p.shape) != (N, 32, 128):
        raise ValueError("score: needs de_feat (N, 64, H, W) and p (N, 32, 128)")
    n = H * W
    out = torch.empty((N, 32, n), device=de_feat.device, dtype=torch.float32)
    name, w1, w2 = ("tpspp_score_x3_fwd", sw.w1_x3, sw.w2_x3) if x3 else ("tpspp_score_fwd", sw.w1_slab, sw.w2_slab)
    _call(name, de_feat, de_feat, w1, sw.b1, w2, sw.b2, p, float(scale), out, N, n)
    return out.transpose(1, 2)


class FrontWeights:
    def __init__(self, m):
        """m: TPS_PP (ResNet45v2 wiring): down0, down1, down2, down_feat ConvModules."""
        f = lambda t: t.detach().float().contiguous()
        perm = _mfma_feature_perm(m.down0.conv.weight.device)
        self.w0 = f(m.down0.conv.weight.view(64, 32).t())
        self.w1 = f(m.down1.conv.weight.view(64, 32).t())
        self.w2 = f(m.down2.conv.weight.view(64, 64).t())
        wg = m.down_feat.conv.weight.detach().float().view(64, 192)
        self.wg = torch.stack([wg[:, blk * 64 + perm].t() for blk in range(3)]).contiguous()
        self.b0, self.b1, self.b2, self.bg = (f(c.conv.bias) for c in (m.down0, m.down1, m.down2, m.down_feat))


def front(o0, o1, x, fw, store01=True):
    """down0/down1/down2 + grid() of TPS_PP.forward (tps_pp.py:560-562,581-585) in one kernel.
    Returns (feat0, feat1, feat2, feat_grid); `store01=False`: feat0 / feat1 stay operands of feat_grid and are returned as
    None (`down_fused_f32` recomputes them where they are consumed)."""
    o0, o1, x = _chk("outs[0]", o0, 4), _chk("outs[1]", o1, 4), _chk("x", x, 4)
    N, c0, H, W = o0.shape
    if c0 != 32 or tuple(o1.shape) != (N, 32, H, W) or tuple(x.shape) != (N, 64, H // 2, W // 2):
        raise ValueError("front: needs outs (N,32,H,W) x2 and x (N,64,H/2,W/2)")
    dev = o0.device
    feat_grid = torch.empty((N, 64, H, W), device=dev, dtype=torch.float32)
    feat0 = torch.empty_like(feat_grid) if store01 else None
    feat1 = torch.empty_like(feat_grid) if store01 else None
    feat2 = torch.empty((N, 64, H // 2, W // 2), device=dev, dtype=torch.float32)
    _call("tpspp_front_fwd", o0, o0, o1, x, fw.w0, fw.b0, fw.w1, fw.b1, fw.w2, fw.b2, fw.wg, fw.bg, feat0, feat1, feat2,
          feat_grid, N, H, W)
    return feat0, feat1, feat2, feat_grid


def down_fused_f32_applicable(o, cw):
    """`down_fused_f32` takes a float32 (N, 32, H, 128) map with an even H and a 64 -> 64 3x3 fp32 weight with a bias."""
    return (o.dtype == torch.float32 and o.dim() == 4 and o.shape[1] == 32 and o.shape[2] % 2 == 0 and o.shape[3] == 128
            and cw.kernel == 3 and cw.tiled is not None and tuple(cw.tiled.shape) == (16, 3, 3, 4, 64) and cw.bias is not None
            and cw.post_scale is None)


def down_fused_f32(o, w0_slab, b0, cw, relu=True):
    """`down0_1(down0(outs[0]))` / `down1_1(down1(outs[1]))` of TPS_PP.forward (tps_pp.py:560-563) in one exact-fp32 kernel
    (`tpspp_down_fused_f32_fwd`); `w0_slab`, `b0`: the 1x1 layer as `FrontWeights` holds it; `cw`: the 3x3 stride-2 layer
    (`prep_conv_weight`).  Returns (N, 64, H/2, 64) float32."""
    o = _chk("outs", o, 4)
    if not down_fused_f32_applicable(o, cw):
        raise ValueError("down_fused_f32: needs a float32 (N, 32, H, 128) map with an even H and a 64 -> 64 3x3 weight with a bias")
    N, _, H, W = o.shape
    out = torch.empty((N, 64, H // 2, W // 2), device=o.device, dtype=torch.float32)
    if N == 0:
        return out
    _call("tpspp_down_fused_f32_fwd", o, o, w0_slab, b0, cw.tiled, cw.bias, out, N, H, W, int(relu))
    return out


class FrontWeightsBf16:
    def __init__(self, m, x3=False):
        """m: TPS_PP (ResNet45v2 wiring).  Slabs for tpspp_front_bf16_fwd (include/tpspp.h); x3: hi + lo halves."""
        f = lambda t: t.detach().float().contiguous()          # noqa: E731
        self.x3 = x3
        self.w0 = _bf16_slab(f(m.down0.conv.weight).view(64, 32), False, x3)
        self.w1 = _bf16_slab(f(m.down1.conv.weight).view(64, 32), False, x3)
        self.w2 = _bf16_slab(f(m.down2.conv.weight).view(64, 64), False, x3)
        self.wg = _bf16_slab(f(m.down_feat.conv.weight).view(64, 192), True, x3)
        self.b0, self.b1, self.b2, self.bg = (f(c.conv.bias) for c in (m.down0, m.down1, m.down2, m.down_feat))


def front_bf16_applicable(o0, o1, x, x3=False):
    dt = torch.float32 if x3 else torch.bfloat16
    return all(t.dtype == dt for t in (o0, o1, x)) and o0.shape[2] % 2 == 0 and o0.shape[3] % 32 == 0


def front_bf16(o0, o1, x, fw, feat_grid_dtype=torch.bfloat16, blocked=False, store01=True):
    """`front` on the bf16 matrix cores: bf16 in, bf16 feat0 / feat1 / feat2, feat_grid bf16 or fp32; with x3 weights
    (`FrontWeightsBf16(m, x3=True)`) fp32 in and out, three-term split.  `store01=False` (blocked bf16 only): feat0 / feat1
    stay operands of feat_grid and are returned as None -- `down_fused_bf16` recomputes them where they are consumed."""
    o0, o1, x = (_chk(nm, t, 4, _F32_BF16) for nm, t in (("outs[0]", o0), ("outs[1]", o1), ("x", x)))
    N, c0, H, W = o0.shape
    if c0 != 32 or tuple(o1.shape) != (N, 32, H, W) or tuple(x.shape) != (N, 64, H // 2, W // 2):
        raise ValueError("front_bf16: needs outs (N,32,H,W) x2 and x (N,64,H/2,W/2)")
    if not front_bf16_applicable(o0, o1, x, fw.x3):
        raise ValueError("front_bf16: needs bfloat16 inputs (float32 with x3 weights), an even height and a width that "
                         "is a multiple of 32")
    dev = o0.device
    bf = torch.float32 if fw.x3 else torch.bfloat16
    if fw.x3:
        feat_grid_dtype = torch.float32
    blocked = bool(blocked)                     # feat0 / feat1 / feat2 as `Blocked` / `Blocked32` maps (they only feed convolutions)
    if blocked:
        feat0 = torch.empty((N, 8, H, W, 8), device=dev, dtype=bf)
        feat2 = torch.empty((N, 8, H // 2, W // 2, 8), device=dev, dtype=bf)
    else:
        feat0 = torch.empty((N, 64, H, W), device=dev, dtype=bf)
        feat2 = torch.empty((N, 64, H // 2, W // 2), device=dev, dtype=bf)
    feat1 = torch.empty_like(feat0)
    if not store01:
        if not blocked:
            raise ValueError("front_bf16: store01=False goes with the blocked form")
        feat0 = feat1 = None
    feat_grid = torch.empty((N, 64, H, W), device=dev, dtype=feat_grid_dtype)
    _call("tpspp_front_bf16_fwd", o0, o0, o1, x, fw.w0, fw.b0, fw.w1, fw.b1, fw.w2, fw.b2, fw.wg, fw.bg, feat0, feat1, feat2,
          feat_grid, int(feat_grid_dtype == torch.float32) | (2 if blocked else 0), N, H, W, int(fw.x3))
    if blocked:
        B = Blocked32 if fw.x3 else Blocked
        return (B(feat0), B(feat1), B(feat2), feat_grid) if store01 else (None, None, B(feat2), feat_grid)
    return feat0, feat1, feat2, feat_grid


def token_gemm_bf16(x_cm, cw, act=None, residual=None, out_dtype=torch.float32):
    """`out (Co, M) = act(W^T x + bias) [+ residual]` for channel-major tokens `x_cm` (K, M) float32 on the bf16 matrix cores
    (`tpspp_token_gemm_bf16_fwd`); `cw`: a 1x1 `prep_conv_weight_bf16` weight (x3: the three-term split); act None | "gelu"."""
    x_cm = _chk("x_cm", x_cm, 2)
    K, M = x_cm.shape
    if cw.kernel != 1 or cw.cin != K or cw.post_scale is not None:
        raise ValueError("token_gemm_bf16: needs a 1x1 weight with Cin = x_cm.shape[0] and no post-affine")
    if residual is not None:
        residual = _chk("residual", residual, 2)
        if tuple(residual.shape) != (cw.cout, M):
            raise ValueError("token_gemm_bf16: residual must be (Co, M)")
    if out_dtype not in (torch.float32, torch.bfloat16) or act not in (None, "gelu"):
        raise ValueError("token_gemm_bf16: out_dtype float32 | bfloat16, act None | 'gelu'")
    out = torch.empty((cw.cout, M), device=x_cm.device, dtype=out_dtype)
    _call("tpspp_token_gemm_bf16_fwd", x_cm, x_cm, cw.arranged, cw.bias, residual, out,
          int(out_dtype == torch.float32), K, cw.cout, M, 2 if act == "gelu" else 0, int(cw.x3))
    return out


def down_fused_bf16_applicable(o, cw):
    """`down_fused_bf16` takes a (N, 32, H, 128) map with an even H -- bfloat16 with a plain-bf16 64 -> 64 3x3 weight, float32
    with an x3 (three-term split) weight."""
    return (o.dtype == (torch.float32 if cw.x3 else torch.bfloat16) and o.dim() == 4 and o.shape[1] == 32
            and o.shape[2] % 2 == 0 and o.shape[3] == 128
            and cw.kernel == 3 and cw.cin == 64 and cw.cout == 64 and cw.bias is not None and cw.post_scale is None)


def down_fused_bf16(o, w0_slab, b0, cw, relu=True):
    """`down0_1(down0(outs[0]))` / `down1_1(down1(outs[1]))` of TPS_PP.forward (tps_pp.py:560-563) in one kernel
    (`tpspp_down_fused_bf16_fwd`): the 1x1 result never exists in HBM.  `w0_slab`, `b0`: the 1x1 layer as
    `FrontWeightsBf16` holds it; `cw`: the 3x3 stride-2 layer (`prep_conv_weight_bf16`).  Returns a `Blocked` map."""
    o = _chk("outs", o, 4, _F32_BF16)
    if not down_fused_bf16_applicable(o, cw):
        raise ValueError("down_fused_bf16: needs a (N, 32, H, 128) map with an even H -- bfloat16 with a 64 -> 64 3x3 bf16 weight, "
                         "float32 with an x3 weight -- and a bias")
    N, _, H, W = o.shape
    if cw.x3:                                           # three-term split: fp32 maps, `w0_slab` with its hi and lo halves
        out = Blocked32(torch.empty((N, 8, H // 2, W // 2, 8), device=o.device, dtype=torch.float32))
        name = "tpspp_down_fused_x3_fwd"
    else:
        out = Blocked(torch.empty((N, 8, H // 2, W // 2, 8), device=o.device, dtype=torch.bfloat16))
        name = "tpspp_down_fused_bf16_fwd"
    if N == 0:
        return out
    _call(name, o, o, w0_slab, b0, cw.arranged, cw.bias, out.t, N, H, W, int(relu))
    return out


def cbam(x, atten):
    """CBAM.forward (tps_pp.py:77-82) on the (N, 64, 2, 16) bottleneck map, one fused kernel."""
    x = _chk("x", x, 4)
    if tuple(x.shape[1:]) != (64, 2, 16):
        raise ValueError("cbam: needs (N, 64, 2, 16)")
    f = lambda t: t.detach().float().contiguous()
    ca, sa = atten.channel_attention, atten.spatial_attention
    out = torch.empty_like(x)
    _call("tpspp_cbam_fwd", x, x, f(ca.shared_MLP[0].weight.view(4, 64)), f(ca.shared_MLP[2].weight.view(64, 4)),
          f(sa.conv2d.weight), f(sa.conv2d.bias), out, x.shape[0])
    return out


def tpe_points(en_feat, tpe):
    """localization_fc1/fc2 and p_linear of Transformation_Parameter_Estimation (tps_pp.py:305,321-323)
    on en_feat (N, 64, 2, 16): returns (ctrl (N, 32, 2), p (N, 32, 128))."""
    en_feat = _chk("en_feat", en_feat, 4)
    if tuple(en_feat.shape[1:]) != (64, 2, 16):
        raise ValueError("tpe_points: needs (N, 64, 2, 16)")
    N = en_feat.shape[0]
    f = lambda t: t.detach().float().contiguous()
    l1a, l1b, l2 = tpe.localization_fc1[0], tpe.localization_fc1[2], tpe.localization_fc2
    p0, p1 = tpe.p_linear[0], tpe.p_linear[1]
    ctrl = torch.empty((N, 32, 2), device=en_feat.device, dtype=torch.float32)
    p = torch.empty((N, 32, 128), device=en_feat.device, dtype=torch.float32)
    ws = [f(t) for t in (l1a.weight, l1a.bias, l1b.weight, l1b.bias, l2.weight, l2.bias, p0.weight, p0.bias,
                         p1.weight, p1.bias)]
    _call("tpspp_tpe_points_fwd", en_feat, en_feat, *ws, ctrl, p, N)
    return ctrl, p


def maxpool2x2(x):
    """nn.MaxPool2d(2, 2) (tps_preprocessor.py:110,114,118)."""
    x = _chk("input", x, 4)
    N, C, H, W = x.shape
    out = torch.empty((N, C, H // 2, W // 2), device=x.device, dtype=torch.float32)
    _call("tpspp_maxpool2x2_fwd", x, x, N, C, H, W, out)
    return out


def global_avgpool(x):
    """nn.AdaptiveAvgPool2d(1) -> (N, C) (tps_preprocessor.py:126)."""
    x = _chk("input", x, 4)
    N, C, H, W = x.shape
    out = torch.empty((N, C), device=x.device, dtype=torch.float32)
    _call("tpspp_global_avgpool_fwd", x, x, N, C, H, W, out)
    return out


def linear(x, cw, relu=False):
    """y = act(x @ W^T + b) for x (N, Cin) on the conv kernel: the batch plays the role of the pixels
    of a 1x1 convolution over a (1, Cin, 1, N) image.  cw = prep_conv_weight(W.view(Cout, Cin, 1, 1), conv_bias=b).
    Returns (N, Cout)."""
    x = _chk("input", x, 2)
    n, cin = x.shape
    xt = x.t().contiguous().view(1, cin, 1, n)
    y = conv2d([xt], cw, 1, relu)                      # (1, Cout, 1, N)
    return y.view(-1, n).t().contiguous()


def set_warp_bwd_accumulator(fixed_point: bool = False):
    """`tpspp_warp_bwd_set_accumulator`: the process-wide default of how dL/d input is accumulated in LDS (fp64 atomics;
    True: round 3's 64-bit fixed point, bitwise reproducible but with a per-pass scale).  Measurement scripts only: prefer
    `warp_backward(..., fixed_point=True)`, which is per call and per stream."""
    _lib.check(_lib.lib().tpspp_warp_bwd_set_accumulator(1 if fixed_point else 0), "tpspp_warp_bwd_set_accumulator")


def set_warp_tuning(images_per_group=0, threads_per_group=0, kernel_choice=0, bands=0):
    """`tpspp_warp_set_tuning` (process-wide lab knobs; 0 everywhere = the automatic choice).
    kernel_choice: 0 automatic, 1 gather kernel, 2 LDS-staged kernel, 3 the same without the mirror trick, 4 plane-streaming
    kernel, 5 image-pair kernel, 6 instantiated in-place kernel (tpspp_warp_img.h), 7 a run-time-geometry kernel (the
    in-place kernel of tpspp_warp_geo.h where one workgroup covers the image, else the span-staging kernel), 8 span-staging
    kernel (tpspp_warp_span.h), 9 the in-place kernel of tpspp_warp_geo.h in its banded form as well (2..9: error if not
    applicable to the call's shapes);
    bands: kernel_choice 0 / 2 / 3: workgroups per image (pair) in the LDS-staged kernels, 0..8 (0 = heuristic);
    kernel_choice 7 / 9: bits 0-2 = workgroups per image (0 = heuristic), bit 3 (value 8) = never an image pair per
    workgroup, so 0..15; kernel_choice 8: bits 0-5 = workgroups per image, bit 6 (64) = every workgroup on the
    global-memory path, bit 7 (128) = measured row spans instead of the windows requested at launch, bits 8-15 = LDS budget
    in KB; values above 8 are rejected for every other choice."""
    _lib.check(_lib.lib().tpspp_warp_set_tuning(int(images_per_group), int(threads_per_group),
                                                int(kernel_choice), int(bands)),
               "tpspp_warp_set_tuning")


# ---- recogniser head (NRTR encoder / decoder): channel-major matrices, K-major weights -------------------
def transpose2d(x):
    """(rows, cols) -> (cols, rows) on the device (`tpspp_transpose2d`)."""
    x = _chk("input", x, 2)
    r, c = x.shape
    out = torch.empty((c, r), device=x.device, dtype=torch.float32)
    _call("tpspp_transpose2d", x, x, r, c, out)
    return out


def layernorm_cm(x, gamma, beta, eps=1e-5):
    """LayerNorm over the rows of a channel-major (C, M) matrix (`tpspp_layernorm_cm_fwd`)."""
    x = _chk("input", x, 2)
    C, M = x.shape
    y = torch.empty_like(x)
    _call("tpspp_layernorm_cm_fwd", x, x, _chk("gamma", gamma, 1), _chk("beta", beta, 1), C, M, float(eps), y)
    return y


def fold_layernorm(gamma, beta, w_kmajor, bias=None):
    """LayerNorm affine folded into the following projection (done once per weight):
    -> (w_gamma = diag(gamma) W, w_colsum = column sums of w_gamma, bias_eff = beta^T W (+ bias))."""
    w = w_kmajor.detach().float()
    wg = (gamma.detach().float()[:, None] * w).contiguous()
    be = beta.detach().float() @ w
    if bias is not None:
        be = be + bias.detach().float()
    return wg, wg.sum(0).contiguous(), be.contiguous()


def linear_ln(x, folded, eps=1e-5, act=0, residual=None, token_major=False):
    """Fused LayerNorm -> Linear on a channel-major (K, M) activation (`tpspp_linear_ln_fwd`);
    `folded` = fold_layernorm(gamma, beta, w_kmajor, bias)."""
    wg, colsum, bias_eff = folded
    x, wg = _chk("x", x, 2), _chk("w_gamma", wg, 2)
    K, M = x.shape
    Cout = wg.shape[1]
    out = torch.empty((M, Cout) if token_major else (Cout, M), device=x.device, dtype=torch.float32)
    _call("tpspp_linear_ln_fwd", x, x, K, M, float(eps), wg, _chk("w_colsum", colsum, 1), Cout, bias_eff, int(act),
          residual, int(bool(token_major)), out)
    return out


def attn_enc(qkv, N, T, valid_len=None):
    """Encoder multi-head self-attention on projected (3C, N*T) q/k/v (`tpspp_attn_enc_fwd`) -> (C, N*T)."""
    qkv = _chk("qkv", qkv, 2)
    C = qkv.shape[0] // 3
    out = torch.empty((C, N * T), device=qkv.device, dtype=torch.float32)
    _call("tpspp_attn_enc_fwd", qkv, qkv, N, C, T, valid_len, out)
    return out


def kmajor(weight):
    """PyTorch Linear weight (out, in) -> K-major (in, out) fp32 contiguous device copy."""
    return weight.detach().float().t().contiguous()


def arrange_x3(w_kmajor):
    """K-major (K, Co) fp32 weight -> the step GEMM's operand (`dec_gemm_x3_kernel`, include/tpspp.h): hi = bf16(w),
    lo = bf16(w - hi), Co zero-padded to a multiple of 32, [Co/32][K/16][hi|lo][2 k halves][32 outputs][8 k] bf16."""
    w = w_kmajor.detach().float()
    K, Co = w.shape
    if K % 16:
        raise ValueError("arrange_x3: K must be a multiple of 16")
    Cop = (Co + 31) // 32 * 32
    if Cop != Co:
        w = torch.cat([w, w.new_zeros((K, Cop - Co))], dim=1)
    st = torch.stack(_hi_lo(w))                                        # (s, K, Cop)
    st = st.reshape(2, K // 16, 2, 8, Cop // 32, 32)                   # (s, ks, h, e, ct, r)
    return st.permute(4, 1, 0, 2, 5, 3).contiguous()                   # (ct, ks, s, h, r, e)


def arrange_f32(w_kmajor):
    """K-major (K, Co) fp32 weight -> the exact-fp32 step GEMM's operand (`dec_gemm_f32_kernel`): Co zero-padded to a
    multiple of 32, [Co/32][K/8][2 k halves][32 outputs][4 k] fp32 with k = 8 u + 4 half + e."""
    w = w_kmajor.detach().float()
    K, Co = w.shape
    if K % 8:
        raise ValueError("arrange_f32: K must be a multiple of 8")
    Cop = (Co + 31) // 32 * 32
    if Cop != Co:
        w = torch.cat([w, w.new_zeros((K, Cop - Co))], dim=1)
    return w.reshape(K // 8, 2, 4, Cop // 32, 32).permute(3, 0, 1, 4, 2).contiguous()     # (u, h, e, ct, r) -> (ct, u, h, r, e)


class PtrTable:
    """Host array of device pointers (`const float* const*`) + the tensors it points at (kept alive)."""

    def __init__(self, tensors):
        self.keep = list(tensors)
        self.arr = _ptr_array(self.keep)
        self.ptr = _vp(self.arr)

    def __len__(self):
        return len(self.keep)


def _workspace(holder, nbytes, device):
    """Scratch of the encoder / decoder, cached on the module per (device, stream): two calls on different HIP streams
    must not share a buffer (they could overlap on the GPU)."""
    key = (str(device), _stream(torch.empty(0, device=device)))
    cache = getattr(holder, "_tpspp_ws", None)
    if not isinstance(cache, dict):
        cache = {}
        holder._tpspp_ws = cache
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), device=device, dtype=torch.uint8)
        cache[key] = ws
    return ws


HEAD_BF16 = 1            # TPSPP_HEAD_BF16
HEAD_BF16X3 = 2          # TPSPP_HEAD_BF16X3


def nrtr_encoder(feat, table, n_layers, d_inner, ln_g, ln_b, valid_len=None, holder=None, want_ntc=True, flags=0):
    """`tpspp_nrtr_encoder_fwd`: feat (N, C, H, W) -> (out (N, T, C) | None, out_cm (C, N*T))."""
    feat = _chk("feat", feat, 4)
    N, C, H, W = feat.shape
    T = H * W
    nbytes = _query("tpspp_nrtr_encoder_workspace", N, C, T, d_inner)
    ws = _workspace(holder if holder is not None else table, nbytes, feat.device)
    out_cm = torch.empty((C, N * T), device=feat.device, dtype=torch.float32)
    out = torch.empty((N, T, C), device=feat.device, dtype=torch.float32) if want_ntc else None
    _call("tpspp_nrtr_encoder_fwd", feat, feat, N, C, T, d_inner, n_layers, table.ptr, ln_g, ln_b, valid_len, ws,
          ws.numel(), out_cm, out, int(flags))
    return out, out_cm


def nrtr_decoder(enc_cm, N, T, table, n_layers, d_inner, emb, pos_table, cls_folded, max_seq_len,
                 start_idx, padding_idx, valid_len=None, forced_tokens=None, holder=None, flags=0):
    """`tpspp_nrtr_decoder_fwd` -> (out (N, L, num_out), tokens (N, L+1) int32, status (1,) int32).
    `status` is the device word the decode leaves behind itself: 0 = every step completed, 1 = a cluster barrier of the
    persistent step kernel timed out (the affected images' scores are NaN from that step on; include/tpspp.h).  Nothing
    here synchronises; whoever copies the scores / tokens to the host reads it in the same copy (`check_decoder_status`,
    `attn_tensor2idx`)."""
    enc_cm = _chk("enc_cm", enc_cm, 2)
    C = enc_cm.shape[0]
    if enc_cm.shape[1] != N * T:
        raise ValueError("nrtr_decoder: enc_cm must be (C, N*T)")
    w_cls, cls_colsum, b_cls = cls_folded              # fold_layernorm(final layer_norm, classifier)
    num_out = w_cls.shape[1]
    nbytes = _query("tpspp_nrtr_decoder_workspace", N, C, T, d_inner, n_layers, max_seq_len, num_out)
    ws = _workspace(holder if holder is not None else table, nbytes, enc_cm.device)
    out = torch.empty((N, max_seq_len, num_out), device=enc_cm.device, dtype=torch.float32)
    # tokens and the status word in one buffer: one device->host copy fetches both
    tok_status = torch.empty((N * (max_seq_len + 1) + 1,), device=enc_cm.device, dtype=torch.int32)
    tokens = tok_status[:-1].view(N, max_seq_len + 1)
    status = tok_status[-1:]
    if forced_tokens is not None:
        if forced_tokens.dtype != torch.int32 or tuple(forced_tokens.shape) != (N, max_seq_len) or \
                not forced_tokens.is_contiguous() or forced_tokens.device != enc_cm.device:
            raise ValueError("nrtr_decoder: forced_tokens must be a contiguous (N, max_seq_len) int32 device tensor")
    _call("tpspp_nrtr_decoder_fwd", enc_cm, enc_cm, N, C, T, d_inner, n_layers, table.ptr, len(table), emb, pos_table,
          pos_table.shape[0], w_cls, cls_colsum, b_cls, num_out, max_seq_len, int(start_idx), int(padding_idx), valid_len,
          forced_tokens, ws, ws.numel(), out, tokens, status, int(flags))
    return out, tokens, status


DecoderRoute = collections.namedtuple("DecoderRoute", "pipeline kv gemm cross persist")


def nrtr_decoder_route(C, T, table, n_layers, d_inner, num_out, flags=0):
    """`tpspp_nrtr_decoder_route`: what `nrtr_decoder` with these sizes, `flags` and this `PtrTable` dispatches to, as
    `DecoderRoute(pipeline "plain" | "arranged" | "persistent", kv "bf16" | "fp32", gemm "fp32" | "x3", cross 2 | 1 heads
    per wavefront, persist = the persistent kernel's instantiation 0..11 or None)`.  A host-side query: of the table only
    which entries are None is read, nothing is launched.  "persistent" means eligible (include/tpspp.h)."""
    code = _lib.lib().tpspp_nrtr_decoder_route(int(C), int(T), int(d_inner), int(n_layers), table.ptr, len(table),
                                               int(num_out), int(flags))
    if code < 0:
        _lib.check(code, "tpspp_nrtr_decoder_route")
    return DecoderRoute(("plain", "arranged", "persistent")[code & 3], "bf16" if code & 4 else "fp32",
                        "fp32" if code & 8 else "x3", 2 if code & 16 else 1, ((code >> 8) & 15) - 1 if code >> 8 else None)


DECODER_TIMEOUT_MESSAGE = (
    "tpspp_nrtr_decoder_fwd: a cluster barrier of the persistent decoder kernel timed out (status 1): the scores of the "
    "affected images are NaN.  The kernel needs its workgroups co-resident; this happens only when another PROCESS runs a "
    "persistent decode on the same GPU or the device stayed occupied for longer than TPSPP_HEAD_TIMEOUT_MS "
    "(include/tpspp.h).  TPSPP_HEAD_NO_PERSIST=1 selects the launch-per-phase pipeline.")


def check_decoder_status(status):
    """Synchronising check of a decode's status word (one 4-byte device->host copy): raises `TpsppError` on a timeout."""
    if status is not None and int(status.cpu()[0]) != 0:
        raise _lib.TpsppError(DECODER_TIMEOUT_MESSAGE)


def attn_tensor2idx(scores, end_idx, padding_idx, status=None):
    """`tpspp_attn_tensor2idx_fwd` + ONE device->host copy: (idx (N, L) int32 numpy with -1 where the reference's scan drops
    the position, val (N, L) float32 numpy).  `status`: a decode's status word, fetched in the same copy; non-zero raises."""
    scores = _chk("scores", scores, 3)
    N, L, C = scores.shape
    # [idx (N*L) | val (N*L) as raw bits | status]: one int32 buffer, one copy
    buf = torch.empty((2 * N * L + 1,), device=scores.device, dtype=torch.int32)
    _call("tpspp_attn_tensor2idx_fwd", scores, scores, N, L, C, int(end_idx), int(padding_idx), buf.data_ptr(),
          buf.data_ptr() + 4 * N * L)
    if status is not None and status.device == scores.device:
        buf[-1:].copy_(status)
    else:
        buf[-1:].zero_()
    host = buf.cpu().numpy()
    if host[-1] != 0:
        raise _lib.TpsppError(DECODER_TIMEOUT_MESSAGE)
    return host[:N * L].reshape(N, L), host[N * L:2 * N * L].view("float32").reshape(N, L)


RESIZE_CV2, RESIZE_PILLOW = 0, 1


def resize_normalize(packed, offsets, src_h, src_w, resize_w, lut, pad_value, N, C, H, W, interpolation=RESIZE_CV2):
    """`tpspp_resize_normalize_fwd`: packed uint8 HWC images -> (N, C, H, W) fp32 (ocr_transforms.py:67-156).
    `interpolation`: RESIZE_CV2 (OpenCV's INTER_LINEAR arithmetic, unpinned) or RESIZE_PILLOW (Pillow's BILINEAR, pinned)."""
    if interpolation not in (RESIZE_CV2, RESIZE_PILLOW):
        raise ValueError("resize_normalize: interpolation must be RESIZE_CV2 or RESIZE_PILLOW")
    for name, t, dt in (("packed", packed, torch.uint8), ("offsets", offsets, torch.int64), ("src_h", src_h, torch.int32),
                        ("src_w", src_w, torch.int32), ("resize_w", resize_w, torch.int32), ("lut", lut, torch.float32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.TpsppError(f"resize_normalize: {name} must be a GPU tensor (no CPU fallback)")
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"resize_normalize: {name} must be a contiguous {dt} tensor")
    if offsets.numel() != N or src_h.numel() != N or src_w.numel() != N or resize_w.numel() != N or \
            tuple(lut.shape) != (C, 256):
        raise ValueError("resize_normalize: per-image arrays need N entries, lut must be (C, 256)")
    out = torch.empty((N, C, H, W), device=packed.device, dtype=torch.float32)
    _call("tpspp_resize_normalize_fwd", packed, packed, offsets, src_h, src_w, resize_w, lut, int(pad_value), int(N),
          int(C), int(H), int(W), out, int(interpolation))
    return out


# op codes of include/tpspp_augment.h
AUG_END, AUG_AFFINE_NEAREST_PIL, AUG_PERSPECTIVE_BILINEAR_PIL, AUG_AFFINE_NEAREST_CV2 = 0, 1, 2, 3
AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE = 4, 5, 6, 7
AUG_MAX_OPS, AUG_OP_PARAMS = 8, 8


def augment_normalize(packed, offsets, src_h, src_w, resize_w, lut, pad_value, N, C, H, W, op_codes, op_params,
                      interpolation=RESIZE_CV2, bgr=True):
    """`tpspp_augment_normalize_fwd`: `resize_normalize` with a list of augmentation ops per image between the resize and
    the normalisation (crnn_pp_pipeline.py:2-84; include/tpspp_augment.h has the arithmetic of each code).
    `op_codes` (N, max_ops) int32 and `op_params` (N, max_ops, 8) float64 on the GPU, max_ops 1..8, code 0 ends a list;
    `bgr`: channel 0 is blue, as mmcv.imread loads.  Codes 1, 2, 4..7 are Pillow's arithmetic (pinned), code 3 OpenCV's
    (unpinned).  With every list empty the result has the bits of `resize_normalize`."""
    if interpolation not in (RESIZE_CV2, RESIZE_PILLOW):
        raise ValueError("augment_normalize: interpolation must be RESIZE_CV2 or RESIZE_PILLOW")
    for name, t, dt in (("packed", packed, torch.uint8), ("offsets", offsets, torch.int64), ("src_h", src_h, torch.int32),
                        ("src_w", src_w, torch.int32), ("resize_w", resize_w, torch.int32), ("lut", lut, torch.float32),
                        ("op_codes", op_codes, torch.int32), ("op_params", op_params, torch.float64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.TpsppError(f"augment_normalize: {name} must be a GPU tensor (no CPU fallback)")
        if t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"augment_normalize: {name} must be a contiguous {dt} tensor")
    if offsets.numel() != N or src_h.numel() != N or src_w.numel() != N or resize_w.numel() != N or \
            tuple(lut.shape) != (C, 256):
        raise ValueError("augment_normalize: per-image arrays need N entries, lut must be (C, 256)")
    if op_codes.dim() != 2 or op_codes.shape[0] != N or not 1 <= op_codes.shape[1] <= AUG_MAX_OPS or \
            tuple(op_params.shape) != (N, op_codes.shape[1], AUG_OP_PARAMS):
        raise ValueError(f"augment_normalize: op_codes must be (N, 1..{AUG_MAX_OPS}), op_params (N, max_ops, {AUG_OP_PARAMS})")
    out = torch.empty((N, C, H, W), device=packed.device, dtype=torch.float32)
    _call("tpspp_augment_normalize_fwd", packed, packed, offsets, src_h, src_w, resize_w, lut, int(pad_value), int(N),
          int(C), int(H), int(W), out, int(interpolation), op_codes, op_params, int(op_codes.shape[1]), int(bool(bgr)))
    return out


# ---- backward of the fused warp ------------------------------------------------
_WarpBwdCall = collections.namedtuple("_WarpBwdCall", "args in0 in1 ctrl inv_delta_C score N F Ho Wo flags")


def _warp_bwd_marshal(who, gpu, g_out0, in0, grid, ctrl, inv_delta_C, P_hat, out_hw, P_xy, score, in1, g_out1, P_hat_t,
                      fixed_point, two_kernels):
    """The checks and the argument order of one `tpspp_warp_bwd` call, shared by `warp_backward` (gpu=True) and
    `warp_backward_route` (gpu=False: CPU tensors pass), so that the query sees exactly the launch's flags, sizes and
    (contiguous) tensors.  `.args(T, g_in0, g_in1, g_ctrl, g_score, ws, ws_floats)` completes the argument tuple."""
    io_dtype = in0.dtype if isinstance(in0, torch.Tensor) else None
    for nm, t in (("g_out0", g_out0), ("in1", in1), ("g_out1", g_out1)):
        if isinstance(t, torch.Tensor) and t.dtype != io_dtype:
            raise TypeError(f"{who}: in0 / in1 / g_out0 / g_out1 must share their dtype (all float32 or all "
                            f"bfloat16); in0 is {io_dtype}, {nm} is {t.dtype}")
    io = (torch.bfloat16,) if io_dtype == torch.bfloat16 else _F32
    chk = lambda name, t, ndim, dtypes=_F32: _chk(name, t, ndim, dtypes, gpu=gpu)      # noqa: E731
    g_out0, in0 = chk("g_out0", g_out0, 4, io), chk("in0", in0, 4, io)
    grid, ctrl = chk("grid", grid, 3), chk("ctrl", ctrl, 3)
    inv_delta_C, P_hat = chk("inv_delta_C", inv_delta_C, 2), chk("P_hat", P_hat, 2)
    N, C0, H0, W0 = in0.shape
    F = int(ctrl.shape[1])
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    n = Ho * Wo
    if tuple(g_out0.shape) != (N, C0, Ho, Wo) or tuple(grid.shape) != (N, n, 2):
        raise ValueError(f"{who}: g_out0 / grid shape")
    flags = (BWD_FIXED_POINT if fixed_point else 0) | (BWD_TWO_KERNELS if two_kernels else 0) | \
        (IO_BF16 if io_dtype == torch.bfloat16 else 0)
    if score is not None:
        score, transposed = _chk_score(who, score, N, n, F, gpu=gpu)
        flags |= transposed
    if P_xy is not None:
        P_xy = chk("P_xy", P_xy, 2)
    if P_hat_t is not None:
        P_hat_t = chk("P_hat_t", P_hat_t, 2)
    C1 = H1 = W1 = 0
    if in1 is not None:
        in1, g_out1 = chk("in1", in1, 4, io), chk("g_out1", g_out1, 4, io)
        _, C1, H1, W1 = in1.shape
        if tuple(g_out1.shape) != (N, C1, Ho, Wo):
            raise ValueError(f"{who}: g_out1 shape")

    def args(T, g_in0, g_in1, g_ctrl, g_score, ws, ws_floats):
        return (g_out0, in0, C0, H0, W0, g_out1, in1, C1, H1, W1, grid, T, inv_delta_C, P_hat, P_hat.shape[1], P_xy, score,
                P_hat_t, flags, N, F, Ho, Wo, g_in0, g_in1, g_ctrl, g_score, ws, ws_floats)
    return _WarpBwdCall(args, in0, in1, ctrl, inv_delta_C, score, N, F, Ho, Wo, flags)


def warp_backward(g_out0, in0, grid, ctrl, inv_delta_C, P_hat, out_hw, P_xy=None, score=None, in1=None,
                  g_out1=None, P_hat_t=None, need_in0=True, need_in1=True, need_score=True, fixed_point=False,
                  two_kernels=False):
    """`tpspp_warp_bwd`: (g_in0 | None, g_in1 | None, g_ctrl, g_score | None) for the call
    `warp(in0, ctrl, inv_delta_C, P_hat, out_hw, P_xy, score, in1)`; `grid` is that call's grid output.
    `fixed_point=True` (TPSPP_BWD_FIXED_POINT, this call only): dL/d input accumulated in 64-bit fixed point -- bitwise
    reproducible from run to run; the default fp64 LDS atomics keep every term's bits but their sum depends on arrival
    order, so two runs may differ by one fp32 ulp at rounding ties (include/tpspp.h).  `two_kernels=True`
    (TPSPP_BWD_TWO_KERNELS, this call only): the sampling + parameter kernels even where the classic rectifier's one-launch
    form would run.
    The images and the output gradients are all float32 or all bfloat16 (TPSPP_IO_BF16; mixed dtypes raise TypeError before
    anything else is looked at): g_in0 / g_in1 come back in the images' dtype, g_ctrl / g_score, the grid, the tables and
    all accumulation stay fp32.  bfloat16 is served where dL/d input is finished in LDS (include/tpspp.h); any other
    shape raises with the library's message."""
    m = _warp_bwd_marshal("warp_backward", True, g_out0, in0, grid, ctrl, inv_delta_C, P_hat, out_hw, P_xy, score, in1, g_out1,
                          P_hat_t, fixed_point, two_kernels)
    g_score = torch.empty_like(m.score) if (m.score is not None and need_score) else None
    T = solve_T(m.inv_delta_C, m.ctrl) if m.score is not None else None      # (only dL/d score reads T)
    g_in0 = torch.empty_like(m.in0) if need_in0 else None
    g_in1 = torch.empty_like(m.in1) if (m.in1 is not None and need_in1) else None
    g_ctrl = torch.empty((m.N, m.F, 2), device=m.in0.device, dtype=torch.float32)
    g_grid = torch.empty((_query("tpspp_warp_bwd_workspace_floats", m.N, m.Ho, m.Wo),), device=m.in0.device, dtype=torch.float32)
    _call("tpspp_warp_bwd", m.in0, *m.args(T, g_in0, g_in1, g_ctrl, g_score, g_grid, g_grid.numel()))
    if g_score is not None and (m.flags & SCORE_TRANSPOSED):
        g_score = g_score.transpose(1, 2)                  # back to the logical (N, n, F) view
    return g_in0, g_in1, g_ctrl, g_score


class WarpBwdRoute(collections.namedtuple("WarpBwdRoute", (
        "family", "ppt", "nt", "f64", "bf16", "G", "cpt0", "cpt1", "chunks0", "chunks1", "slots", "params", "kmax", "table",
        "transposed", "score", "gscore", "S"))):
    """What `tpspp_warp_bwd_route` reports (include/tpspp.h), with the family as a word: "classic", "classic_bf16", "lds2",
    "lds", "atomics", or "none" for an empty batch.  `str()` reads `lds2 ppt4 nt256 f64 G3 | params k36 tpspp T score_t
    gscore S4`; `params_key` is the parameter kernel's instantiation (KMAX, TABLE, TRANSPOSED, SCORE, GSCORE) or None."""
    __slots__ = ()
    FAMILIES = ("classic", "classic_bf16", "lds2", "lds", "atomics")

    @property
    def params_key(self):
        return (self.kmax, self.table, self.transposed, self.score, self.gscore) if self.params else None

    def __str__(self):
        io = " bf16" if self.bf16 else ""
        acc = "f64" if self.f64 else "fix"
        if self.family == "lds2":
            s = f"lds2 ppt{self.ppt} nt{self.nt} {acc}{io} G{self.G}"
        elif self.family == "lds":
            s = f"lds cpt{self.cpt0},{self.cpt1} G{self.G}"
        elif self.family == "atomics":
            s = f"atomics chunks{self.chunks0}+{self.chunks1}"
        else:
            s = self.family
        if self.params:
            s += (f" | params k{self.kmax} {'tpspp' if self.table else 'classic'} {'T' if self.transposed else 'N'} "
                  f"{('noscore', 'score', 'score_t')[self.score]}{' gscore' if self.gscore else ''} S{self.S}")
        return s


def warp_backward_route(g_out0, in0, grid, ctrl, inv_delta_C, P_hat, out_hw, P_xy=None, score=None, in1=None,
                        g_out1=None, P_hat_t=None, need_in0=True, need_in1=True, need_score=True, fixed_point=False,
                        two_kernels=False, g_in0=None, g_in1=None):
    """The kernels `warp_backward` would launch for these arguments (`tpspp_warp_bwd_route`), as a `WarpBwdRoute`.  A
    host-side query that launches nothing: the tensors are read for their shapes, dtypes and addresses only (the library
    looks at a pointer's alignment, never behind it), so CPU tensors will do.  `g_in0` / `g_in1`: tensors that stand for the
    buffers dL/d input would be written to, for callers of the entry point that bring their own -- `warp_backward`
    allocates them, 16-byte aligned, which is what is assumed without them.  Whatever `tpspp_warp_bwd` refuses raises the
    same `TpsppError` here."""
    m = _warp_bwd_marshal("warp_backward_route", False, g_out0, in0, grid, ctrl, inv_delta_C, P_hat, out_hw, P_xy, score, in1,
                          g_out1, P_hat_t, fixed_point, two_kernels)
    aligned = 64                                            # stands for a buffer warp_backward allocates itself
    ws = _query("tpspp_warp_bwd_workspace_floats", m.N, m.Ho, m.Wo)
    route = _int_array([0] * 18)
    args = m.args(aligned if m.score is not None else None,
                  (g_in0 if g_in0 is not None else aligned) if need_in0 else None,
                  (g_in1 if g_in1 is not None else aligned) if (m.in1 is not None and need_in1) else None,
                  aligned, aligned if (m.score is not None and need_score) else None, aligned, ws)
    rc = _lib.lib().tpspp_warp_bwd_route(*_marshal(args), _vp(route), len(route))
    _lib.check(rc, "tpspp_warp_bwd_route")
    v = list(route)
    return WarpBwdRoute("none" if v[0] < 0 else WarpBwdRoute.FAMILIES[v[0]], *v[1:])


class _WarpFunction(torch.autograd.Function):
    """Differentiable `warp`: HIP forward (`tpspp_warp_fwd`) and HIP backward (`tpspp_warp_bwd`).  The tables
    (inv_delta_C, P_hat, P_xy) are constants of the module and get no gradient.  bfloat16 in0 (and in1): the bf16 forward
    (its grid output is fp32, with the bits the fp32 forward gives for the same control points) and the bf16 backward:
    bf16 outputs, bf16 gradients to in0 / in1, fp32 gradients to ctrl / score."""

    @staticmethod
    def forward(ctx, in0, ctrl, score, in1, inv_delta_C, P_hat, P_xy, P_hat_t, out_hw, table_flags):
        if isinstance(in0, torch.Tensor) and in0.dtype == torch.bfloat16 and in0.is_cuda:
            # a geometry the bf16 backward refuses raises here, with the library's message, not in the middle of .backward():
            # tpspp_warp_bwd checks it before its N == 0 return (no launch; the pointers only stand in for their alignment)
            H1, W1 = (int(in1.shape[2]), int(in1.shape[3])) if in1 is not None else (0, 0)
            a, b = in0, in1
            _call("tpspp_warp_bwd", a, a, a, 1, int(in0.shape[2]), int(in0.shape[3]), b, b, 1 if in1 is not None else 0,
                  H1, W1, a, a, a, a, 64, None, None, None, IO_BF16, 0, 1, int(out_hw[0]), int(out_hw[1]), a, b, a, None, a, 0)
        out0, out1, grid, _ = warp(in0, ctrl, inv_delta_C, P_hat, out_hw, P_xy=P_xy, score=score, in1=in1,
                                   want_grid=True, P_hat_t=P_hat_t, table_flags=table_flags)
        ctx.out_hw = out_hw
        ctx.has = (score is not None, in1 is not None)
        ctx.save_for_backward(in0, ctrl, score, in1, inv_delta_C, P_hat, P_xy, P_hat_t, grid)
        if out1 is None:
            return out0
        return out0, out1

    @staticmethod
    def backward(ctx, *g):
        in0, ctrl, score, in1, inv_delta_C, P_hat, P_xy, P_hat_t, grid = ctx.saved_tensors
        g0 = g[0]
        g1 = g[1] if len(g) > 1 else None
        # (a missing or differently typed output gradient takes the images' dtype: bf16 images give and take bf16 gradients)
        if g0 is None:
            g0 = torch.zeros((in0.shape[0], in0.shape[1]) + tuple(ctx.out_hw), device=in0.device, dtype=in0.dtype)
        if in1 is not None and g1 is None:
            g1 = torch.zeros((in1.shape[0], in1.shape[1]) + tuple(ctx.out_hw), device=in0.device, dtype=in0.dtype)
        need = ctx.needs_input_grad
        g_in0, g_in1, g_ctrl, g_score = warp_backward(
            g0.to(in0.dtype), in0, grid, ctrl, inv_delta_C, P_hat, ctx.out_hw, P_xy=P_xy, score=score, in1=in1,
            g_out1=None if g1 is None else g1.to(in0.dtype), P_hat_t=P_hat_t, need_in0=need[0],
            need_in1=need[3], need_score=need[2])
        return (g_in0, g_ctrl if need[1] else None, g_score, g_in1, None, None, None, None, None, None)


def warp_autograd(in0, ctrl, inv_delta_C, P_hat, out_hw, P_xy=None, score=None, in1=None, P_hat_t=None,
                  table_flags=0):
    """`warp` inside an autograd graph: returns out0 or (out0, out1); gradients flow to in0, ctrl, score, in1.
    bfloat16 in0 / in1 stay bfloat16 in both directions (no fp32 copy of the images, the outputs or their gradients)."""
    return _WarpFunction.apply(in0, ctrl, score, in1, inv_delta_C, P_hat, P_xy, P_hat_t,
                               (int(out_hw[0]), int(out_hw[1])), int(table_flags))


# ---- training graph of the regressor's other layers (train backend "hip_all", tpspp_regressor_bwd.hip) -----------------
# Every Linear layer, LayerNorm, gate, softmax, activation and CBAM of the control-point regressor forward and backward on
# HIP kernels.  The kernels read PyTorch's own parameter layouts (an nn.Linear weight (O, K) is the B operand of
# `tpspp_mm_f32` as it is), so nothing is prepared from the parameters and nothing can go stale.  A token operand is
# described as (nb, Mi, sb, si, sk): row r = (q, i) with q < nb, i < Mi, feature k at q*sb + i*si + k*sk -- dense rows
# are (1, M, 0, K, 1), the tokens of an NCHW map (b c h w -> b (h w) c) are (N, H*W, C*H*W, 1, H*W).

def _i64(*v):
    return _int_array(v, ctypes.c_longlong)


def _dense(M, K):
    return (1, M, 0, K, 1)


def _nchw_tokens(t):
    n, c = t.shape[0], t.shape[1]
    hw = t.numel() // max(1, n * c)
    return (n, hw, c * hw, 1, hw)


def mm(A, a_strides, B, b_strides, C, c_strides, batch, M, N, K, bias=None, R=None, epi=0, alpha=1.0, k_total=0):
    """`tpspp_mm_f32`: C[b][i][j] = epi(alpha * sum_k A[b][i][k] B[b][j][k] + bias[j]) (+ R[b][i][j]); strides in
    elements, (batch, row, k) for A / B and (batch, row, column) for C and R.  epi: 0 none, 1 ReLU, 2 GELU, 3 tanh."""
    sa, sb, sc = _i64(*a_strides), _i64(*b_strides), _i64(*c_strides)
    _call("tpspp_mm_f32", C, batch, M, N, K, A, _vp(sa), B, _vp(sb), C, _vp(sc), bias, R, epi, float(alpha), k_total)
    return C


def linear_fwd(x, desc, weight, bias=None, epi=0, R=None):
    """y (rows, O) dense = epi(x W^T + b) (+ R) for the token operand x described by `desc`."""
    nb, Mi, sb, si, sk = desc
    O, K = weight.shape
    y = torch.empty((nb * Mi, O), device=weight.device, dtype=torch.float32)
    mm(x, (sb, si, sk), weight, (0, K, 1), y, (Mi * O, O, 1), nb, Mi, O, K, bias=bias, R=R, epi=epi)
    return y


def linear_bwd_data(dy, weight, out=None, desc=None):
    """out (token operand `desc`) = dy (rows, O) W; dy dense.  Without `out`: a fresh (rows, K) tensor, `desc` then being
    `_dense(rows, K)` or left out (the tokens of an NCHW map are written into the caller's `out`)."""
    O, K = weight.shape
    if out is None:
        rows = dy.numel() // O
        if desc not in (None, _dense(rows, K)):
            raise ValueError(f"linear_bwd_data: the token operand {desc} is not _dense({rows}, {K}): pass `out`")
        out, desc = torch.empty((rows, K), device=dy.device, dtype=torch.float32), _dense(rows, K)
    nb, Mi, sb, si, sk = desc
    mm(dy, (Mi * O, O, 1), weight, (0, 1, K), out, (sb, si, sk), nb, Mi, K, O)
    return out


def linear_bwd_weight_workspace_floats(M, O, K):
    return _query("tpspp_linear_bwd_weight_workspace_floats", M, O, K)


def linear_bwd_weight(dy, x, desc, O, K, want_weight=True, want_bias=True, x_gelu=False):
    """(dW (O, K) | None, db (O) | None) of a Linear layer from dy (rows, O) dense and its input x (`desc`), or GELU(x)
    with x_gelu: `tpspp_linear_bwd_weight`, fixed split-K, bitwise reproducible."""
    if not (want_weight or want_bias):
        return None, None
    nb, Mi, sb, si, sk = desc
    M = nb * Mi
    dev = dy.device
    dw = torch.empty((O, K), device=dev, dtype=torch.float32) if want_weight else None
    db = torch.empty((O,), device=dev, dtype=torch.float32) if want_bias else None
    ws, n = _ws_n(linear_bwd_weight_workspace_floats(M, O, K), dev)
    lay = _i64(Mi, sb, si, sk)
    _call("tpspp_linear_bwd_weight", dy, dy, x, _vp(lay), 2 if x_gelu else 0, M, O, K, dw, db, ws, n)
    return dw, db


ACT_RELU, ACT_GELU, ACT_TANH = 0, 1, 2


def act_bwd(op, g, t, scale=1.0, out=None):
    """`tpspp_act_bwd`: g * f'(.) for ReLU (t = output), GELU (t = input) or tanh(scale * u) (t = output, d/du)."""
    out = torch.empty_like(g) if out is None else out
    _call("tpspp_act_bwd", g, op, g.numel(), g, t, float(scale), out)
    return out


def plane_ln_fwd(x, weight, bias, eps):
    """nn.LayerNorm over the last weight.numel() elements: (y, mean, rstd)."""
    P = weight.numel()
    rows = x.numel() // P
    y = torch.empty_like(x)
    mean = torch.empty((rows,), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    _call("tpspp_plane_ln_fwd", x, x, weight, bias, rows, P, float(eps), y, mean, rstd)
    return y, mean, rstd


def plane_ln_bwd_workspace_floats(rows, P):
    return _query("tpspp_plane_ln_bwd_workspace_floats", rows, P)


def plane_ln_bwd(dy, x, weight, mean, rstd, dx=None, accumulate=False, want_params=True):
    """Backward of `plane_ln_fwd`: writes (or adds to) dx when given; returns (dweight, dbias) | (None, None)."""
    P = weight.numel()
    rows = x.numel() // P
    dev = x.device
    dw = db = ws = None
    n = 0
    if want_params:
        dw = torch.empty((P,), device=dev, dtype=torch.float32)
        db = torch.empty((P,), device=dev, dtype=torch.float32)
        ws, n = _ws_n(plane_ln_bwd_workspace_floats(rows, P), dev)
    if dx is None and not want_params:
        return None, None
    _call("tpspp_plane_ln_bwd", x, dy, x, weight, mean, rstd, rows, P, dx, int(bool(accumulate)), dw, db, ws, n)
    return (dw.view(weight.shape), db.view(weight.shape)) if want_params else (None, None)


def _ln_bwd(dy, x, weight, mean, rstd, need, into=None):
    """`plane_ln_bwd` as an autograd backward wants it, need = (x, weight, bias) -> (dx, dweight, dbias), None where not
    needed and no launch when none is.  dx is a fresh tensor, or `into` with the gradient added to it in place."""
    dx = (torch.empty_like(x) if into is None else into) if need[0] else None
    dw, db = plane_ln_bwd(dy, x, weight, mean, rstd, dx=dx, accumulate=into is not None, want_params=need[1] or need[2])
    return dx, dw if need[1] else None, db if need[2] else None


def _mlp_fwd(x, nw, nb, eps, w1, b1, w2, b2, residual=False):
    """fc2(GELU(fc1(LayerNorm(x)))) (+ x with residual) over rows of w1.shape[1] elements: (y shaped like x, mean, rstd)."""
    hid, K = w1.shape
    rows = x.numel() // K
    xn, mean, rstd = plane_ln_fwd(x, nw, nb, eps)
    g = linear_fwd(xn, _dense(rows, K), w1, b1, epi=2)
    return linear_fwd(g, _dense(rows, hid), w2, b2, R=x if residual else None).view(x.shape), mean, rstd


def _mlp_bwd(gy, x, nw, nb, mean, rstd, eps, w1, b1, w2, need, residual=False):
    """Backward of `_mlp_fwd` from gy (contiguous, shaped like x), need = (x, nw, nb, w1, b1, w2, b2) -> the seven
    gradients in that order.  The LayerNorm output and fc1's pre-activation u are recomputed.  With residual, dx is a copy
    of gy that the LayerNorm backward adds to in place."""
    hid, K = w1.shape
    rows = x.numel() // K
    xn, _, _ = plane_ln_fwd(x, nw, nb, eps)
    u = linear_fwd(xn, _dense(rows, K), w1, b1)
    # fc2's input GELU(u) is formed from u as the weight gradient stages it
    dw2, db2 = linear_bwd_weight(gy, u, _dense(rows, hid), K, hid, need[5], need[6], x_gelu=True)
    du = linear_bwd_data(gy, w2)
    act_bwd(ACT_GELU, du, u, out=du)
    del u
    dw1, db1 = linear_bwd_weight(du, xn, _dense(rows, K), hid, K, need[3], need[4])
    del xn
    dx = dnw = dnb = None
    if any(need[:3]):
        dxn = linear_bwd_data(du, w1)
        del du
        into = torch.empty_like(gy).copy_(gy) if residual else None
        dx, dnw, dnb = _ln_bwd(dxn, x, nw, mean, rstd, need[:3], into=into)
    return dx, dnw, dnb, dw1, db1, dw2, db2


def _two_linear_bwd(dy, h, w2, x, desc, w1, need, act=None):
    """Backward of W2 f(W1 x + b1) + b2 from dy (rows, O) dense: h (rows, H) is the saved f(W1 x + b1), f the identity or
    the activation `act` (ACT_RELU: one whose derivative `act_bwd` takes from its output), x the token operand `desc`.
    need = (x, w1, b1, w2, b2) -> the five gradients in that order, dx shaped like x."""
    H, K = w1.shape
    rows = desc[0] * desc[1]
    dw2, db2 = linear_bwd_weight(dy, h, _dense(rows, H), w2.shape[0], H, need[3], need[4])
    dh = linear_bwd_data(dy, w2)
    if act is not None:
        act_bwd(act, dh, h, out=dh)
    dw1, db1 = linear_bwd_weight(dh, x, desc, H, K, need[1], need[2])
    dx = linear_bwd_data(dh, w1, torch.empty_like(x), desc) if need[0] else None
    return dx, dw1, db1, dw2, db2


class _DgabFunction(torch.autograd.Function):
    """DGAB (`DGAB.py:58-77`) forward and backward on HIP kernels.  Saves x, y, the gate vectors w / h, x1 = x + attn and
    both LayerNorms' statistics; xn, A, the norm2 output and fc1's pre-activation are recomputed in the backward (GELU of
    it inside fc2's weight-gradient staging)."""

    @staticmethod
    def forward(ctx, x, y, ln1w, ln1b, mww, mhw, pw, pb, ln2w, ln2b, f1w, f1b, f2w, f2b, eps1, eps2):
        N, C, H, W = x.shape
        T = y.shape[2]
        xn, m1, r1 = plane_ln_fwd(x, ln1w, ln1b, eps1)
        catw = torch.empty((N * C, W + T), device=x.device, dtype=torch.float32)
        cath = torch.empty((N * C, H + T), device=x.device, dtype=torch.float32)
        _call("tpspp_dgab_pool_fwd", x, xn, y, N, C, H, W, T, catw, cath)
        wv = linear_fwd(catw, _dense(N * C, W + T), mww)
        hv = linear_fwd(cath, _dense(N * C, H + T), mhw)
        A = torch.empty_like(x)
        _call("tpspp_dgab_gate_fwd", x, xn, wv, hv, N, C, H, W, A)
        x1 = linear_fwd(A, _dense(N * C * H, W), pw, pb, R=x).view(N, C, H, W)
        del A, xn, catw, cath
        out, m2, r2 = _mlp_fwd(x1, ln2w, ln2b, eps2, f1w, f1b, f2w, f2b, residual=True)
        ctx.eps = (eps1, eps2)
        ctx.save_for_backward(x, y, wv, hv, x1, m1, r1, m2, r2, ln1w, ln1b, mww, mhw, pw, pb, ln2w, ln2b, f1w, f1b, f2w)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        (x, y, wv, hv, x1, m1, r1, m2, r2, ln1w, ln1b, mww, mhw, pw, pb, ln2w, ln2b, f1w, f1b, f2w) = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:14]):
            return (None,) * 16
        N, C, H, W = x.shape
        T = y.shape[2]
        rows = N * C * H
        eps1, eps2 = ctx.eps
        # ---- mlp (fc1 - GELU - fc2 along W) and norm2; x2n and u recomputed.  dx1 starts as a copy of gout (the residual)
        # and the kernels below accumulate into it in place
        dx1, *d_mlp = _mlp_bwd(gout.float().contiguous(), x1, ln2w, ln2b, m2, r2, eps2, f1w, f1b, f2w, (True, *need[8:14]),
                               residual=True)
        # ---- attention: proj, gate, mlp_w / mlp_h, the pooled means; xn and A recomputed
        xn, _, _ = plane_ln_fwd(x, ln1w, ln1b, eps1)
        dw_p = db_p = None
        if need[6] or need[7]:
            A = torch.empty_like(x)
            _call("tpspp_dgab_gate_fwd", x, xn, wv, hv, N, C, H, W, A)
            dw_p, db_p = linear_bwd_weight(dx1, A, _dense(rows, W), W, W, need[6], need[7])
            del A
        dA = linear_bwd_data(dx1, pw)
        dxn = torch.empty_like(x)
        dwv, dhv = torch.empty_like(wv), torch.empty_like(hv)
        _call("tpspp_dgab_gate_bwd", x, dA, xn, wv, hv, N, C, H, W, dxn, dwv, dhv)
        del dA
        dw_mw = dw_mh = None
        if need[4] or need[5]:
            catw = torch.empty((N * C, W + T), device=x.device, dtype=torch.float32)
            cath = torch.empty((N * C, H + T), device=x.device, dtype=torch.float32)
            _call("tpspp_dgab_pool_fwd", x, xn, y, N, C, H, W, T, catw, cath)
            dw_mw, _ = linear_bwd_weight(dwv, catw, _dense(N * C, W + T), W + 1, W + T, need[4], False)
            dw_mh, _ = linear_bwd_weight(dhv, cath, _dense(N * C, H + T), H + 1, H + T, need[5], False)
            del catw, cath
        dcatw = linear_bwd_data(dwv, mww)
        dcath = linear_bwd_data(dhv, mhw)
        dy = torch.empty_like(y) if need[1] else None
        _call("tpspp_dgab_pool_bwd", x, dcatw, dcath, N, C, H, W, T, dxn, dy)
        del dcatw, dcath
        dx, dw_ln1, db_ln1 = _ln_bwd(dxn, x, ln1w, m1, r1, (need[0], need[2], need[3]), into=dx1)
        return (dx, dy, dw_ln1, db_ln1, dw_mw, dw_mh, dw_p, db_p, *d_mlp, None, None)


def _lin(m):
    return m.weight, m.bias


def dgab_autograd(x, y, blk):
    """DGAB `blk` (tps_pp.DGAB) on x (N, C, H, W) and the point map y (N, C, T) (en_feat, flattened), differentiable:
    `tpspp_plane_ln_*`, `tpspp_dgab_pool_*`, `tpspp_dgab_gate_*`, `tpspp_mm_f32`, `tpspp_linear_bwd_weight`, `tpspp_act_bwd`.
    The backward honours `needs_input_grad`: no launch for a frozen layer's parameters or an input without a gradient."""
    x = _chk("dgab_autograd x", x, 4)
    y = _chk("dgab_autograd y", y, 3)
    at = blk.attn
    if at.mlp_w[0].bias is not None or at.mlp_h[0].bias is not None:
        raise ValueError("dgab_autograd: qkv_bias=True is not supported (the reference builds DGAB without it)")
    if blk.skip_lam != 1.0:
        raise ValueError("dgab_autograd: skip_lam must be 1")
    n1, n2 = blk.norm1, blk.norm2
    return _DgabFunction.apply(x, y, n1.weight, n1.bias, at.mlp_w[0].weight, at.mlp_h[0].weight, *_lin(at.proj),
                               n2.weight, n2.bias, *_lin(blk.mlp.fc1), *_lin(blk.mlp.fc2), float(n1.eps), float(n2.eps))


class _ScoreFunction(torch.autograd.Function):
    """The attention score (`tps_pp.py:293-312`): S (N, F, H*W) = tanh(scale * p_linear(en) . feat_linear(de)), the
    (N, F, n) buffer the warp reads (its (N, n, F) transpose is the reference's pc_score).  Saves the Linear layers'
    outputs and S."""

    @staticmethod
    def forward(ctx, de, en, f1w, f1b, f2w, f2b, p1w, p1b, p2w, p2b, scale):
        N = de.shape[0]
        dd, de_ = _nchw_tokens(de), _nchw_tokens(en)
        HW, F, D = dd[1], de_[1], f2w.shape[0]
        a1 = linear_fwd(de, dd, f1w, f1b)
        a = linear_fwd(a1, _dense(N * HW, f1w.shape[0]), f2w, f2b)
        p1 = linear_fwd(en, de_, p1w, p1b)
        b = linear_fwd(p1, _dense(N * F, p1w.shape[0]), p2w, p2b)
        S = torch.empty((N, F, HW), device=de.device, dtype=torch.float32)
        mm(b, (F * D, D, 1), a, (HW * D, D, 1), S, (F * HW, HW, 1), N, F, HW, D, epi=3, alpha=scale)
        ctx.scale = scale
        ctx.save_for_backward(de, en, a1, a, p1, b, S, f1w, f2w, p1w, p2w)
        return S

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gS):
        de, en, a1, a, p1, b, S, f1w, f2w, p1w, p2w = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:10]):
            return (None,) * 11
        N = de.shape[0]
        dd, de_ = _nchw_tokens(de), _nchw_tokens(en)
        HW, F, D = dd[1], de_[1], f2w.shape[0]
        dev = de.device
        dT = act_bwd(ACT_TANH, gS.float().contiguous(), S, ctx.scale)
        res = [None] * 11
        if need[0] or any(need[2:6]):
            da = torch.empty((N * HW, D), device=dev, dtype=torch.float32)
            mm(dT, (F * HW, 1, HW), b, (F * D, 1, D), da, (HW * D, D, 1), N, HW, D, F)
            res[0], *res[2:6] = _two_linear_bwd(da, a1, f2w, de, dd, f1w, (need[0], *need[2:6]))
            del da
        if need[1] or any(need[6:10]):
            db = torch.empty((N * F, D), device=dev, dtype=torch.float32)
            mm(dT, (F * HW, HW, 1), a, (HW * D, 1, D), db, (F * D, D, 1), N, F, D, HW)
            res[1], *res[6:10] = _two_linear_bwd(db, p1, p2w, en, de_, p1w, (need[1], *need[6:10]))
        return tuple(res)


def score_autograd(de_feat, en_feat, tpe):
    """Differentiable score of `Transformation_Parameter_Estimation` `tpe` on de_feat (N, C, H, W) and en_feat (N, C, h, w):
    returns the (N, F, H*W) buffer; `.transpose(1, 2)` is the reference's (N, H*W, F) pc_score."""
    de_feat = _chk("score_autograd de_feat", de_feat, 4)
    en_feat = _chk("score_autograd en_feat", en_feat, 4)
    f, p = tpe.feat_linear, tpe.p_linear
    return _ScoreFunction.apply(de_feat, en_feat, *_lin(f[0]), *_lin(f[1]), *_lin(p[0]), *_lin(p[1]), float(tpe.scale))


class _CbamFunction(torch.autograd.Function):
    """CBAM (`tps_pp.py:27-82`): `tpspp_cbam_train_fwd` / `tpspp_cbam_bwd` (the backward recomputes the gates)."""

    @staticmethod
    def forward(ctx, x, w1, w2, cw, cb):
        N, C, H, W = x.shape
        Cr = w1.shape[0]
        out = torch.empty_like(x)
        ca = torch.empty((N, C), device=x.device, dtype=torch.float32)
        sa = torch.empty((N, H * W), device=x.device, dtype=torch.float32)
        _call("tpspp_cbam_train_fwd", x, x, w1, w2, cw, cb, N, C, Cr, H, W, out, ca, sa)
        ctx.save_for_backward(x, w1, w2, cw, cb)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, w1, w2, cw, cb = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:5]):
            return (None,) * 5
        N, C, H, W = x.shape
        Cr = w1.shape[0]
        dev = x.device
        gout = gout.float().contiguous()
        dx = torch.empty_like(x)          # the kernel forms dx on the way to the parameter gradients in any case
        g = [torch.empty(t.shape, device=dev, dtype=torch.float32) if need[i + 1] else None
             for i, t in enumerate((w1, w2, cw, cb))]
        ws, n = _ws_n(cbam_bwd_workspace_floats(N, C, Cr), dev)
        _call("tpspp_cbam_bwd", x, gout, x, w1, w2, cw, cb, N, C, Cr, H, W, dx, *g, ws, n)
        return (dx if need[0] else None, *g)


def cbam_bwd_workspace_floats(N, C, Cr):
    return _query("tpspp_cbam_bwd_workspace_floats", N, C, Cr)


def cbam_autograd(x, mod):
    """CBAM module `mod` (tps_pp.CBAM) on x (N, C, H, W), differentiable, HIP forward and backward."""
    x = _chk("cbam_autograd x", x, 4)
    ca, sa = mod.channel_attention, mod.spatial_attention
    w1, w2 = ca.shared_MLP[0].weight, ca.shared_MLP[2].weight
    if ca.shared_MLP[0].bias is not None or ca.shared_MLP[2].bias is not None or tuple(sa.conv2d.kernel_size) != (3, 3):
        raise ValueError("cbam_autograd: expects the reference's CBAM (bias-free shared MLP, 3x3 spatial conv)")
    return _CbamFunction.apply(x, w1, w2, sa.conv2d.weight, sa.conv2d.bias)


class _TpePointsFunction(torch.autograd.Function):
    """Control points (`tps_pp.py:321-323`): localization_fc2(relu(fc1b(relu(fc1a(tokens)))).view(N, -1)) on
    `tpspp_mm_f32`, backward on `tpspp_mm_f32` / `tpspp_linear_bwd_weight` / `tpspp_act_bwd`."""

    @staticmethod
    def forward(ctx, en, aw, ab, bw, bb, cw, cb):
        N = en.shape[0]
        de_ = _nchw_tokens(en)
        T = de_[1]
        h1 = linear_fwd(en, de_, aw, ab, epi=1)
        h2 = linear_fwd(h1, _dense(N * T, aw.shape[0]), bw, bb, epi=1)
        cp = linear_fwd(h2, _dense(N, T * bw.shape[0]), cw, cb)
        ctx.save_for_backward(en, h1, h2, aw, bw, cw)
        return cp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gcp):
        en, h1, h2, aw, bw, cw = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:7]):
            return (None,) * 7
        N = en.shape[0]
        de_ = _nchw_tokens(en)
        T = de_[1]
        Hb = bw.shape[0]
        gcp = gcp.float().contiguous()
        res = [None] * 7
        res[5], res[6] = linear_bwd_weight(gcp, h2, _dense(N, T * Hb), cw.shape[0], T * Hb, need[5], need[6])
        if any(need[:5]):
            dh2 = linear_bwd_data(gcp, cw)          # (N, T * Hb): the (N * T, Hb) rows of fc1b
            act_bwd(ACT_RELU, dh2, h2, out=dh2)
            res[:5] = _two_linear_bwd(dh2, h1, bw, en, de_, aw, need[:5], act=ACT_RELU)
        return tuple(res)


def tpe_points_autograd(en_feat, tpe):
    """Differentiable control points of `tpe` from en_feat (N, C, h, w): (N, F, 2)."""
    en_feat = _chk("tpe_points_autograd en_feat", en_feat, 4)
    f1, f2 = tpe.localization_fc1, tpe.localization_fc2
    cp = _TpePointsFunction.apply(en_feat, *_lin(f1[0]), *_lin(f1[2]), *_lin(f2))
    return cp.view(en_feat.shape[0], tpe.num_fiducial, 2)


# ---- BatchNorm training kernels (tpspp_bn_train.hip): training the backbone on the HIP kernels ---------------------------
def _bn_dims(who, z):
    z = _chk(f"{who} z", z, 4)
    N, C, H, W = z.shape
    return z, N, C, H * W


def _chk_vec(who, name, t, C, dev):
    t = _chk(f"{who} {name}", t, 1)
    if t.shape[0] != C or t.device != dev:
        raise ValueError(f"{who}: {name} must be ({C},) on {dev}, got {tuple(t.shape)} on {t.device}")
    return t


def _chk_like(who, name, t, ref):
    t = _chk(f"{who} {name}", t, 4)
    if t.shape != ref.shape or t.device != ref.device:
        raise ValueError(f"{who}: {name} must be {tuple(ref.shape)} on {ref.device}, got {tuple(t.shape)} on {t.device}")
    return t


def bn_stats_workspace_floats(N, C, HW):
    """Floats of workspace `bn_train_stats` needs (`tpspp_bn_stats_workspace_floats`): 3 per channel and slice of 4096."""
    return _query("tpspp_bn_stats_workspace_floats", N, C, HW)


def bn_bwd_reduce_workspace_floats(N, C, HW):
    """Floats of workspace `bn_bwd_reduce` needs (`tpspp_bn_bwd_reduce_workspace_floats`)."""
    return _query("tpspp_bn_bwd_reduce_workspace_floats", N, C, HW)


def bn_train_stats(z, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, num_batches_tracked=None):
    """Batch statistics of a training-mode BatchNorm2d (`tpspp_bn_train_stats`): (mean, rstd) per channel of z (N, C, H, W),
    rstd = 1 / sqrt(biased var + eps).  With running_mean / running_var they are updated on the device with PyTorch's rule
    (momentum None: the cumulative average, 1 / num_batches_tracked), and num_batches_tracked (int64) is incremented."""
    z, N, C, HW = _bn_dims("bn_train_stats", z)
    dev = z.device
    if (running_mean is None) != (running_var is None):
        raise ValueError("bn_train_stats: running_mean and running_var go together")
    if running_mean is not None:
        for name, t in (("running_mean", running_mean), ("running_var", running_var)):
            if not t.is_contiguous():
                raise ValueError(f"bn_train_stats: {name} must be contiguous (it is updated in place)")
            _chk_vec("bn_train_stats", name, t, C, dev)
    if num_batches_tracked is not None:
        if num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1 or num_batches_tracked.device != dev:
            raise ValueError("bn_train_stats: num_batches_tracked must be one int64 on z's device")
    if momentum is None and running_mean is not None and num_batches_tracked is None:
        raise ValueError("bn_train_stats: momentum=None needs num_batches_tracked")
    mean = torch.empty((C,), device=dev, dtype=torch.float32)
    rstd = torch.empty((C,), device=dev, dtype=torch.float32)
    ws, nws = _ws_n(bn_stats_workspace_floats(N, C, HW), dev)
    _call("tpspp_bn_train_stats", z, z, N, C, HW, float(eps), -1.0 if momentum is None else float(momentum),
          num_batches_tracked, running_mean, running_var, mean, rstd, ws, nws)
    return mean, rstd


def bn_eval_stats(running_mean, running_var, eps=1e-5):
    """(mean, rstd) an eval-mode BatchNorm2d normalises with (`tpspp_bn_eval_stats`): a copy of running_mean and
    1 / sqrt(running_var + eps)."""
    rm = _chk("bn_eval_stats running_mean", running_mean, 1)
    rv = _chk_vec("bn_eval_stats", "running_var", running_var, rm.shape[0], rm.device)
    mean, rstd = torch.empty_like(rm), torch.empty_like(rm)
    _call("tpspp_bn_eval_stats", rm, rm, rv, rm.shape[0], float(eps), mean, rstd)
    return mean, rstd


def bn_apply(za, stats_a, gamma_a, beta_a, residual=None, zb=None, stats_b=None, gamma_b=None, beta_b=None, relu=True):
    """y = relu(gamma_a (za - mean_a) rstd_a + beta_a + r) (`tpspp_bn_apply_fwd`), r = nothing, `residual`, or the second
    normalised branch gamma_b (zb - mean_b) rstd_b + beta_b.  stats_* = (mean, rstd) from `bn_train_stats` / `bn_eval_stats`."""
    who = "bn_apply"
    za, N, C, HW = _bn_dims(who, za)
    dev = za.device
    ma, ra = (_chk_vec(who, n, t, C, dev) for n, t in zip(("mean_a", "rstd_a"), stats_a))
    ga, ba = _chk_vec(who, "gamma_a", gamma_a, C, dev), _chk_vec(who, "beta_a", beta_a, C, dev)
    if residual is not None and zb is not None:
        raise ValueError("bn_apply: a residual tensor or a second branch, not both")
    res_mode, mb = 0, (None,) * 5
    if residual is not None:
        res_mode, residual = 1, _chk_like(who, "residual", residual, za)
    elif zb is not None:
        res_mode = 2
        mb = (_chk_like(who, "zb", zb, za),) + tuple(_chk_vec(who, n, t, C, dev) for n, t in
                                                       zip(("mean_b", "rstd_b", "gamma_b", "beta_b"),
                                                           (*stats_b, gamma_b, beta_b)))
    y = torch.empty_like(za)
    _call("tpspp_bn_apply_fwd", za, za, ma, ra, ga, ba, res_mode, residual, *mb, int(bool(relu)), N, C, HW, y)
    return y


def bn_bwd_reduce(dy, y, za, stats_a, zb=None, stats_b=None, relu=True):
    """Per-channel sums of dr = dy [y > 0] (relu) or dy (`tpspp_bn_bwd_reduce`): (sum dr, sum dr xhat_a, sum dr xhat_b or
    None) = the beta gradient and the gamma gradients of the branches.  Fixed split, bitwise reproducible."""
    who = "bn_bwd_reduce"
    za, N, C, HW = _bn_dims(who, za)
    dev = za.device
    dy = _chk_like(who, "dy", dy, za)
    y = _chk_like(who, "y", y, za) if relu else None
    ma, ra = (_chk_vec(who, n, t, C, dev) for n, t in zip(("mean_a", "rstd_a"), stats_a))
    mb = rb = sxb = None
    if zb is not None:
        zb = _chk_like(who, "zb", zb, za)
        mb, rb = (_chk_vec(who, n, t, C, dev) for n, t in zip(("mean_b", "rstd_b"), stats_b))
        sxb = torch.empty((C,), device=dev, dtype=torch.float32)
    sdr = torch.empty((C,), device=dev, dtype=torch.float32)
    sxa = torch.empty((C,), device=dev, dtype=torch.float32)
    ws, nws = _ws_n(bn_bwd_reduce_workspace_floats(N, C, HW), dev)
    _call("tpspp_bn_bwd_reduce", dy, dy, y, int(bool(relu)), za, ma, ra, zb, mb, rb, N, C, HW, sdr, sxa, sxb, ws, nws)
    return sdr, sxa, sxb


def bn_bwd_data(dy, y, za=None, stats_a=None, gamma_a=None, sums=None, train_a=True, zb=None, stats_b=None, gamma_b=None,
                train_b=True, relu=True, dres=None, dres_mode=0, want_a=True, want_b=None):
    """Input gradients of the normalised branches (`tpspp_bn_bwd_data`): (dza | None, dzb | None).  sums = `bn_bwd_reduce`'s
    (sum dr, sum dr xhat_a, sum dr xhat_b); train_* False: an eval-mode BatchNorm (dz = gamma rstd dr).  dres_mode 1 writes
    dr into `dres`, 2 adds it (the shortcut's gradient); with no branch and relu=False that is the ordered sum dres + dy."""
    who = "bn_bwd_data"
    dy = _chk(f"{who} dy", dy, 4)
    N, C, H, W = dy.shape
    HW, dev = H * W, dy.device
    y = _chk_like(who, "y", y, dy) if relu else None
    want_a = want_a and za is not None
    want_b = (zb is not None) if want_b is None else (want_b and zb is not None)
    if sums is None and ((want_a and train_a) or (want_b and train_b)):
        raise ValueError("bn_bwd_data: a training-mode branch needs the sums of bn_bwd_reduce")
    sdr, sxa, sxb = sums if sums is not None else (None, None, None)
    args_a = [None] * 6
    args_b = [None] * 6
    dza = dzb = None
    if want_a:
        dza = torch.empty_like(dy)
        args_a = [_chk_like(who, "za", za, dy)] + [_chk_vec(who, n, t, C, dev) for n, t in
                                                    zip(("mean_a", "rstd_a", "gamma_a"), (*stats_a, gamma_a))]
        args_a += [_chk_vec(who, "sum_dr_xa", sxa, C, dev) if train_a else None, dza]
    if want_b:
        dzb = torch.empty_like(dy)
        args_b = [_chk_like(who, "zb", zb, dy)] + [_chk_vec(who, n, t, C, dev) for n, t in
                                                    zip(("mean_b", "rstd_b", "gamma_b"), (*stats_b, gamma_b))]
        args_b += [_chk_vec(who, "sum_dr_xb", sxb, C, dev) if train_b else None, dzb]
    if (want_a and train_a) or (want_b and train_b):
        sdr = _chk_vec(who, "sum_dr", sdr, C, dev)
    if dres_mode:
        if not isinstance(dres, torch.Tensor) or not dres.is_contiguous():
            raise ValueError("bn_bwd_data: dres must be a contiguous tensor (it is written in place)")
        dres = _chk_like(who, "dres", dres, dy)
    _call("tpspp_bn_bwd_data", dy, dy, y, int(bool(relu)), *args_a[:5], int(bool(train_a)), args_a[5],
          *args_b[:5], int(bool(train_b)), args_b[5], sdr, dres, int(dres_mode), N, C, HW)
    return dza, dzb


def _bn_stats_of(z, spec):
    """(mean, rstd) a BatchNorm normalises z with, by its own mode (spec: `_bn_spec`)."""
    training, eps, momentum, rm, rv, nbt, name = spec
    if training:
        if z.shape[0] * z.shape[2] * z.shape[3] == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {z.shape}")
        return bn_train_stats(z, eps, momentum, rm, rv, nbt)
    return bn_eval_stats(rm, rv, eps)


def _bn_spec(bn, name):
    if not isinstance(bn, torch.nn.BatchNorm2d):
        raise ValueError(f"{name}: expected nn.BatchNorm2d, got {type(bn).__name__}")
    if not bn.affine or not bn.track_running_stats:
        raise ValueError(f"{name}: the HIP training path needs BatchNorm2d(affine=True, track_running_stats=True)")
    return (bool(bn.training), float(bn.eps), bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked, name)


def _conv_spec(conv, name, bias_ok=False):
    """(kernel, stride) of an nn.Conv2d the HIP kernels take: 1x1 / 3x3, 'same' padding, stride 1 or 2, no dilation or groups."""
    if not isinstance(conv, torch.nn.Conv2d):
        raise ValueError(f"{name}: expected nn.Conv2d, got {type(conv).__name__}")
    k = conv.kernel_size[0]
    st = tuple(int(s) for s in conv.stride)
    if (conv.kernel_size[1] != k or k not in (1, 3) or tuple(conv.padding) != ((k - 1) // 2,) * 2 or
            tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros" or
            any(s not in (1, 2) for s in st) or (conv.bias is not None and not bias_ok)):
        raise ValueError(f"{name}: the HIP training path takes 1x1 / 3x3 convolutions with 'same' zero padding, stride 1 or 2"
                         f"{', a bias' if bias_ok else ', no bias'}, no dilation and no groups")
    return k, st


class _BnStemFunction(torch.autograd.Function):
    """y = relu(bn(conv(x) + bias)): HIP forward (`conv2d`, `bn_train_stats` / `bn_eval_stats`, `bn_apply`) and backward
    (`bn_bwd_reduce`, `bn_bwd_data`, `conv2d_bwd_weight`, `conv2d_bwd_data`).  Saves z, y and the per-channel mean / rstd."""

    @staticmethod
    def forward(ctx, x, w, cb, g, b, cfg):
        cw, (k, st), spec = cfg
        x = x.float().contiguous()
        z = conv2d([x], cw, st, relu=False)
        mean, rstd = _bn_stats_of(z, spec)
        y = bn_apply(z, (mean, rstd), g, b, relu=True)
        ctx.cfg = (k, st, spec[0], cb is not None)
        ctx.save_for_backward(x, w, g, z, y, mean, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        k, st, train, has_bias = ctx.cfg
        x, w, g, z, y, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        gy = gy.float().contiguous()
        need_z = need[0] or need[1] or (has_bias and need[2])
        dx = dw = dcb = dg = db = None
        sums = (None, None, None)
        if train or need[3] or need[4]:
            sums = bn_bwd_reduce(gy, y, z, (mean, rstd), relu=True)
            dg = sums[1] if need[3] else None
            db = sums[0] if need[4] else None
        if need_z:
            dz, _ = bn_bwd_data(gy, y, z, (mean, rstd), g, sums, train, relu=True)
            if need[1] or (has_bias and need[2]):
                dw, dcb = conv2d_bwd_weight([x], dz, k, st, relu=False, want_weight=need[1], want_bias=has_bias and need[2])
            if need[0]:
                dx = conv2d_bwd_data(dz, w, [x], st, relu=False)[0]
        return dx, dw, dcb, dg, db, None


def bn_stem_autograd(x, conv, bn, cw=None, name="stem"):
    """relu(bn(conv(x))) -- ResNetABI_v2_large's stem -- inside an autograd graph on the HIP kernels.  conv: nn.Conv2d
    (bias allowed); bn: nn.BatchNorm2d, which follows its own mode (.training: batch statistics, running statistics and
    num_batches_tracked updated on the device; .eval(): running statistics).  cw: the forward's ConvWeight (a cache the
    caller keys on the parameters' versions), built on the device here if None.  The backward honours
    `needs_input_grad`."""
    _chk_gpu(name, x)
    kst = _conv_spec(conv, f"{name} conv", bias_ok=True)
    spec = _bn_spec(bn, f"{name} bn")
    if cw is None:
        cw = prep_conv_weight_device(conv.weight, conv.bias)
    return _BnStemFunction.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, (cw, kst, spec))


class _BnBlockFunction(torch.autograd.Function):
    """A BasicBlock, y = relu(bn2(conv2(relu(bn1(conv1 x)))) + shortcut), shortcut = x or bn_d(conv_d x): HIP forward and
    backward.  Saves z1, h = relu(bn1(z1)), z2, z_d, y and the per-channel mean / rstd of each BatchNorm."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, wd, gd, bd, cfg):
        (cw1, cw2, cwd), (kst1, kst2, kstd), (s1, s2, sd) = cfg
        x = x.float().contiguous()
        z1 = conv2d([x], cw1, kst1[1], relu=False)
        st1 = _bn_stats_of(z1, s1)
        h = bn_apply(z1, st1, g1, b1, relu=True)
        z2 = conv2d([h], cw2, kst2[1], relu=False)
        st2 = _bn_stats_of(z2, s2)
        if cwd is None:
            zd, std = None, (None, None)
            y = bn_apply(z2, st2, g2, b2, residual=x, relu=True)
        else:
            zd = conv2d([x], cwd, kstd[1], relu=False)
            std = _bn_stats_of(zd, sd)
            y = bn_apply(z2, st2, g2, b2, zb=zd, stats_b=std, gamma_b=gd, beta_b=bd, relu=True)
        ctx.cfg = (kst1, kst2, kstd, s1[0], s2[0], None if sd is None else sd[0], cwd is not None)
        ctx.save_for_backward(x, w1, g1, w2, g2, wd, gd, z1, h, z2, zd, y, *st1, *st2, *std)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        kst1, kst2, kstd, t1, t2, td, down = ctx.cfg
        x, w1, g1, w2, g2, wd, gd, z1, h, z2, zd, y, m1, r1, m2, r2, md, rd = ctx.saved_tensors
        need = ctx.needs_input_grad       # x, w1, g1, b1, w2, g2, b2, wd, gd, bd
        gy = gy.float().contiguous()
        grads = [None] * 11
        # relu(bn2(z2) + shortcut): the sums of both normalised branches in one pass over dr = gy [y > 0]
        sdr, sx2, sxd = bn_bwd_reduce(gy, y, z2, (m2, r2), zd, (md, rd) if down else None, relu=True)
        grads[5] = sx2 if need[5] else None
        grads[6] = sdr if need[6] else None
        if down:
            grads[8] = sxd if need[8] else None
            grads[9] = sdr.clone() if need[9] else None        # both betas see sum dr; two tensors for two parameters
        up = need[0] or need[1] or need[2] or need[3]       # anything behind conv2's input h
        want_d = down and (need[0] or need[7])
        dz2 = dzd = None
        if need[4] or up or want_d:
            dz2, dzd = bn_bwd_data(gy, y, z2, (m2, r2), g2, (sdr, sx2, sxd), t2, zb=zd, stats_b=(md, rd), gamma_b=gd,
                                   train_b=bool(td), relu=True, want_a=need[4] or up, want_b=want_d)
        if need[4]:
            grads[4] = conv2d_bwd_weight([h], dz2, kst2[0], kst2[1], relu=False, want_bias=False)[0]
        if down and need[7]:
            grads[7] = conv2d_bwd_weight([x], dzd, kstd[0], kstd[1], relu=False, want_bias=False)[0]
        if up:
            dh = conv2d_bwd_data(dz2, w2, [h], kst2[1], relu=False)[0]
            s1 = bn_bwd_reduce(dh, h, z1, (m1, r1), relu=True)
            grads[2] = s1[1] if need[2] else None
            grads[3] = s1[0] if need[3] else None
            if need[0] or need[1]:
                dz1, _ = bn_bwd_data(dh, h, z1, (m1, r1), g1, s1, t1, relu=True)
                if need[1]:
                    grads[1] = conv2d_bwd_weight([x], dz1, kst1[0], kst1[1], relu=False, want_bias=False)[0]
                if need[0]:
                    dx = conv2d_bwd_data(dz1, w1, [x], kst1[1], relu=False)[0]
                    # + the shortcut's gradient, added in this order: dx = conv1's data gradient + shortcut
                    if down:
                        dxd = conv2d_bwd_data(dzd, wd, [x], kstd[1], relu=False)[0]
                        bn_bwd_data(dxd, None, relu=False, dres=dx, dres_mode=2, want_a=False, want_b=False)
                    else:
                        bn_bwd_data(gy, y, relu=True, dres=dx, dres_mode=2, want_a=False, want_b=False)
                    grads[0] = dx
        return tuple(grads)


def bn_block_autograd(x, blk, cws=None, name="block"):
    """A BasicBlock (conv1, bn1, conv2, bn2, optional downsample = Sequential(conv, bn)) inside an autograd graph on the HIP
    kernels: every convolution on `conv2d` / `conv2d_bwd_*` (relu = 0), every BatchNorm + shortcut + ReLU on the
    tpspp_bn_train.hip kernels.  Each BatchNorm follows its own mode.  cws: the forward's ConvWeights (conv1, conv2,
    downsample conv or None), built on the device here if None.  The backward honours `needs_input_grad`: no data-gradient
    launch when x needs none, no weight-gradient launch for a frozen convolution; a frozen BatchNorm still passes its
    input gradient on."""
    _chk_gpu(name, x)
    kst1 = _conv_spec(blk.conv1, f"{name}.conv1")
    kst2 = _conv_spec(blk.conv2, f"{name}.conv2")
    s1, s2 = _bn_spec(blk.bn1, f"{name}.bn1"), _bn_spec(blk.bn2, f"{name}.bn2")
    ds = blk.downsample
    if ds is not None:
        if not isinstance(ds, torch.nn.Sequential) or len(ds) != 2:
            raise ValueError(f"{name}.downsample: the HIP training path takes Sequential(Conv2d, BatchNorm2d)")
        kstd, sd = _conv_spec(ds[0], f"{name}.downsample.0"), _bn_spec(ds[1], f"{name}.downsample.1")
        wd, gd, bd = ds[0].weight, ds[1].weight, ds[1].bias
    else:
        kstd = sd = wd = gd = bd = None
    if cws is None:
        cws = (prep_conv_weight_device(blk.conv1.weight), prep_conv_weight_device(blk.conv2.weight),
               None if ds is None else prep_conv_weight_device(wd))
    return _BnBlockFunction.apply(x, blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, blk.conv2.weight, blk.bn2.weight,
                                  blk.bn2.bias, wd, gd, bd, (tuple(cws), (kst1, kst2, kstd), (s1, s2, sd)))


# ---- BatchNorm + ReLU + MaxPool2d(2, 2) in one pass (tpspp_bn_pool_train.hip): training the classic rectifier's
# localisation network (TPSPreprocessor.set_train_backend("hip")) -----------------------------------------------------------
def _bn_pool_args(who, z, stats, gamma, beta):
    """z (N, C, H, W) with H, W >= 2 and its per-channel (mean, rstd, gamma, beta), checked."""
    z = _chk(f"{who} z", z, 4)
    N, C, H, W = z.shape
    if H < 2 or W < 2:
        raise ValueError(f"{who}: a 2x2 window needs H, W >= 2, got {tuple(z.shape)}")
    vecs = [_chk_vec(who, n, t, C, z.device) for n, t in zip(("mean", "rstd", "gamma", "beta"), (*stats, gamma, beta))]
    return z, (N, C, H, W), vecs


def _chk_pooled_grad(who, dp, dims, dev):
    N, C, H, W = dims
    dp = _chk(f"{who} dp", dp, 4)
    if tuple(dp.shape) != (N, C, H // 2, W // 2) or dp.device != dev:
        raise ValueError(f"{who}: dp must be {(N, C, H // 2, W // 2)} on {dev}, got {tuple(dp.shape)} on {dp.device}")
    return dp


def bn_pool2x2_fwd(z, stats, gamma, beta):
    """maxpool2x2(relu(gamma (z - mean) rstd + beta)) as one kernel (`tpspp_bn_pool2x2_fwd`): (N, C, H/2, W/2) with the bits
    of `maxpool2x2(bn_apply(z, stats, gamma, beta, relu=True))`; the activated map is never written."""
    who = "bn_pool2x2_fwd"
    z, (N, C, H, W), vecs = _bn_pool_args(who, z, stats, gamma, beta)
    p = torch.empty((N, C, H // 2, W // 2), device=z.device, dtype=torch.float32)
    _call("tpspp_bn_pool2x2_fwd", z, z, *vecs, N, C, H, W, p)
    return p


def bn_pool2x2_bwd_reduce_workspace_floats(N, C, H, W):
    """Floats of workspace `bn_pool2x2_bwd_reduce` needs: 2 per channel and slice of 4096 elements of N*H*W."""
    return _query("tpspp_bn_pool2x2_bwd_reduce_workspace_floats", N, C, H, W)


def bn_pool2x2_bwd_reduce(dp, z, stats, gamma, beta):
    """(sum dr, sum dr xhat) per channel (`tpspp_bn_pool2x2_bwd_reduce`), dr = dp at each window's selected element where
    the activation is positive and 0 elsewhere: the beta and gamma gradients.  Fixed split, bitwise reproducible."""
    who = "bn_pool2x2_bwd_reduce"
    z, (N, C, H, W), vecs = _bn_pool_args(who, z, stats, gamma, beta)
    dev = z.device
    dp = _chk_pooled_grad(who, dp, (N, C, H, W), dev)
    sdr = torch.empty((C,), device=dev, dtype=torch.float32)
    sx = torch.empty((C,), device=dev, dtype=torch.float32)
    ws, nws = _ws_n(bn_pool2x2_bwd_reduce_workspace_floats(N, C, H, W), dev)
    _call("tpspp_bn_pool2x2_bwd_reduce", dp, dp, z, *vecs, N, C, H, W, sdr, sx, ws, nws)
    return sdr, sx


def bn_pool2x2_bwd_data(dp, z, stats, gamma, beta, sums=None, train=True):
    """dz (N, C, H, W) of `bn_pool2x2_fwd` (`tpspp_bn_pool2x2_bwd_data`).  sums = `bn_pool2x2_bwd_reduce`'s pair, needed
    with train=True (batch statistics); train=False (running statistics): dz = gamma rstd dr."""
    who = "bn_pool2x2_bwd_data"
    z, (N, C, H, W), vecs = _bn_pool_args(who, z, stats, gamma, beta)
    dev = z.device
    dp = _chk_pooled_grad(who, dp, (N, C, H, W), dev)
    sdr = sx = None
    if train:
        if sums is None:
            raise ValueError("bn_pool2x2_bwd_data: a training-mode BatchNorm needs the sums of bn_pool2x2_bwd_reduce")
        sdr, sx = (_chk_vec(who, n, t, C, dev) for n, t in zip(("sum_dr", "sum_dr_x"), sums))
    dz = torch.empty_like(z)
    _call("tpspp_bn_pool2x2_bwd_data", dp, dp, z, *vecs, sdr, sx, int(bool(train)), N, C, H, W, dz)
    return dz


def global_avgpool_bwd(g, hw):
    """Backward of `global_avgpool` (`tpspp_global_avgpool_bwd`): g (N, C) -> (N, C, H, W) = g / (H W), hw = (H, W)."""
    g = _chk("global_avgpool_bwd g", g, 2)
    N, C = g.shape
    H, W = int(hw[0]), int(hw[1])
    dx = torch.empty((N, C, H, W), device=g.device, dtype=torch.float32)
    _call("tpspp_global_avgpool_bwd", g, g, N, C, H, W, dx)
    return dx


class _BnPoolFunction(torch.autograd.Function):
    """p = maxpool2x2(relu(bn(conv(x) + bias))): HIP forward (`conv2d`, `bn_train_stats` / `bn_eval_stats`,
    `bn_pool2x2_fwd`) and backward (`bn_pool2x2_bwd_reduce`, `bn_pool2x2_bwd_data`, `conv2d_bwd_weight`, `conv2d_bwd_data`).
    Saves x, w, z and the per-channel vectors; neither the activated map nor a selector (the backward rescans z)."""

    @staticmethod
    def forward(ctx, x, w, cb, g, b, cfg):
        cw, (k, st), spec = cfg
        x = x.float().contiguous()
        z = conv2d([x], cw, st, relu=False)
        mean, rstd = _bn_stats_of(z, spec)
        p = bn_pool2x2_fwd(z, (mean, rstd), g, b)
        ctx.cfg = (k, st, spec[0], cb is not None)
        ctx.save_for_backward(x, w, z, mean, rstd, g, b)
        return p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gp):
        k, st, train, has_bias = ctx.cfg
        x, w, z, mean, rstd, g, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        gp = gp.float().contiguous()
        need_z = need[0] or need[1] or (has_bias and need[2])
        dx = dw = dcb = dg = db = None
        sums = None
        if (train and need_z) or need[3] or need[4]:
            sums = bn_pool2x2_bwd_reduce(gp, z, (mean, rstd), g, b)
            dg = sums[1] if need[3] else None
            db = sums[0] if need[4] else None
        if need_z:
            dz = bn_pool2x2_bwd_data(gp, z, (mean, rstd), g, b, sums, train)
            if need[1] or (has_bias and need[2]):
                dw, dcb = conv2d_bwd_weight([x], dz, k, st, relu=False, want_weight=need[1], want_bias=has_bias and need[2])
            if need[0]:
                dx = conv2d_bwd_data(dz, w, [x], st, relu=False)[0]
        return dx, dw, dcb, dg, db, None


def bn_pool_autograd(x, conv, bn, cw=None, name="pooled layer"):
    """maxpool2x2(relu(bn(conv(x)))) -- a pooled layer of the classic rectifier's localisation network -- inside an autograd
    graph on the HIP kernels, the BatchNorm, the ReLU and the pool as one pass forward and backward.  conv, bn, cw and the
    handling of `needs_input_grad` as `bn_stem_autograd`: the BatchNorm follows its own mode (.training: batch statistics,
    running statistics and num_batches_tracked updated on the device; .eval(): running statistics)."""
    _chk_gpu(name, x)
    kst = _conv_spec(conv, f"{name} conv", bias_ok=True)
    spec = _bn_spec(bn, f"{name} bn")
    if cw is None:
        cw = prep_conv_weight_device(conv.weight, conv.bias)
    return _BnPoolFunction.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, (cw, kst, spec))


class _GlobalAvgPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = tuple(x.shape[2:])
        return global_avgpool(x.float())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return global_avgpool_bwd(g.float().contiguous(), ctx.hw)


def global_avgpool_autograd(x):
    """nn.AdaptiveAvgPool2d(1) -> (N, C) inside an autograd graph: `global_avgpool` and `global_avgpool_bwd`."""
    return _GlobalAvgPoolFunction.apply(_chk("global_avgpool_autograd x", x, 4))


class _TwoLinearFunction(torch.autograd.Function):
    """fc2(relu(fc1(x))) for x (N, K) on `tpspp_mm_f32`, backward on `_two_linear_bwd` (the `_TpePointsFunction` pattern)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x = x.float().contiguous()
        N, K = x.shape
        h = linear_fwd(x, _dense(N, K), w1, b1, epi=1)
        y = linear_fwd(h, _dense(N, w1.shape[0]), w2, b2)
        ctx.save_for_backward(x, h, w1, w2)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, h, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:5]):
            return (None,) * 5
        return tuple(_two_linear_bwd(gy.float().contiguous(), h, w2, x, _dense(*x.shape), w1, need[:5], act=ACT_RELU))


def two_linear_autograd(x, fc1, fc2):
    """fc2(relu(fc1(x))) of two nn.Linear layers on x (N, K), differentiable, on the HIP GEMM kernels."""
    x = _chk("two_linear_autograd x", x, 2)
    if x.shape[1] != fc1.in_features or fc2.in_features != fc1.out_features:
        raise ValueError(f"two_linear_autograd: x {tuple(x.shape)} does not fit Linear({fc1.in_features}, "
                         f"{fc1.out_features}) -> Linear({fc2.in_features}, {fc2.out_features})")
    return _TwoLinearFunction.apply(x, *_lin(fc1), *_lin(fc2))


# ---- training graph of the NRTR encoder (NRTREncoder.set_train_backend("hip"), tpspp_attn_train.hip) -------------------
# Scaled-dot-product attention with the valid_ratio key mask and dropout on the probabilities, forward and backward
# (include/tpspp_train_attn.h; every autograd path calls the `_ex` entry points of include/tpspp_train_dec.h, which add a
# per-key mask, a causal mask and separate row strides and without them give the same bits), and around it an encoder
# layer composed of the kernels above: `tpspp_plane_ln_*`, `tpspp_mm_f32` (q / k / v as one product, GELU as w_1's
# epilogue), `tpspp_linear_bwd_weight`, `tpspp_act_bwd`.  Each layer is two once-differentiable functions (norm1 -
# attention - fc, norm2 - w_1 - GELU - w_2); the two element-wise dropouts and the residual additions between them stay
# PyTorch element-wise ops.

_U64 = (1 << 64) - 1


def _row_stride(t):
    """Row stride of an (N, T, C) operand whose tokens lie one row stride apart with contiguous columns, else None."""
    N, T, C = t.shape
    if C > 1 and t.stride(2) != 1:
        return None
    if T > 1:
        ld = t.stride(1)
        if N > 1 and t.stride(0) != T * ld:
            return None
    else:
        ld = t.stride(0) if N > 1 else C
    return ld if ld >= C else None


def _attn_operands(who, q, k, v):
    """q (N, Tq, C), k / v (N, Tk, C) as `tpspp_attn_train_fwd_ex` takes them: q with a row stride of its own, one row
    stride for k and v (views of a fused (N, T, 2C) or (N, T, 3C) projection pass as they are), dense copies otherwise.
    -> (q, k, v, ld_q, ld_kv)"""
    for name, t in (("q", q), ("k", k), ("v", v)):
        _chk_gpu(f"{who} {name}", t)
        if t.dtype != torch.float32:
            raise TypeError(f"{who} {name}: expected float32, got {t.dtype}")
        if t.dim() != 3:
            raise ValueError(f"{who} {name}: expected (N, T, C), got {tuple(t.shape)}")
    if k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise ValueError(f"{who}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit together")
    if q.shape[2] % 64 or q.shape[2] == 0:
        raise ValueError(f"{who}: expected (N, T, 64 * heads) operands, got q {tuple(q.shape)}")
    ld_q = _row_stride(q)
    if ld_q is None:
        q, ld_q = q.contiguous(), q.shape[2]
    ld_kv = _row_stride(k)
    if ld_kv is None or ld_kv != _row_stride(v):
        k, v, ld_kv = k.contiguous(), v.contiguous(), k.shape[2]
    return q, k, v, ld_q, ld_kv


def _attn_valid_len(who, valid_len, N, dev):
    if valid_len is None:
        return None
    valid_len = _chk(f"{who} valid_len", valid_len, 1, (torch.int32,))
    if valid_len.shape[0] != N or valid_len.device != dev:
        raise ValueError(f"{who}: valid_len must be {N} int32 lengths on {dev}")
    return valid_len


def _attn_key_mask(who, key_mask, N, Tk, dev):
    """(N, Tk) bool or uint8 on the device, 0 = masked -> contiguous uint8, or None."""
    if key_mask is None:
        return None
    if not isinstance(key_mask, torch.Tensor) or key_mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{who}: key_mask must be a bool or uint8 tensor")
    if tuple(key_mask.shape) != (N, Tk) or key_mask.device != dev:
        raise ValueError(f"{who}: key_mask must be ({N}, {Tk}) on {dev}, got {tuple(key_mask.shape)} on {key_mask.device}")
    key_mask = key_mask.contiguous()
    return key_mask.view(torch.uint8) if key_mask.dtype == torch.bool else key_mask


def _attn_rate(who, drop_p):
    if not 0.0 <= float(drop_p) < 1.0:
        raise ValueError(f"{who}: drop_p must lie in [0, 1), got {drop_p!r}")
    return float(drop_p)


def attn_train_fwd(q, k, v, ld, N, C, heads, Tq, Tk, valid_len, drop_p, seed, offset):
    """`tpspp_attn_train_fwd` on raw operands (rows `ld` elements apart): (out (N*Tq, C), lse (N, heads, Tq))."""
    out = torch.empty((N * Tq, C), device=q.device, dtype=torch.float32)
    lse = torch.empty((N, heads, Tq), device=q.device, dtype=torch.float32)
    _call("tpspp_attn_train_fwd", q, q, k, v, ld, N, C, heads, Tq, Tk, valid_len, float(drop_p), int(seed) & _U64,
          int(offset) & _U64, out, lse)
    return out, lse


def attn_train_bwd(d_out, q, k, v, ld, out, lse, N, C, heads, Tq, Tk, valid_len, drop_p, seed, offset, dq, dk, dv, ld_grad):
    """`tpspp_attn_train_bwd`: writes dq (N*Tq rows), dk, dv (N*Tk rows), rows `ld_grad` elements apart."""
    _call("tpspp_attn_train_bwd", d_out, d_out, q, k, v, ld, out, lse, N, C, heads, Tq, Tk, valid_len, float(drop_p),
          int(seed) & _U64, int(offset) & _U64, dq, dk, dv, ld_grad)


def attn_train_fwd_ex(q, ld_q, k, v, ld_kv, N, C, heads, Tq, Tk, valid_len, key_mask, causal, drop_p, seed, offset):
    """`tpspp_attn_train_fwd_ex` on raw operands: (out (N*Tq, C), lse (N, heads, Tq))."""
    out = torch.empty((N * Tq, C), device=q.device, dtype=torch.float32)
    lse = torch.empty((N, heads, Tq), device=q.device, dtype=torch.float32)
    _call("tpspp_attn_train_fwd_ex", q, q, ld_q, k, v, ld_kv, N, C, heads, Tq, Tk, valid_len, key_mask, int(bool(causal)),
          float(drop_p), int(seed) & _U64, int(offset) & _U64, out, lse)
    return out, lse


def attn_train_bwd_ex(d_out, q, ld_q, k, v, ld_kv, out, lse, N, C, heads, Tq, Tk, valid_len, key_mask, causal, drop_p, seed,
                      offset, dq, ld_dq, dk, dv, ld_dkv):
    """`tpspp_attn_train_bwd_ex`: writes dq (N*Tq rows, `ld_dq` apart), dk, dv (N*Tk rows, `ld_dkv` apart)."""
    _call("tpspp_attn_train_bwd_ex", d_out, d_out, q, ld_q, k, v, ld_kv, out, lse, N, C, heads, Tq, Tk, valid_len, key_mask,
          int(bool(causal)), float(drop_p), int(seed) & _U64, int(offset) & _U64, dq, ld_dq, dk, dv, ld_dkv)


def attn_dropout_mask(N, heads, Tq, Tk, drop_p, seed, offset, device):
    """`tpspp_attn_dropout_mask`: the (N, heads, Tq, Tk) uint8 keep mask the attention kernels apply for
    (seed, offset, drop_p).  For tests and debugging."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.TpsppError(f"attn_dropout_mask: device is {device}; the HIP path needs a GPU (no CPU fallback)")
    mask = torch.empty((N, heads, Tq, Tk), device=device, dtype=torch.uint8)
    _call("tpspp_attn_dropout_mask", device, N, heads, Tq, Tk, float(drop_p), int(seed) & _U64, int(offset) & _U64, mask)
    return mask


class _AttnTrainFunction(torch.autograd.Function):
    """Attention of `transformer_module.py:24-33` per head.  Saves q, k, v, out and the log-sum-exp; the backward
    recomputes the probabilities and regenerates the dropout mask from (seed, offset)."""

    @staticmethod
    def forward(ctx, q, k, v, valid_len, key_mask, cfg):
        causal, drop_p, seed, offset = cfg
        q, k, v, ld_q, ld_kv = _attn_operands("attn_train_autograd_ex", q, k, v)
        N, Tq, C = q.shape
        Tk, heads = k.shape[1], C // 64
        out, lse = attn_train_fwd_ex(q, ld_q, k, v, ld_kv, N, C, heads, Tq, Tk, valid_len, key_mask, causal, drop_p, seed,
                                     offset)
        ctx.save_for_backward(q, k, v, out, lse, valid_len, key_mask)
        ctx.cfg = (ld_q, ld_kv) + cfg
        return out.view(N, Tq, C)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        q, k, v, out, lse, valid_len, key_mask = ctx.saved_tensors
        if not any(ctx.needs_input_grad[:3]):
            return (None,) * 6
        ld_q, ld_kv, causal, drop_p, seed, offset = ctx.cfg
        N, Tq, C = q.shape
        Tk, heads = k.shape[1], C // 64
        dq = torch.empty((N, Tq, C), device=q.device, dtype=torch.float32)
        dk = torch.empty((N, Tk, C), device=q.device, dtype=torch.float32)
        dv = torch.empty((N, Tk, C), device=q.device, dtype=torch.float32)
        attn_train_bwd_ex(gout.float().contiguous(), q, ld_q, k, v, ld_kv, out, lse, N, C, heads, Tq, Tk, valid_len, key_mask,
                          causal, drop_p, seed, offset, dq, C, dk, dv, C)
        return dq, dk, dv, None, None, None


def attn_train_autograd_ex(q, k, v, valid_len=None, key_mask=None, causal=False, drop_p=0.0, seed=0, offset=0):
    """Differentiable multi-head attention on projected q (N, Tq, C), k, v (N, Tk, C), head h = columns [64h, 64h + 64):
    dropout(softmax(mask(q k^T / 8))) v -> (N, Tq, C) (`tpspp_attn_train_fwd_ex` / `_bwd_ex`).  Key j is visible to query i
    iff j < valid_len[b] (int32, on the device), key_mask[b, j] != 0 ((N, Tk) bool / uint8 on the device) and, with causal,
    j <= i -- whichever are given.  A query with no visible key gives an output row of zeros and no gradient.  The dropout
    keep decision of element (b, h, i, j) is a pure function of (seed, offset, b, h, i, j) (`attn_dropout_mask`
    materialises it).  q may have a row stride of its own and k, v share one: views of one fused (N, T, 3C) projection, or a
    (N, L, C) projection next to the halves of a fused (N, T, 2C) one, are read in place."""
    who = "attn_train_autograd_ex"
    drop_p = _attn_rate(who, drop_p)
    _chk_gpu(f"{who} q", q)
    if q.dim() != 3 or k.dim() != 3:
        raise ValueError(f"{who}: expected (N, T, 64 * heads) operands, got q {tuple(q.shape)}")
    if max(q.shape[1], k.shape[1]) > 256:
        raise ValueError(f"{who}: at most 256 tokens, got Tq = {q.shape[1]}, Tk = {k.shape[1]}")
    valid_len = _attn_valid_len(who, valid_len, q.shape[0], q.device)
    key_mask = _attn_key_mask(who, key_mask, q.shape[0], k.shape[1], q.device)
    return _AttnTrainFunction.apply(q, k, v, valid_len, key_mask, (bool(causal), drop_p, int(seed), int(offset)))


def attn_train_autograd(q, k, v, valid_len=None, drop_p=0.0, seed=0, offset=0):
    """`attn_train_autograd_ex` with the valid_len mask alone: the encoder's attention."""
    return attn_train_autograd_ex(q, k, v, valid_len, None, False, drop_p, seed, offset)


def _unfuse(g, need, C):
    """The gradient `g` of a fused weight or bias (or None), cut back into its projections' row blocks of C: one per entry
    of `need`, None where that projection wants none."""
    return [g[i * C:(i + 1) * C] if g is not None and n else None for i, n in enumerate(need)]


def _attn_block_args(who, x, attn, drop_p):
    x = _chk(f"{who} x", x, 3)
    N, T, C = x.shape
    if C != attn.dim_k or attn.d_k != 64 or attn.d_v != 64:
        raise ValueError(f"{who}: token width {C} against {attn.n_head} heads of {attn.d_k}")
    if T > 256:
        raise ValueError(f"{who}: at most 256 tokens, got {T}")
    biases = (attn.linear_q.bias, attn.linear_k.bias, attn.linear_v.bias)
    if any(b is None for b in biases) and not all(b is None for b in biases):
        raise ValueError(f"{who}: linear_q / _k / _v must all have a bias or none")
    return x, biases, _attn_rate(who, drop_p)


def _attn_proj_bwd(dp, x, nw, nb, mean, rstd, eps, w, need):
    """Tail of an attention block's backward, the projection p = LayerNorm(x) W^T + b of the block's input, from dp (M, O):
    need = (x, nw, nb, w, b) -> the five gradients in that order.  The LayerNorm output is recomputed for dW / db only."""
    O, C = w.shape
    dw = db = None
    if need[3] or need[4]:
        y, _, _ = plane_ln_fwd(x, nw, nb, eps)
        dw, db = linear_bwd_weight(dp, y, _dense(x.numel() // C, C), O, C, need[3], need[4])
        del y
    dx = dnw = dnb = None
    if any(need[:3]):
        dx, dnw, dnb = _ln_bwd(linear_bwd_data(dp, w), x, nw, mean, rstd, need[:3])
    return dx, dnw, dnb, dw, db


class _AttnBlockFunction(torch.autograd.Function):
    """norm1 - q / k / v projections (one product) - attention - fc on x (N, T, C): the attention block of a TFEncoderLayer
    and, with key_mask and causal, the self-attention block of a TFDecoderLayer.  Saves x, the LayerNorm statistics, the
    fused projection, the attention output and its log-sum-exp; the LayerNorm output is recomputed in the backward."""

    @staticmethod
    def forward(ctx, x, n1w, n1b, wq, wk, wv, bq, bk, bv, fcw, fcb, valid_len, cfg, key_mask, causal):
        eps, drop_p, seed, offset = cfg
        N, T, C = x.shape
        M, heads = N * T, C // 64
        y, m1, r1 = plane_ln_fwd(x, n1w, n1b, eps)
        wqkv = torch.cat([wq, wk, wv], dim=0)
        bqkv = None if bq is None else torch.cat([bq, bk, bv])
        qkv = linear_fwd(y, _dense(M, C), wqkv, bqkv)
        out, lse = attn_train_fwd_ex(qkv, 3 * C, qkv[:, C:], qkv[:, 2 * C:], 3 * C, N, C, heads, T, T, valid_len, key_mask,
                                     causal, drop_p, seed, offset)
        a = linear_fwd(out, _dense(M, C), fcw, fcb)
        ctx.cfg = cfg + (causal,)
        ctx.save_for_backward(x, m1, r1, qkv, out, lse, n1w, n1b, wqkv, bqkv, fcw, valid_len, key_mask)
        return a.view(N, T, C)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ga):
        x, m1, r1, qkv, out, lse, n1w, n1b, wqkv, bqkv, fcw, valid_len, key_mask = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:11]):
            return (None,) * 15
        eps, drop_p, seed, offset, causal = ctx.cfg
        N, T, C = x.shape
        M, heads = N * T, C // 64
        res = [None] * 15
        ga = ga.float().contiguous()
        res[9], res[10] = linear_bwd_weight(ga, out, _dense(M, C), C, C, need[9], need[10])
        dout = linear_bwd_data(ga, fcw)
        dqkv = torch.empty((M, 3 * C), device=x.device, dtype=torch.float32)
        attn_train_bwd_ex(dout, qkv, 3 * C, qkv[:, C:], qkv[:, 2 * C:], 3 * C, out, lse, N, C, heads, T, T, valid_len, key_mask,
                          causal, drop_p, seed, offset, dqkv, 3 * C, dqkv[:, C:], dqkv[:, 2 * C:], 3 * C)
        del dout
        *res[:3], dw, db = _attn_proj_bwd(dqkv, x, n1w, n1b, m1, r1, eps, wqkv, (*need[:3], any(need[3:6]), any(need[6:9])))
        res[3:6], res[6:9] = _unfuse(dw, need[3:6], C), _unfuse(db, need[6:9], C)
        return tuple(res)


def attn_block_autograd(x, attn, norm, valid_len=None, drop_p=0.0, seed=0, offset=0, key_mask=None, causal=False):
    """fc(attention(norm(x))) on tokens x (N, T, C), differentiable, on HIP kernels only: of a TFEncoderLayer
    (`transformer_layers.py:57-75` up to the first dropout) and, with the pad mask of the targets as `key_mask` ((N, T) bool
    / uint8, 0 = <PAD>) and `causal`, of a TFDecoderLayer's self-attention (`transformer_layers.py:133-147` up to the
    dropout).  attn: the MultiHeadAttention parameter holder, norm: its LayerNorm."""
    who = "attn_block_autograd"
    x, biases, drop_p = _attn_block_args(who, x, attn, drop_p)
    valid_len = _attn_valid_len(who, valid_len, x.shape[0], x.device)
    key_mask = _attn_key_mask(who, key_mask, x.shape[0], x.shape[1], x.device)
    return _AttnBlockFunction.apply(x, norm.weight, norm.bias, attn.linear_q.weight, attn.linear_k.weight,
                                    attn.linear_v.weight, *biases, attn.fc.weight, attn.fc.bias, valid_len,
                                    (float(norm.eps), drop_p, int(seed), int(offset)), key_mask, bool(causal))


class _FfnBlockFunction(torch.autograd.Function):
    """norm2 - w_1 - GELU - w_2 of a TFEncoderLayer.  Saves x and the LayerNorm statistics; the LayerNorm output and w_1's
    pre-activation are recomputed in the backward (GELU of it inside w_2's weight-gradient staging)."""

    @staticmethod
    def forward(ctx, x, nw, nb, w1, b1, w2, b2, eps):
        f, m, r = _mlp_fwd(x, nw, nb, eps, w1, b1, w2, b2)
        ctx.eps = eps
        ctx.save_for_backward(x, m, r, nw, nb, w1, b1, w2)
        return f

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gf):
        x, m, r, nw, nb, w1, b1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:7]):
            return (None,) * 8
        return (*_mlp_bwd(gf.float().contiguous(), x, nw, nb, m, r, ctx.eps, w1, b1, w2, need[:7]), None)


def ffn_block_autograd(x, mlp, norm):
    """w_2(GELU(w_1(norm(x)))) of a TFEncoderLayer (`transformer_module.py:119-128` up to its dropout) on tokens x
    (N, T, C), differentiable, on HIP kernels only."""
    x = _chk("ffn_block_autograd x", x, 3)
    if mlp.w_1.bias is None or mlp.w_2.bias is None:
        raise ValueError("ffn_block_autograd: w_1 and w_2 carry a bias in every NRTR config")
    return _FfnBlockFunction.apply(x, norm.weight, norm.bias, *_lin(mlp.w_1), *_lin(mlp.w_2), float(norm.eps))


class _TokenLnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        y, m, r = plane_ln_fwd(x, w, b, eps)
        ctx.save_for_backward(x, w, m, r)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w, m, r = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:3]):
            return (None,) * 4
        return (*_ln_bwd(gy.float().contiguous(), x, w, m, r, need[:3]), None)


def token_ln_autograd(x, ln):
    """nn.LayerNorm `ln` over the last dimension of x, differentiable (`tpspp_plane_ln_fwd` / `_bwd`)."""
    x = _chk("token_ln_autograd x", x)
    return _TokenLnFunction.apply(x, ln.weight, ln.bias, float(ln.eps))


def encoder_layer_autograd(x, lyr, valid_len=None, drop_p=0.0, seed=0, offset=0):
    """One pre-norm TFEncoderLayer (`transformer_layers.py:57-75`) on tokens x (N, T, C) in the training graph: every
    matrix product, softmax, LayerNorm and GELU on HIP kernels; the residual additions and the two element-wise dropouts
    (after fc and after w_2, rate drop_p, PyTorch's generator) are PyTorch element-wise ops.  drop_p also drives the
    dropout on the attention probabilities, seeded by (seed, offset)."""
    a = attn_block_autograd(x, lyr.attn, lyr.norm1, valid_len, drop_p, seed, offset)
    x = x + Fn.dropout(a, drop_p, drop_p > 0)
    f = ffn_block_autograd(x, lyr.mlp, lyr.norm2)
    return x + Fn.dropout(f, drop_p, drop_p > 0)


# ---- the decoder's training graph and the loss on HIP kernels ---------------------------------------------------------------
# include/tpspp_train_dec.h: the attention above with its per-key mask, its causal mask and separate row strides for q and
# k / v (the decoder's self- and cross-attention), the target embedding and the sequence cross-entropy.  A decoder layer is
# three once-differentiable functions (norm1 - qkv - causal attention - fc, norm2 - q / fused k|v - attention - fc, norm3 -
# w_1 - GELU - w_2); residual additions and element-wise dropouts stay PyTorch ops as in the encoder.

class _CrossAttnBlockFunction(torch.autograd.Function):
    """norm2 - q projection on x (N, L, C); one fused k | v projection (N*T, 2C) on the encoder output; attention with
    ld_q = C, ld_kv = 2C; fc.  Saves x, out_enc, the LayerNorm statistics, both projections, the attention output and its
    log-sum-exp; the LayerNorm output is recomputed in the backward."""

    @staticmethod
    def forward(ctx, x, enc, nw, nb, wq, wk, wv, bq, bk, bv, fcw, fcb, valid_len, cfg):
        eps, drop_p, seed, offset = cfg
        N, L, C = x.shape
        T, heads = enc.shape[1], C // 64
        y, m, r = plane_ln_fwd(x, nw, nb, eps)
        qp = linear_fwd(y, _dense(N * L, C), wq, bq)
        wkv = torch.cat([wk, wv], dim=0)
        bkv = None if bk is None else torch.cat([bk, bv])
        kv = linear_fwd(enc, _dense(N * T, C), wkv, bkv)
        out, lse = attn_train_fwd_ex(qp, C, kv, kv[:, C:], 2 * C, N, C, heads, L, T, valid_len, None, False, drop_p, seed,
                                     offset)
        a = linear_fwd(out, _dense(N * L, C), fcw, fcb)
        ctx.cfg = cfg
        ctx.save_for_backward(x, enc, m, r, qp, kv, out, lse, nw, nb, wq, bq, wkv, fcw, valid_len)
        return a.view(N, L, C)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ga):
        x, enc, m, r, qp, kv, out, lse, nw, nb, wq, bq, wkv, fcw, valid_len = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:12]):
            return (None,) * 14
        eps, drop_p, seed, offset = ctx.cfg
        N, L, C = x.shape
        T, heads = enc.shape[1], C // 64
        M, MT = N * L, N * T
        res = [None] * 14
        ga = ga.float().contiguous()
        res[10], res[11] = linear_bwd_weight(ga, out, _dense(M, C), C, C, need[10], need[11])
        dout = linear_bwd_data(ga, fcw)
        dqp = torch.empty((M, C), device=x.device, dtype=torch.float32)
        dkv = torch.empty((MT, 2 * C), device=x.device, dtype=torch.float32)
        attn_train_bwd_ex(dout, qp, C, kv, kv[:, C:], 2 * C, out, lse, N, C, heads, L, T, valid_len, None, False, drop_p, seed,
                          offset, dqp, C, dkv, dkv[:, C:], 2 * C)
        del dout
        if any(need[5:7]) or any(need[8:10]):
            dw, db = linear_bwd_weight(dkv, enc, _dense(MT, C), 2 * C, C, any(need[5:7]), any(need[8:10]))
            res[5:7], res[8:10] = _unfuse(dw, need[5:7], C), _unfuse(db, need[8:10], C)
        res[0], res[2], res[3], res[4], res[7] = _attn_proj_bwd(dqp, x, nw, nb, m, r, eps, wq,
                                                                (need[0], need[2], need[3], need[4], need[7]))
        if need[1]:
            res[1] = linear_bwd_data(dkv, wkv).view(enc.shape)
        return tuple(res)


def cross_attn_block_autograd(x, out_enc, attn, norm, valid_len=None, drop_p=0.0, seed=0, offset=0):
    """fc(attention(norm(x), out_enc)) of a TFDecoderLayer's encoder-decoder attention (`transformer_layers.py:149-156` up
    to the dropout): queries from the decoder tokens x (N, L, C), keys and values from the encoder output (N, T, C) through
    ONE (N*T, 2C) product, keys j >= valid_len[b] masked.  Differentiable in x, out_enc and every parameter."""
    who = "cross_attn_block_autograd"
    x, biases, drop_p = _attn_block_args(who, x, attn, drop_p)
    out_enc = _chk(f"{who} out_enc", out_enc, 3)
    if out_enc.shape[0] != x.shape[0] or out_enc.shape[2] != x.shape[2]:
        raise ValueError(f"{who}: x {tuple(x.shape)} against out_enc {tuple(out_enc.shape)}")
    if out_enc.shape[1] > 256:
        raise ValueError(f"{who}: at most 256 encoder tokens, got {out_enc.shape[1]}")
    valid_len = _attn_valid_len(who, valid_len, x.shape[0], x.device)
    return _CrossAttnBlockFunction.apply(x, out_enc, norm.weight, norm.bias, attn.linear_q.weight, attn.linear_k.weight,
                                         attn.linear_v.weight, *biases, attn.fc.weight, attn.fc.bias, valid_len,
                                         (float(norm.eps), drop_p, int(seed), int(offset)))


def _embed_tokens(who, tokens, num_classes, dev):
    """(N, L) integer tokens -> int32 on `dev`.  Tokens that live on the host -- where the targets originate -- are
    refused when they lie outside [0, num_classes); tokens already on the device are taken as they are (the kernels
    ignore such a token)."""
    if not isinstance(tokens, torch.Tensor) or tokens.dim() != 2 or tokens.is_floating_point():
        raise ValueError(f"{who}: tokens must be an (N, L) integer tensor")
    if tokens.device.type == "cpu" and tokens.numel():
        lo, hi = int(tokens.min()), int(tokens.max())
        if lo < 0 or hi >= num_classes:
            raise ValueError(f"{who}: tokens must lie in [0, {num_classes}), got [{lo}, {hi}]")
    return tokens.to(device=dev, dtype=torch.int32).contiguous()


def embed_pos_fwd(tok, weight, pos):
    """`tpspp_embed_pos_fwd`: weight[tok] + pos[:L] -> (N, L, C); tok (N, L) int32 on the device."""
    N, L = tok.shape
    out = torch.empty((N, L, weight.shape[1]), device=weight.device, dtype=torch.float32)
    _call("tpspp_embed_pos_fwd", weight, tok, weight, pos, N, L, weight.shape[1], weight.shape[0], out)
    return out


def embed_bwd_workspace_floats(M, num_classes, C):
    return _query("tpspp_embed_bwd_workspace_floats", M, num_classes, C)


def embed_bwd(dx, tok, num_classes, padding_idx):
    """`tpspp_embed_bwd`: d_weight (num_classes, C) from dx (M, C) dense and tok (M) int32, every row written."""
    M, C = tok.numel(), dx.shape[-1]
    if M == 0:
        return torch.zeros((num_classes, C), device=dx.device, dtype=torch.float32)
    dw = torch.empty((num_classes, C), device=dx.device, dtype=torch.float32)
    ws, n = _ws_n(embed_bwd_workspace_floats(M, num_classes, C), dx.device)
    _call("tpspp_embed_bwd", dx, dx, tok, M, C, num_classes, -1 if padding_idx is None else padding_idx, dw, ws, n)
    return dw


class _EmbedPosFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, tok, pos, padding_idx):
        ctx.save_for_backward(tok)
        ctx.cfg = (weight.shape[0], padding_idx)
        return embed_pos_fwd(tok, weight, pos)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gx):
        if not ctx.needs_input_grad[0]:
            return (None,) * 4
        (tok,) = ctx.saved_tensors
        return embed_bwd(gx.float().contiguous(), tok, *ctx.cfg), None, None, None


def embed_pos_autograd(tokens, emb_weight, pos_table, padding_idx=None):
    """nn.Embedding(tokens) + the first L rows of the position table (`nrtr_decoder.py:95-99` before the dropout) ->
    (N, L, C), differentiable in emb_weight (`tpspp_embed_pos_fwd` / `tpspp_embed_bwd`: the row of padding_idx gets a zero
    gradient, in a fixed summation order)."""
    who = "embed_pos_autograd"
    emb_weight = _chk(f"{who} emb_weight", emb_weight, 2)
    tok = _embed_tokens(who, tokens, emb_weight.shape[0], emb_weight.device)
    pos = _chk(f"{who} pos_table", pos_table.detach())
    pos = pos.reshape(-1, pos.shape[-1])
    if pos.shape[1] != emb_weight.shape[1] or pos.shape[0] < tok.shape[1] or pos.device != emb_weight.device:
        raise ValueError(f"{who}: position table {tuple(pos.shape)} against {tok.shape[1]} tokens of width "
                         f"{emb_weight.shape[1]}")
    return _EmbedPosFunction.apply(emb_weight, tok, pos, padding_idx)


_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def _ce_operands(who, logits, targets, shift):
    """logits (N, L, K) float32 on the device with any strides, targets (N, L) integers -> int32 on that device."""
    _chk_gpu(f"{who} logits", logits)
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise TypeError(f"{who}: logits must be (N, L, K) float32, got {tuple(logits.shape)} {logits.dtype}")
    N, L, K = logits.shape
    if not 1 <= K <= 1024:
        raise ValueError(f"{who}: 1 to 1024 classes, got {K}")
    if not isinstance(targets, torch.Tensor) or targets.is_floating_point() or tuple(targets.shape) != (N, L):
        raise ValueError(f"{who}: targets must be ({N}, {L}) integers")
    if L - int(bool(shift)) < 0 or L == 0:
        raise ValueError(f"{who}: no position to score")
    return targets.to(device=logits.device, dtype=torch.int32).contiguous()


def seq_ce_fwd(logits, tgt, shift, ignore_index, reduction):
    """`tpspp_seq_ce_fwd`: (loss (N, Lp), lse (N, Lp), reduced (1) | None, count (1) | None), Lp = L - shift."""
    N, L, K = logits.shape
    Lp = L - int(shift)
    dev = logits.device
    loss = torch.empty((N, Lp), device=dev, dtype=torch.float32)
    lse = torch.empty((N, Lp), device=dev, dtype=torch.float32)
    red = cnt = None
    if reduction:
        red = torch.empty((1,), device=dev, dtype=torch.float32)
        cnt = torch.empty((1,), device=dev, dtype=torch.float32)
    if N == 0 and reduction:                   # the library returns before any launch
        red.fill_(float("nan") if reduction == 1 else 0.0)
        cnt.zero_()
    _call("tpspp_seq_ce_fwd", logits, logits, logits.stride(0), logits.stride(1), logits.stride(2), tgt, N, L, K,
          int(shift), int(ignore_index), reduction, loss, lse, red, cnt)
    return loss, lse, red, cnt


def seq_ce_bwd(g, logits, tgt, lse, cnt, shift, ignore_index, reduction):
    """`tpspp_seq_ce_bwd`: d_logits (N, L, K) dense."""
    N, L, K = logits.shape
    d = torch.empty((N, L, K), device=logits.device, dtype=torch.float32)
    _call("tpspp_seq_ce_bwd", logits, g, logits, logits.stride(0), logits.stride(1), logits.stride(2), tgt, lse, cnt, N, L,
          K, int(shift), int(ignore_index), reduction, d)
    return d


class _SeqCeFunction(torch.autograd.Function):
    """Saves the logits, the targets, the per-position log-sum-exp and the count; the softmax is recomputed."""

    @staticmethod
    def forward(ctx, logits, tgt, cfg):
        shift, ignore_index, reduction, flatten = cfg
        loss, lse, red, cnt = seq_ce_fwd(logits, tgt, shift, ignore_index, reduction)
        ctx.save_for_backward(logits, tgt, lse, cnt)
        ctx.cfg = cfg
        if reduction:
            return red.view(())
        return loss.view(-1) if flatten else loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        logits, tgt, lse, cnt = ctx.saved_tensors
        shift, ignore_index, reduction, _ = ctx.cfg
        if logits.shape[0] == 0:
            return torch.zeros_like(logits), None, None
        return seq_ce_bwd(g.float().contiguous(), logits, tgt, lse, cnt, shift, ignore_index, reduction), None, None


def seq_cross_entropy_autograd(logits, targets, ignore_index=-100, reduction="none", shift=False, flatten=True):
    """`losses.sequence_cross_entropy` on HIP kernels (`tpspp_seq_ce_fwd` / `_bwd`), with its result shapes: a scalar for
    "mean" / "sum", (N * L',) for "none" with flatten, else (N, L'), L' = L - shift.  The logits are read through their
    strides (no copy for a view such as logits[:, :-1]); targets on the host or on the device, any integer type."""
    who = "seq_cross_entropy_autograd"
    if reduction not in _REDUCTIONS:
        raise ValueError(f'{who}: reduction must be "none", "mean" or "sum", got {reduction!r}')
    tgt = _ce_operands(who, logits, targets, shift)
    return _SeqCeFunction.apply(logits, tgt, (bool(shift), int(ignore_index), _REDUCTIONS[reduction], bool(flatten)))


class _LinearFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return linear_fwd(x, _dense(x.numel() // w.shape[1], w.shape[1]), w, b).view(*x.shape[:-1], w.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        O, K = w.shape
        M = x.numel() // K
        gy = gy.float().contiguous().view(M, O)
        dw, db = linear_bwd_weight(gy, x, _dense(M, K), O, K, need[1], need[2])
        dx = linear_bwd_data(gy, w).view(x.shape) if need[0] else None
        return dx, dw, db


def linear_autograd(x, lin):
    """nn.Linear `lin` on the last dimension of x, differentiable (`tpspp_mm_f32` / `tpspp_linear_bwd_weight`)."""
    x = _chk("linear_autograd x", x)
    if x.shape[-1] != lin.weight.shape[1]:
        raise ValueError(f"linear_autograd: input width {x.shape[-1]} against weight {tuple(lin.weight.shape)}")
    return _LinearFunction.apply(x, lin.weight, lin.bias)


def decoder_layer_autograd(x, out_enc, lyr, key_mask=None, valid_len=None, drop_p=0.0, seed=0, offset=0):
    """One pre-norm TFDecoderLayer (`transformer_layers.py:133-163`) on tokens x (N, L, C) and the encoder output
    (N, T, C) in the training graph: causal self-attention under the targets' pad mask `key_mask`, attention over the
    encoder tokens below valid_len, feed-forward -- every matrix product, softmax, LayerNorm and GELU on HIP kernels; the
    three residual additions and the three element-wise dropouts (rate drop_p, PyTorch's generator) are PyTorch ops.
    `offset` is the layer's index: the dropout on the attention probabilities uses (seed, 2 * offset) in the
    self-attention and (seed, 2 * offset + 1) in the cross-attention."""
    a = attn_block_autograd(x, lyr.self_attn, lyr.norm1, None, drop_p, seed, 2 * offset, key_mask=key_mask, causal=True)
    x = x + Fn.dropout(a, drop_p, drop_p > 0)
    a = cross_attn_block_autograd(x, out_enc, lyr.enc_attn, lyr.norm2, valid_len, drop_p, seed, 2 * offset + 1)
    x = x + Fn.dropout(a, drop_p, drop_p > 0)
    f = ffn_block_autograd(x, lyr.mlp, lyr.norm3)
    return x + Fn.dropout(f, drop_p, drop_p > 0)


# ---- the CRNN recogniser (include/tpspp_crnn.h, tpspp_crnn.hip) ---------------------------------------------------
def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def crnn_maxpool(x, kernel=(2, 2), stride=(2, 2), padding=(0, 0)):
    """nn.MaxPool2d(kernel, stride, padding) with rectangular stride / padding (`tpspp_crnn_maxpool_fwd`;
    very_deep_vgg.py:51-60): padding counts as -inf, a NaN in a window gives NaN."""
    x = _chk("crnn_maxpool input", x, 4)
    (kh, kw), (sh, sw), (ph, pw) = _pair(kernel), _pair(stride), _pair(padding)
    N, C, H, W = x.shape
    if min(kh, kw, sh, sw) < 1 or H + 2 * ph < kh or W + 2 * pw < kw:
        raise ValueError(f"crnn_maxpool: kernel {(kh, kw)} / stride {(sh, sw)} / padding {(ph, pw)} on a {H} x {W} map")
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    out = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
    _call("tpspp_crnn_maxpool_fwd", x, x, N, C, H, W, kh, kw, sh, sw, ph, pw, out, Ho, Wo)
    return out


# ---- VeryDeepVgg's training graph (tpspp_crnn_pool_train.hip; VeryDeepVgg.set_vgg_train_backend("hip")) ------------------
def crnn_maxpool_bwd(dp, y, kernel=(2, 2), stride=(2, 2), padding=(0, 0), relu_mask=True):
    """Backward of `crnn_maxpool(y, kernel, stride, padding)` (`tpspp_crnn_maxpool_bwd`): dp (N, C, Ho, Wo) -> dy like y.
    No index map: every window of y is scanned again with the forward's rule, and an element gathers dp over the windows
    that selected it (no atomics, bitwise reproducible).  relu_mask: the backward of the in-place ReLU that produced y in
    the same pass -- an element with not (y > 0) receives +0."""
    who = "crnn_maxpool_bwd"
    y = _chk(f"{who} y", y, 4)
    (kh, kw), (sh, sw), (ph, pw) = _pair(kernel), _pair(stride), _pair(padding)
    N, C, H, W = y.shape
    if min(kh, kw, sh, sw) < 1 or H + 2 * ph < kh or W + 2 * pw < kw:
        raise ValueError(f"{who}: kernel {(kh, kw)} / stride {(sh, sw)} / padding {(ph, pw)} on a {H} x {W} map")
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    dp = _chk(f"{who} dp", dp, 4)
    if tuple(dp.shape) != (N, C, Ho, Wo) or dp.device != y.device:
        raise ValueError(f"{who}: dp must be {(N, C, Ho, Wo)} on {y.device}, got {tuple(dp.shape)} on {dp.device}")
    dy = torch.empty_like(y)
    if N == 0:          # an empty batch has no device pointer to hand over
        return dy
    _call("tpspp_crnn_maxpool_bwd", y, dp, y, int(bool(relu_mask)), N, C, H, W, kh, kw, sh, sw, ph, pw, dy, Ho, Wo)
    return dy


class _ConvReluPoolFunction(torch.autograd.Function):
    """p = maxpool(relu(conv(x) + bias)): HIP forward (`conv2d`, `crnn_maxpool`) and backward (`crnn_maxpool_bwd` with the
    ReLU mask, then `conv2d_bwd_weight` / `conv2d_bwd_data` with relu=False, which do not read y).  Saves x, the weight and
    y; no index map (the backward rescans y)."""

    @staticmethod
    def forward(ctx, x, w, cb, cfg):
        cw, (k, st), pool = cfg
        x = x.float().contiguous()
        y = conv2d([x], cw, st, relu=True)
        p = crnn_maxpool(y, *pool)
        ctx.cfg = (k, st, pool, cb is not None)
        ctx.save_for_backward(x, w, y)
        return p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gp):
        k, st, pool, has_bias = ctx.cfg
        x, w, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_w, want_b = need[1], has_bias and need[2]
        dx = dw = dcb = None
        if need[0] or want_w or want_b:
            dy = crnn_maxpool_bwd(gp.float().contiguous(), y, *pool, relu_mask=True)
            if want_w or want_b:
                dw, dcb = conv2d_bwd_weight([x], dy, k, st, relu=False, want_weight=want_w, want_bias=want_b)
            if need[0]:
                dx = conv2d_bwd_data(dy, w, [x], st, relu=False)[0]
        return dx, dw, dcb, None


def conv_relu_pool_autograd(x, conv, kernel=(2, 2), stride=(2, 2), padding=(0, 0), cw=None, name="pooled layer"):
    """maxpool(relu(conv(x))) -- conv0, conv1, conv3 and conv5 of VeryDeepVgg with the nn.MaxPool2d(kernel, stride, padding)
    behind them -- inside an autograd graph on the HIP kernels.  conv: nn.Conv2d (3x3 'same', bias allowed); cw: the
    forward's ConvWeight (a cache the caller keys on the parameters' versions), built on the device here if None.  The
    backward honours `needs_input_grad`: nothing is launched for a frozen layer whose input needs no gradient."""
    _chk_gpu(name, x)
    kst = _conv_spec(conv, f"{name} conv", bias_ok=True)
    pool = (_pair(kernel), _pair(stride), _pair(padding))
    if cw is None:
        cw = prep_conv_weight_device(conv.weight, conv.bias)
    return _ConvReluPoolFunction.apply(x, conv.weight, conv.bias, (cw, kst, pool))


def conv6_extend(conv):
    """(ConvWeight, w3) of VeryDeepVgg's conv6 for the HIP kernels: the 2x2 valid convolution as the 3x3 kernel w3 whose
    first row and first column are zero (`VeryDeepVgg._hip_weights`), prepared on the device without BatchNorm folded."""
    w3 = Fn.pad(conv.weight.detach().float(), (1, 0, 1, 0)).contiguous()
    return prep_conv_weight_device(w3, conv.bias), w3


class _Conv6BnFunction(torch.autograd.Function):
    """y = relu(bn(conv6(x) + bias)) of a (N, C, 2, W) map -> (N, Cout, 1, W - 1).  The zero-extended 3x3 kernel at stride
    (2, 1) gives a W-wide map whose last column reads the right padding: it is dropped BEFORE the batch statistics (a
    contiguous copy of the small map), and receives a zero gradient on the way back.  Otherwise `_BnStemFunction`."""

    @staticmethod
    def forward(ctx, x, w, cb, g, b, cfg):
        (cw, w3), spec = cfg
        x = x.float().contiguous()
        z = conv2d([x], cw, (2, 1), relu=False)[:, :, :, :x.shape[3] - 1].contiguous()
        mean, rstd = _bn_stats_of(z, spec)
        y = bn_apply(z, (mean, rstd), g, b, relu=True)
        ctx.cfg = (spec[0], cb is not None)
        ctx.save_for_backward(x, w3, g, z, y, mean, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        train, has_bias = ctx.cfg
        x, w3, g, z, y, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        gy = gy.float().contiguous()
        need_z = need[0] or need[1] or (has_bias and need[2])
        dx = dw = dcb = dg = db = None
        sums = (None, None, None)
        if train or need[3] or need[4]:
            sums = bn_bwd_reduce(gy, y, z, (mean, rstd), relu=True)
            dg = sums[1] if need[3] else None
            db = sums[0] if need[4] else None
        if need_z:
            dz, _ = bn_bwd_data(gy, y, z, (mean, rstd), g, sums, train, relu=True)
            dz = Fn.pad(dz, (0, 1))                                # the dropped column: a zero gradient
            if need[1] or (has_bias and need[2]):
                dw, dcb = conv2d_bwd_weight([x], dz, 3, (2, 1), relu=False, want_weight=need[1], want_bias=has_bias and need[2])
                if dw is not None:
                    dw = dw[:, :, 1:, 1:].contiguous()             # the four real taps
            if need[0]:
                dx = conv2d_bwd_data(dz, w3, [x], (2, 1), relu=False)[0]
        return dx, dw, dcb, dg, db, None


def conv6_bn_autograd(x, conv, bn, prepared6=None, name="conv6"):
    """relu(bn(conv(x))) for VeryDeepVgg's conv6 -- nn.Conv2d(C, Cout, 2, 1, 0) on a two-row map -- inside an autograd
    graph on the HIP kernels; (N, C, 2, W) -> (N, Cout, 1, W - 1).  bn follows its own mode as in `bn_stem_autograd`
    (.training: batch statistics over the (N, Cout, 1, W - 1) map, running statistics and num_batches_tracked updated on
    the device).  prepared6: `conv6_extend(conv)` (a cache the caller keys on the parameters' versions)."""
    _chk_gpu(name, x)
    if not isinstance(conv, torch.nn.Conv2d) or (tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding),
                                                   tuple(conv.dilation), conv.groups) != ((2, 2), (1, 1), (0, 0), (1, 1), 1):
        raise ValueError(f"{name}: expected nn.Conv2d(C, Cout, 2, 1, 0) without dilation or groups")
    if x.dim() != 4 or x.shape[2] != 2 or x.shape[3] < 2:
        raise ValueError(f"{name}: the HIP path needs an image height of 32 (a two-row map before conv6) and at least two "
                         f"columns, got {tuple(x.shape)}")
    spec = _bn_spec(bn, f"{name} bn")
    if prepared6 is None:
        prepared6 = conv6_extend(conv)
    return _Conv6BnFunction.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, (prepared6, spec))


def crnn_maxpool_blocked(x, kernel=(2, 2), stride=(2, 2), padding=(0, 0)):
    """`crnn_maxpool` on a `Blocked` (bf16) or `Blocked32` (fp32) map -> the same class (`tpspp_crnn_maxpool_blk_fwd`,
    include/tpspp_crnn_bf16.h): the bits `F.max_pool2d` gives on the NCHW view."""
    if not isinstance(x, Blocked):
        raise TypeError("crnn_maxpool_blocked: expected a Blocked or Blocked32 map")
    _chk_gpu("crnn_maxpool_blocked input", x.t)
    (kh, kw), (sh, sw), (ph, pw) = _pair(kernel), _pair(stride), _pair(padding)
    N, C, H, W = x.shape
    if min(kh, kw, sh, sw) < 1 or H + 2 * ph < kh or W + 2 * pw < kw:
        raise ValueError(f"crnn_maxpool_blocked: kernel {(kh, kw)} / stride {(sh, sw)} / padding {(ph, pw)} on a {H} x {W} map")
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    out = type(x)(torch.empty((N, C // 8, Ho, Wo, 8), device=x.device, dtype=x.dtype))
    if N == 0:          # an empty batch has no device pointer to hand over
        return out
    _call("tpspp_crnn_maxpool_blk_fwd", x.t, x.t, _layout_code(x), N, C, H, W, kh, kw, sh, sw, ph, pw, out.t, Ho, Wo)
    return out


CRNN_HIDDEN = 256
CRNN_LSTM_GROUPS = (4, 8, 16)          # the accepted non-zero images_per_group of tpspp_crnn_lstm_fwd


def crnn_lstm_plan(N, images_per_group=0, compute_units=0):
    """`tpspp_crnn_lstm_plan`: the images per workgroup `crnn_lstm` uses (host only; compute_units 0: the current device's)."""
    g = _query("tpspp_crnn_lstm_plan", N, images_per_group, compute_units)
    _lib.check(min(g, 0), "tpspp_crnn_lstm_plan")
    return g


def _lstm_operand(who, name, t, shape_tail, T=None, N=None):
    t = _chk(f"{who} {name}", t, 2 + len(shape_tail))
    if tuple(t.shape[2:]) != tuple(shape_tail) or (T is not None and tuple(t.shape[:2]) != (T, N)):
        raise ValueError(f"{who}: {name} must be (T, N, {', '.join(map(str, shape_tail))}), got {tuple(t.shape)}")
    return t


def _chk_arranged(who, mw, lead, rows, k, device):
    if not isinstance(mw, MfmaWeight) or mw.arranged.dim() != 5 + len(lead):
        raise TypeError(f"{who}: the weight must be an MfmaWeight of the {lead + (rows, k)} stack (arrange_mfma16)")
    _chk_gpu(f"{who} weight", mw.arranged)
    if tuple(mw.arranged.shape[:len(lead)]) != lead or (mw.rows, mw.k) != (rows, k) or mw.arranged.device != device:
        raise ValueError(f"{who}: the weight must be {lead + (rows, k)} arranged, on the operands' device, got "
                         f"{tuple(mw.arranged.shape)}")


def _lstm_weight(who, name, w, rows, k, device, bf16):
    """The recurrent weight of both directions, a dense fp32 (2, rows, k) tensor or (bf16) its `MfmaWeight` -> (what the
    entry point reads, the split3 argument that only a bf16 entry point takes)."""
    if bf16:
        _chk_arranged(who, w, (2,), rows, k, device)
        return w.arranged, (int(w.x3),)
    w = _chk(f"{who} {name}", w, 3)
    if tuple(w.shape) != (2, rows, k) or w.device != device:
        raise ValueError(f"{who}: {name} must be (2, {rows}, {k}) on the operands' device, got {tuple(w.shape)}")
    return w, ()


def _lstm_fwd(who, entry, xg, w_hh, images_per_group, bf16, save):
    """The four forward recurrences on their entry points -> out, or (save: a `_train_fwd`) -> (out, gates, cell)."""
    xg = _lstm_operand(who, "xg", xg, (2, 4 * CRNN_HIDDEN))
    w, split3 = _lstm_weight(who, "w_hh", w_hh, 4 * CRNN_HIDDEN, CRNN_HIDDEN, xg.device, bf16)
    T, N = xg.shape[0], xg.shape[1]
    tails = ((2 * CRNN_HIDDEN,), (2, 4 * CRNN_HIDDEN), (2, CRNN_HIDDEN))[:3 if save else 1]
    outs = [torch.empty((T, N) + tail, device=xg.device, dtype=torch.float32) for tail in tails]
    if N > 0:
        _call(entry, xg, xg, w, *outs, T, N, CRNN_HIDDEN, int(images_per_group), *split3)
    return tuple(outs) if save else outs[0]


def _lstm_bwd(who, entry, d_out, gates, cell, w_hh_t, images_per_group, bf16, direction_major=False):
    """The two backwards through time on their entry points -> (d_xg, its direction-major copy | None)."""
    gates = _lstm_operand(who, "gates", gates, (2, 4 * CRNN_HIDDEN))
    T, N = gates.shape[0], gates.shape[1]
    d_out = _lstm_operand(who, "d_out", d_out, (2 * CRNN_HIDDEN,), T, N)
    cell = _lstm_operand(who, "cell", cell, (2, CRNN_HIDDEN), T, N)
    w, split3 = _lstm_weight(who, "w_hh_t", w_hh_t, CRNN_HIDDEN, 4 * CRNN_HIDDEN, gates.device, bf16)
    if len({t.device for t in (d_out, gates, cell)}) != 1:
        raise ValueError(f"{who}: all operands on one device")
    d_xg = torch.empty((T, N, 2, 4 * CRNN_HIDDEN), device=gates.device, dtype=torch.float32)
    d_dir = torch.empty((2, T, N, 4 * CRNN_HIDDEN), device=gates.device, dtype=torch.float32) if direction_major else None
    if N > 0:
        _call(entry, gates, d_out, gates, cell, w, d_xg, *(() if bf16 else (d_dir,)), T, N, CRNN_HIDDEN, int(images_per_group),
              *split3)
    return d_xg, d_dir


def crnn_lstm(xg, w_hh, images_per_group=0):
    """The recurrence of one bidirectional nn.LSTM(., 256) layer with zero initial state (`tpspp_crnn_lstm_fwd`;
    lstm_layer.py:14): xg (T, N, 2, 1024) input pre-activations of both directions, w_hh (2, 1024, 256) -> (T, N, 512)."""
    return _lstm_fwd("crnn_lstm", "tpspp_crnn_lstm_fwd", xg, w_hh, images_per_group, False, False)


class MfmaWeight:
    """A (rows, K) weight -- or a stack (n, rows, K) of them -- arranged for the B operand of v_mfma_f32_16x16x32_bf16
    (`arrange_mfma16`): `arranged` bf16 ([n], [hi | lo], rows / 16, K / 32, 64, 8), fp32 `bias` | None."""

    def __init__(self, arranged, bias, rows, k, x3):
        self.arranged, self.bias, self.rows, self.k, self.x3 = arranged, bias, rows, k, x3


def arrange_mfma16(w, bias=None, x3=False):
    """fp32 (rows, K) or (n, rows, K), rows % 16 == 0 and K % 32 == 0 -> MfmaWeight (include/tpspp.h, tpspp_mm_bf16): per
    matrix [hi | lo][rows / 16][K / 32][lane][8] bf16 with lane l holding W[16 ct + (l & 15)][32 ks + 8 (l >> 4) + j];
    one slab bf16(w), or, x3, the two of `_hi_lo`."""
    w = w.detach().float()
    if w.dim() not in (2, 3) or w.shape[-2] % 16 or w.shape[-1] % 32:
        raise ValueError(f"arrange_mfma16: (rows, K) or (n, rows, K) with rows % 16 == 0 and K % 32 == 0, got {tuple(w.shape)}")
    rows, K = w.shape[-2:]
    st = torch.stack(_hi_lo(w) if x3 else (w.to(torch.bfloat16),), dim=-3)          # (..., s, rows, K)
    st = st.reshape(st.shape[:-2] + (rows // 16, 16, K // 32, 4, 8))                # (..., s, ct, col, ks, quad, j)
    nd = st.dim()
    st = st.permute(*range(nd - 5), nd - 5, nd - 3, nd - 2, nd - 4, nd - 1)         # (..., s, ct, ks, quad, col, j)
    arranged = st.reshape(st.shape[:-3] + (64, 8)).contiguous()
    return MfmaWeight(arranged, None if bias is None else bias.detach().float().contiguous(), rows, K, bool(x3))


def dearrange_mfma16(mw):
    """The inverse of `arrange_mfma16`: the bf16 slabs as ([n], [hi | lo], rows, K) (what the tests compare with `_hi_lo`)."""
    a = mw.arranged
    lead = a.shape[:-4]
    a = a.reshape(lead + (mw.rows // 16, mw.k // 32, 4, 16, 8))                     # (..., ct, ks, quad, col, j)
    nd = a.dim()
    a = a.permute(*range(nd - 5), nd - 5, nd - 2, nd - 4, nd - 3, nd - 1)           # (..., ct, col, ks, quad, j)
    return a.reshape(lead + (mw.rows, mw.k))


def mm_bf16(A, a_strides, mw, C, c_strides, batch, M):
    """`tpspp_mm_bf16`: C[b][i][j] = sum_k A[b][i][k] W[j][k] + bias[j] on the bf16 matrix cores, A rounded to bf16 or
    (mw.x3) split as it is staged; strides in elements, (batch, row, k) for A and (batch, row, column) for C."""
    for name, t in (("mm_bf16 A", A), ("mm_bf16 C", C)):        # (strided views: taken as they are, never copied)
        _chk_gpu(name, t)
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if not isinstance(mw, MfmaWeight) or mw.arranged.dim() != 5:
        raise TypeError("mm_bf16: the weight must be an MfmaWeight of one (rows, K) matrix (arrange_mfma16)")
    _chk_gpu("mm_bf16 weight", mw.arranged)
    if mw.arranged.device != C.device or A.device != C.device or (mw.bias is not None and mw.bias.device != C.device):
        raise ValueError("mm_bf16: operands on different devices")
    if batch * M == 0:
        return C
    sa, sc = _i64(*a_strides), _i64(*c_strides)
    _call("tpspp_mm_bf16", C, batch, M, mw.rows, mw.k, A, _vp(sa), mw.arranged, C, _vp(sc), mw.bias, int(mw.x3))
    return C


def linear_bf16_fwd(x, desc, mw):
    """`linear_fwd` on `tpspp_mm_bf16`: y (rows, O) dense fp32 = x W^T + b for the token operand x described by `desc`."""
    nb, Mi, sb, si, sk = desc
    y = torch.empty((nb * Mi, mw.rows), device=mw.arranged.device, dtype=torch.float32)
    return mm_bf16(x, (sb, si, sk), mw, y, (Mi * mw.rows, mw.rows, 1), nb, Mi)


def crnn_lstm_bf16(xg, mw, images_per_group=0):
    """`crnn_lstm` with the recurrent product on the bf16 matrix cores (`tpspp_crnn_lstm_bf16_fwd`): xg (T, N, 2, 1024)
    fp32, mw = `arrange_mfma16(w_hh (2, 1024, 256), x3=...)` -> (T, N, 512) fp32; h is rounded (x3: split) per step."""
    return _lstm_fwd("crnn_lstm_bf16", "tpspp_crnn_lstm_bf16_fwd", xg, mw, images_per_group, True, False)


def crnn_ctc_decode_device(logits, decode_len, blank=0):
    """`tpspp_crnn_ctc_decode` into fresh device tensors: (idx (N, T) int32, -1 where the scan of ctc.py:119-129 drops the
    position; score (N, T) float32, 0 there).  decode_len: (N) int32 on the logits' device."""
    logits = _chk("crnn_ctc_decode logits", logits, 3)
    N, T, C = logits.shape
    decode_len = _chk("crnn_ctc_decode decode_len", decode_len, 1, (torch.int32,))
    if decode_len.shape[0] != N or decode_len.device != logits.device:
        raise ValueError("crnn_ctc_decode: decode_len must be (N) on the logits' device")
    idx = torch.empty((N, T), device=logits.device, dtype=torch.int32)
    score = torch.empty((N, T), device=logits.device, dtype=torch.float32)
    if N == 0:
        return idx, score
    _call("tpspp_crnn_ctc_decode", logits, logits, decode_len, N, T, C, int(blank), idx, score)
    return idx, score


def crnn_ctc_decode(logits, decode_len, blank=0):
    """`tpspp_crnn_ctc_decode` + ONE device->host copy (as `attn_tensor2idx`): (idx (N, T) int32 numpy, score (N, T)
    float32 numpy).  decode_len: a sequence of N ints (host); it travels in the same buffer as the outputs."""
    logits = _chk("crnn_ctc_decode logits", logits, 3)
    N, T, C = logits.shape
    if len(decode_len) != N:
        raise ValueError("crnn_ctc_decode: one decode_len per image")
    # [idx (N*T) | score (N*T) as raw bits | decode_len (N)]: one int32 buffer, one copy back
    buf = torch.empty((2 * N * T + N,), device=logits.device, dtype=torch.int32)
    if N == 0:
        z = buf.cpu().numpy()
        return z.reshape(0, T), z.view("float32").reshape(0, T)
    buf[2 * N * T:].copy_(torch.tensor([int(v) for v in decode_len], dtype=torch.int32))
    _call("tpspp_crnn_ctc_decode", logits, logits, buf.data_ptr() + 8 * N * T, N, T, C, int(blank), buf.data_ptr(),
          buf.data_ptr() + 4 * N * T)
    host = buf[:2 * N * T].cpu().numpy()
    return host[:N * T].reshape(N, T), host[N * T:].view("float32").reshape(N, T)


# ---- training of the CRNN decoder and the CTC loss (include/tpspp_crnn_train.h, tpspp_crnn_train.hip) --------------
def crnn_lstm_train_fwd(xg, w_hh, images_per_group=0):
    """`tpspp_crnn_lstm_train_fwd`: `crnn_lstm` (the same bits) that keeps what `crnn_lstm_bwd` reads ->
    (out (T, N, 512), gates (T, N, 2, 1024) after their activations, cell (T, N, 2, 256))."""
    return _lstm_fwd("crnn_lstm_train_fwd", "tpspp_crnn_lstm_train_fwd", xg, w_hh, images_per_group, False, True)


def crnn_lstm_bwd(d_out, gates, cell, w_hh_t, images_per_group=0, direction_major=False):
    """`tpspp_crnn_lstm_bwd`: the backward through time.  d_out (T, N, 512), gates and cell of `crnn_lstm_train_fwd`, w_hh_t
    (2, 256, 1024) the per-direction transpose of w_hh -> d_xg (T, N, 2, 1024), the gradient of the pre-activations; with
    `direction_major` -> (d_xg, its copy as (2, T, N, 1024): what `crnn_lstm_bwd_w_hh` reads)."""
    d_xg, d_dir = _lstm_bwd("crnn_lstm_bwd", "tpspp_crnn_lstm_bwd", d_out, gates, cell, w_hh_t, images_per_group, False,
                            direction_major)
    return (d_xg, d_dir) if direction_major else d_xg


def crnn_lstm_bwd_w_hh(d_xg_dir, out):
    """d w_hh (2, 1024, 256) = sum_t da_t[d]^T h_{t -+ 1}[d] on `tpspp_linear_bwd_weight` (fixed split-K, bitwise
    reproducible): dy is the direction-major d_xg_dir (2, T, N, 1024) of `crnn_lstm_bwd`, shifted by one step -- dense rows
    --, x the shifted view of out (T, N, 512) read through its row stride.  The step whose previous h is h_0 = 0 drops
    out, so T = 1 gives zeros.  (tpspp_mm_f32 over shifted views of the (T, N, 2, 1024) d_xg needs no copy but reads its k
    operand at a stride of 2048 floats: scripts/bench_crnn_train.py measures both.)"""
    T, N = d_xg_dir.shape[1], d_xg_dir.shape[2]
    H, G = CRNN_HIDDEN, 4 * CRNN_HIDDEN
    if T < 2 or N == 0:
        return torch.empty((2, G, H), device=d_xg_dir.device, dtype=torch.float32).zero_()
    M = (T - 1) * N
    pairs = ((d_xg_dir[0, 1:], out[:-1, :, :H]), (d_xg_dir[1, :-1], out[1:, :, H:]))
    return torch.stack([linear_bwd_weight(dy.reshape(M, G), x, (1, M, 0, 2 * H, 1), G, H, True, False)[0] for dy, x in pairs])


def crnn_lstm_bf16_train_fwd(xg, mw, images_per_group=0):
    """`tpspp_crnn_lstm_bf16_train_fwd`: `crnn_lstm_bf16` (the same bits) that keeps what `crnn_lstm_bf16_bwd` reads ->
    (out (T, N, 512), gates (T, N, 2, 1024) after their activations, cell (T, N, 2, 256)), all fp32."""
    return _lstm_fwd("crnn_lstm_bf16_train_fwd", "tpspp_crnn_lstm_bf16_train_fwd", xg, mw, images_per_group, True, True)


def crnn_lstm_bf16_bwd(d_out, gates, cell, mw_t, images_per_group=0):
    """`tpspp_crnn_lstm_bf16_bwd`: `crnn_lstm_bwd` with da W_hh on the bf16 matrix cores.  mw_t =
    `arrange_mfma16(w_hh.transpose(1, 2), x3=...)`, the (2, 256, 1024) per-direction transposes -> d_xg (T, N, 2, 1024), the
    unrounded fp32 gradient of the pre-activations."""
    return _lstm_bwd("crnn_lstm_bf16_bwd", "tpspp_crnn_lstm_bf16_bwd", d_out, gates, cell, mw_t, images_per_group, True)[0]


def linear_bwd_weight_bf16_workspace_floats(batch, M, O, K):
    return _query("tpspp_linear_bwd_weight_bf16_workspace_floats", batch, M, O, K)


def linear_bwd_weight_bf16(dy, dy_strides, x, x_strides, batch, M, O, K, x3=True):
    """`tpspp_linear_bwd_weight_bf16`: dW (O, K) = sum over the batch * M rows of dy[b][r][:]^T x[b][r][:] on the bf16 matrix
    cores, both fp32 operands read through (batch, row, column) element strides (views are taken as they are) and rounded
    or (x3) split as they are staged; a fixed split over the rows, bitwise reproducible."""
    who = "linear_bwd_weight_bf16"
    for name, t in ((f"{who} dy", dy), (f"{who} x", x)):
        _chk_gpu(name, t)
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if dy.device != x.device:
        raise ValueError(f"{who}: operands on different devices")
    dw = torch.empty((O, K), device=dy.device, dtype=torch.float32)
    ws, n = _ws_n(linear_bwd_weight_bf16_workspace_floats(batch, M, O, K), dy.device)
    sd, sx = _i64(*dy_strides), _i64(*x_strides)
    _call("tpspp_linear_bwd_weight_bf16", dy, batch, M, O, K, dy, _vp(sd), x, _vp(sx), dw, ws, n, int(bool(x3)))
    return dw


def _bilstm_bf16_fwd(x, w_ih, b, w_hh, cfg):
    """`_BiLstmFunction.forward` in a reduced mode: both products on the bf16 matrix cores."""
    desc, T, N, group, mode = cfg
    x3 = mode == "bf16x3"
    xg = linear_bf16_fwd(x, desc, arrange_mfma16(w_ih, b, x3=x3)).view(T, N, 2, 4 * CRNN_HIDDEN)
    return crnn_lstm_bf16_train_fwd(xg, arrange_mfma16(w_hh, x3=x3), group)


def _bilstm_bf16_bwd(d_out, x, w_ih, w_hh, out, gates, cell, cfg, need):
    """`_BiLstmFunction.backward` in a reduced mode -> (dx, dw_ih (8 H, K), db (8 H), dw_hh (2, 4 H, H)), None where not
    needed: the recurrence, d w_ih, d w_hh and dx on the bf16 matrix cores, the bias gradient exact fp32."""
    desc, T, N, group, mode = cfg
    x3 = mode == "bf16x3"
    H, G, K = CRNN_HIDDEN, 4 * CRNN_HIDDEN, w_ih.shape[1]
    d_xg = crnn_lstm_bf16_bwd(d_out.float().contiguous(), gates, cell, arrange_mfma16(w_hh.transpose(1, 2), x3=x3), group)
    dy = d_xg.view(T * N, 2 * G)
    nb, Mi, sb, si, sk = desc
    dw_ih = linear_bwd_weight_bf16(dy, (Mi * 2 * G, 2 * G, 1), x, (sb, si, sk), nb, Mi, 2 * G, K, x3) if any(need[1:3]) else None
    db = linear_bwd_weight(dy, x, desc, 2 * G, K, False, True)[1] if any(need[5:9]) else None
    dx = None
    if need[0]:
        dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        w_t = arrange_mfma16(w_ih.t(), x3=x3)                      # (K rows, 8 H): dx = dy w_ih
        if x.dim() == 4:                                            # tokens of an NCHW map: (t, n, c) = x[n, c, 0, t]
            sn, sc, _, sw = dx.stride()
            mm_bf16(dy, (N * 2 * G, 2 * G, 1), w_t, dx, (sw, sn, sc), T, N)
        else:
            mm_bf16(dy, (N * 2 * G, 2 * G, 1), w_t, dx, (N * K, K, 1), T, N)
    dw_hh = None
    if any(need[3:5]):
        if T < 2 or N == 0:
            dw_hh = torch.zeros((2, G, H), device=x.device, dtype=torch.float32)
        else:                                                       # the shifted views, read in place
            sd, sx = (N * 2 * G, 2 * G, 1), (N * 2 * H, 2 * H, 1)
            dw_hh = torch.stack([
                linear_bwd_weight_bf16(d_xg[1:, :, 0], sd, out[:-1, :, :H], sx, T - 1, N, G, H, x3),
                linear_bwd_weight_bf16(d_xg[:-1, :, 1], sd, out[1:, :, H:], sx, T - 1, N, G, H, x3)])
    return dx, dw_ih, db, dw_hh


class _BiLstmFunction(torch.autograd.Function):
    """One bidirectional nn.LSTM layer with zero initial state.  Saves the tokens, the concatenated weights, the output and
    the recurrence's gates and cell states; the input projection's result is not kept.  cfg = (desc, T, N, group, mode): mode
    None runs the exact fp32 kernels, "bf16x3" the bf16 matrix cores (`_bilstm_bf16_fwd` / `_bilstm_bf16_bwd`)."""

    @staticmethod
    def forward(ctx, x, w_ih0, w_ih1, w_hh0, w_hh1, b_ih0, b_hh0, b_ih1, b_hh1, cfg):
        desc, T, N, group, mode = cfg
        w_ih = torch.cat([w_ih0, w_ih1]).float().contiguous()
        b = torch.cat([b_ih0 + b_hh0, b_ih1 + b_hh1]).float().contiguous()
        w_hh = torch.stack([w_hh0, w_hh1]).float().contiguous()
        if mode is None:
            xg = linear_fwd(x, desc, w_ih, b).view(T, N, 2, 4 * CRNN_HIDDEN)
            out, gates, cell = crnn_lstm_train_fwd(xg, w_hh, group)
        else:
            out, gates, cell = _bilstm_bf16_fwd(x, w_ih, b, w_hh, cfg)
        ctx.save_for_backward(x, w_ih, w_hh, out, gates, cell)
        ctx.cfg = cfg
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        x, w_ih, w_hh, out, gates, cell = ctx.saved_tensors
        desc, T, N, group, mode = ctx.cfg
        need = ctx.needs_input_grad
        H, K = CRNN_HIDDEN, w_ih.shape[1]
        if mode is not None:
            dx, dw_ih, db, dw_hh = _bilstm_bf16_bwd(d_out, x, w_ih, w_hh, out, gates, cell, ctx.cfg, need)
        else:
            w_hh_t = torch.stack([transpose2d(w_hh[0]), transpose2d(w_hh[1])])
            d_xg, d_dir = crnn_lstm_bwd(d_out.float().contiguous(), gates, cell, w_hh_t, group, direction_major=True)
            dy = d_xg.view(T * N, 8 * H)
            dw_ih, db = linear_bwd_weight(dy, x, desc, 8 * H, K, any(need[1:3]), any(need[5:9]))
            dx = None
            if need[0]:
                dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
                if x.dim() == 4:                                     # tokens of an NCHW map: (t, n, c) = x[n, c, 0, t]
                    sn, sc, _, sw = dx.stride()
                    linear_bwd_data(dy, w_ih, dx, (T, N, sw, sn, sc))
                else:
                    linear_bwd_data(dy, w_ih, dx, (T, N, N * K, K, 1))
            dw_hh = crnn_lstm_bwd_w_hh(d_dir, out) if any(need[3:5]) else None
        gw = (None, None) if dw_ih is None else (dw_ih[:4 * H], dw_ih[4 * H:])
        # (b_ih and b_hh of a direction receive the same values in tensors of their own: autograd may keep a gradient it is
        # handed as the parameter's .grad, and two parameters must not share one)
        gb = (None,) * 4 if db is None else (db[:4 * H], db[:4 * H].clone(), db[4 * H:], db[4 * H:].clone())
        gh = (None, None) if dw_hh is None else (dw_hh[0], dw_hh[1])
        return (dx, gw[0], gw[1], gh[0], gh[1], *gb, None)


def crnn_bilstm_autograd(x, desc, T, N, lstm, images_per_group=0, mode=None):
    """The bidirectional nn.LSTM(K, 256) `lstm` with zero initial state on the token operand x (`desc` = (T, N, batch stride,
    row stride, k stride) as `linear_fwd` takes it: a dense (T, N, K) tensor, or the (N, K, 1, T) feature map read in place)
    -> (T, N, 512), differentiable in x and in all eight parameters of the layer.
    mode None (exact fp32): the input projection and dx on `tpspp_mm_f32`, d w_ih and the bias gradient on
    `tpspp_linear_bwd_weight`, the recurrence on `tpspp_crnn_lstm_train_fwd` / `tpspp_crnn_lstm_bwd`, d w_hh on
    `tpspp_linear_bwd_weight` over the direction-major copy of d_xg and the shifted view of the output.
    mode "bf16x3" (the three-term split on the bf16 matrix cores, fp32 accumulation): the input projection and dx on
    `tpspp_mm_bf16` (dx of a feature map written through its strides), the recurrence on
    `tpspp_crnn_lstm_bf16_train_fwd` / `tpspp_crnn_lstm_bf16_bwd`, d w_ih and d w_hh on `tpspp_linear_bwd_weight_bf16` (d w_hh
    over the shifted views of d_xg and the output, read in place); the bias gradient stays on `tpspp_linear_bwd_weight`,
    exact fp32.  The weights are arranged (`arrange_mfma16`, torch code on their device) once per forward and once per
    backward; nothing synchronises with the host."""
    who = "crnn_bilstm_autograd"
    if not (mode is None or (isinstance(mode, str) and mode == "bf16x3")):
        raise ValueError(f'{who}: mode must be None or "bf16x3"')
    _chk_gpu(f"{who} x", x)
    if x.dtype != torch.float32:
        raise TypeError(f"{who}: x must be float32, got {x.dtype}")
    if lstm.hidden_size != CRNN_HIDDEN or lstm.num_layers != 1 or not lstm.bidirectional or not lstm.bias:
        raise ValueError(f"{who}: one bidirectional layer of {CRNN_HIDDEN} hidden units with biases")
    K = lstm.input_size
    if x.dim() == 4:
        if x.shape[2] != 1 or (x.shape[3], x.shape[0], x.shape[1]) != (T, N, K):
            raise ValueError(f"{who}: a feature map must be (N, K, 1, T) = ({N}, {K}, 1, {T}), got {tuple(x.shape)}")
    elif tuple(x.shape) != (T, N, K) or not x.is_contiguous():
        raise ValueError(f"{who}: x must be a dense ({T}, {N}, {K}) tensor or an (N, K, 1, T) feature map, got {tuple(x.shape)}")
    return _BiLstmFunction.apply(x, lstm.weight_ih_l0, lstm.weight_ih_l0_reverse, lstm.weight_hh_l0, lstm.weight_hh_l0_reverse,
                                 lstm.bias_ih_l0, lstm.bias_hh_l0, lstm.bias_ih_l0_reverse, lstm.bias_hh_l0_reverse,
                                 (tuple(int(v) for v in desc), int(T), int(N), int(images_per_group), mode))


class _LinearNwcFunction(torch.autograd.Function):
    """nn.Linear on (W, N, K) tokens whose result is written as (N, W, O): no layout pass in either direction."""

    @staticmethod
    def forward(ctx, x, w, b):
        W, N, K = x.shape
        O = w.shape[0]
        ctx.save_for_backward(x, w)
        y = torch.empty((N, W, O), device=x.device, dtype=torch.float32)
        return mm(x, (N * K, K, 1), w, (0, K, 1), y, (O, W * O, 1), W, N, O, K, bias=b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        W, N, K = x.shape
        O = w.shape[0]
        gy = gy.float().contiguous().view(N * W, O)                  # rows (n, w): x[w, n] through its strides
        desc = (N, W, K, N * K, 1)
        dw, db = linear_bwd_weight(gy, x, desc, O, K, need[1], need[2])
        dx = linear_bwd_data(gy, w, torch.empty_like(x), desc) if need[0] else None
        return dx, dw, db


def linear_nwc_autograd(x, lin):
    """nn.Linear `lin` on dense (W, N, K) tokens -> (N, W, O), differentiable: `CRNNDecoder`'s last embedding."""
    x = _chk("linear_nwc_autograd x", x, 3)
    if x.shape[-1] != lin.weight.shape[1]:
        raise ValueError(f"linear_nwc_autograd: input width {x.shape[-1]} against weight {tuple(lin.weight.shape)}")
    return _LinearNwcFunction.apply(x, lin.weight, lin.bias)


CTC_MAX_CLASSES, CTC_MAX_TARGET = 1024, 1024


def crnn_ctc_loss_workspace_floats(N, T, Lmax):
    return _query("tpspp_crnn_ctc_loss_workspace_floats", N, T, Lmax)


def _ctc_operands(who, logits, targets, target_len, input_len):
    logits = _chk(f"{who} logits", logits, 3)
    N = logits.shape[0]
    dev = logits.device
    if not isinstance(targets, torch.Tensor) or targets.is_floating_point() or targets.dim() != 2 or targets.shape[0] != N:
        raise ValueError(f"{who}: targets must be ({N}, Lmax) integers")
    out = [logits, targets.to(device=dev, dtype=torch.int32).contiguous()]
    for name, t in (("target_len", target_len), ("input_len", input_len)):
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or tuple(t.shape) != (N,):
            raise ValueError(f"{who}: {name} must be ({N}) integers")
        out.append(t.to(device=dev, dtype=torch.int32).contiguous())
    return out


def crnn_ctc_loss_fwd(logits, targets, target_len, input_len, blank=0, zero_infinity=False, reduction=0):
    """`tpspp_crnn_ctc_loss_fwd` on raw logits (N, T, C), padded int32 targets (N, Lmax) and int32 lengths (N), all on the
    device -> (loss (N), lse (N, T), reduced (1) | None, ws): lse and ws are what `crnn_ctc_loss_bwd` reads."""
    N, T, C = logits.shape
    Lmax = targets.shape[1]
    dev = logits.device
    loss = torch.empty((N,), device=dev, dtype=torch.float32)
    lse = torch.empty((N, T), device=dev, dtype=torch.float32)
    red = torch.empty((1,), device=dev, dtype=torch.float32) if reduction else None
    ws, n = _ws_n(crnn_ctc_loss_workspace_floats(N, T, Lmax), dev)
    if N == 0 and reduction:                   # the library returns before any launch
        red.fill_(float("nan") if reduction == 1 else 0.0)
    _call("tpspp_crnn_ctc_loss_fwd", logits, logits, targets, target_len, input_len, N, T, C, Lmax, int(blank),
          int(bool(zero_infinity)), reduction, loss, lse, red, ws, n)
    return loss, lse, red, ws


def crnn_ctc_loss_bwd(g, logits, targets, target_len, input_len, lse, ws, blank=0, zero_infinity=False, reduction=0):
    """`tpspp_crnn_ctc_loss_bwd`: d_logits (N, T, C) dense, exact zeros from each image's input length on."""
    N, T, C = logits.shape
    d = torch.empty((N, T, C), device=logits.device, dtype=torch.float32)
    _call("tpspp_crnn_ctc_loss_bwd", logits, g, logits, targets, target_len, input_len, lse, ws, N, T, C, targets.shape[1],
          int(blank), int(bool(zero_infinity)), reduction, d)
    return d


class _CtcLossFunction(torch.autograd.Function):
    """Saves the logits, the targets and lengths, the per-position log-sum-exp and the alpha table."""

    @staticmethod
    def forward(ctx, logits, targets, target_len, input_len, cfg):
        blank, zero_infinity, reduction = cfg
        loss, lse, red, ws = crnn_ctc_loss_fwd(logits, targets, target_len, input_len, blank, zero_infinity, reduction)
        ctx.save_for_backward(logits, targets, target_len, input_len, lse, ws)
        ctx.cfg = cfg
        return red.view(()) if reduction else loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        logits, targets, target_len, input_len, lse, ws = ctx.saved_tensors
        if logits.shape[0] == 0:
            return torch.zeros_like(logits), None, None, None, None
        d = crnn_ctc_loss_bwd(g.float().contiguous().view(-1), logits, targets, target_len, input_len, lse, ws, *ctx.cfg)
        return d, None, None, None, None


def crnn_ctc_loss_autograd(logits, targets, target_len, input_len, blank=0, reduction="mean", zero_infinity=False):
    """`F.ctc_loss(log_softmax(logits, 2).permute(1, 0, 2), ...)` on HIP kernels from the raw logits (N, T, C): a scalar for
    "mean" / "sum", (N) for "none".  targets (N, Lmax) padded, target_len and input_len (N): integers on the host or the
    device; lengths are clamped to 0 .. Lmax and 0 .. T.  Targets on the host are checked here, where they originate: one
    outside 0 .. C - 1 or equal to blank (within its image's length) raises."""
    who = "crnn_ctc_loss_autograd"
    if reduction not in _REDUCTIONS:
        raise ValueError(f'{who}: reduction must be "none", "mean" or "sum", got {reduction!r}')
    if isinstance(logits, torch.Tensor) and logits.dim() == 3:
        N, T, C = logits.shape
        if not 2 <= C <= CTC_MAX_CLASSES or not 0 <= int(blank) < C or T < 1:
            raise ValueError(f"{who}: 2 to {CTC_MAX_CLASSES} classes, blank among them, at least one position; got "
                             f"{tuple(logits.shape)}, blank {blank}")
    if isinstance(targets, torch.Tensor) and targets.dim() == 2:
        if targets.shape[1] > CTC_MAX_TARGET:
            raise ValueError(f"{who}: at most {CTC_MAX_TARGET} target positions, got {targets.shape[1]}")
        if not targets.is_cuda and isinstance(target_len, torch.Tensor) and not target_len.is_cuda and targets.numel():
            used = torch.arange(targets.shape[1])[None, :] < target_len.reshape(-1, 1)
            bad = used & ((targets < 0) | (targets >= logits.shape[2]) | (targets == int(blank)))
            if bad.any():
                n, j = (int(v) for v in bad.nonzero()[0])
                raise ValueError(f"{who}: target {int(targets[n, j])} of image {n}, position {j}: outside 0 .. "
                                 f"{logits.shape[2] - 1} or the blank {int(blank)}")
    logits, targets, target_len, input_len = _ctc_operands(who, logits, targets, target_len, input_len)
    return _CtcLossFunction.apply(logits, targets, target_len, input_len,
                                  (int(blank), bool(zero_infinity), _REDUCTIONS[reduction]))
