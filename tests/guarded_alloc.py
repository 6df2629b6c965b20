"""Guard bands and poison for device allocations (a helper module of the memory-safety sweep, not a conftest).

No sanitizer runs on the GPUs this project targets, so a store a few floats past an output, or an output element a kernel
never writes, goes unseen by a test that compares values only.  `guarded(device)` makes both visible:

    with guarded(dev) as g:
        x = g.input(x_cpu)              # input copied between NaN bands
        y = ops.something(x)            # every torch.empty / torch.empty_like of the wrapper is served from here
        g.check(y)                      # synchronise; guards intact; no poison left in y

Layout of a served allocation (one private uint8 buffer):   [ guard | payload | guard ]
  * each guard is at least GUARD = 64 KiB of 0xA5 (more than one workgroup of the library stores: 128 pixels x 64
    channels x 4 B = 32 KiB), the leading one stretched so that the payload starts on ALIGN = 512 bytes, which is what
    PyTorch's caching allocator gives: kernels take the same vector / scalar paths as in production;
  * the payload is filled with 0xFF: fp32 0xFFFFFFFF and bf16 0xFFFF are NaNs no kernel produces from finite inputs,
    integer types read -1.
Layout of an input (`Guard.input`):   [ guard | NaN band | payload | NaN band | guard ]
  * the bands (GUARD bytes of 0xFF each) make a read outside the input that reaches a result turn that result into NaN;
    they are checked like the guards.

What this cannot see: a read outside an input that never reaches a result, and a store that skips more than a whole guard.
"""
import contextlib
import operator
import traceback

import torch

GUARD = 64 * 1024
ALIGN = 512
GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF

_REAL_EMPTY = torch.empty
_REAL_EMPTY_LIKE = torch.empty_like
_HERE = __file__.rsplit(".", 1)[0]
_FLOAT_AS_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16,
                 torch.float64: torch.int64}
TOTALS = {"allocations": 0, "inputs": 0, "bytes": 0}          # over the whole process: the sweep reports them


class GuardError(AssertionError):
    pass


def _caller():
    for fr in reversed(traceback.extract_stack(limit=12)):
        if not fr.filename.startswith(_HERE) and "contextlib" not in fr.filename:
            return f"{fr.filename.rsplit('/', 1)[-1]}:{fr.lineno} in {fr.name}"
    return "?"


def _same_device(a, b):
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True
    cur = torch.cuda.current_device()
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


class Unguarded:
    """A returned tensor that, for the stated reason, does not live in a guarded allocation (a host copy, a clone made by
    a torch op, ...): `check` holds it to the poison test but not to the "lies inside a recorded allocation" test."""

    def __init__(self, tensor, why):
        assert isinstance(why, str) and len(why) > 10
        self.tensor, self.why = tensor, why


def tensors_in(obj, _loose=None):
    """Every tensor in a nest of tuples, lists, dicts and `Unguarded` markers."""
    if isinstance(obj, Unguarded):
        if _loose is not None and obj.tensor is not None:
            _loose.add(id(obj.tensor))
        yield from tensors_in(obj.tensor, _loose)
    elif isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from tensors_in(v, _loose)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            yield from tensors_in(v, _loose)


def poison_count(t):
    """Number of elements of a float tensor that still hold the all-ones poison word (0 for other dtypes)."""
    it = _FLOAT_AS_INT.get(t.dtype)
    if it is None or t.numel() == 0:
        return 0
    return int((t.detach().view(it) == -1).sum())


class _Record:
    __slots__ = ("buf", "off", "nbytes", "segments", "shape", "dtype", "where", "kind")


class Guard:
    def __init__(self, device):
        self.device = torch.device(device)
        self.records = []
        self.fallthrough = []          # requests on this device that the patch did not recognise: (call site, what)

    # ---- allocation -------------------------------------------------------------------------------------------------
    def _carve(self, shape, dtype, band, kind):
        numel = 1
        for s in shape:
            numel *= int(s)
        nbytes = numel * _itemsize(dtype)
        lead = GUARD + band
        buf = _REAL_EMPTY((lead + ALIGN + nbytes + band + GUARD,), dtype=torch.uint8, device=self.device)
        off = lead + (-(buf.data_ptr() + lead)) % ALIGN
        total = off + nbytes + band + GUARD
        buf = buf[:total]
        buf.fill_(GUARD_BYTE)
        buf[off - band:off + nbytes + band].fill_(POISON_BYTE)
        r = _Record()
        r.buf, r.off, r.nbytes, r.shape, r.dtype, r.where, r.kind = buf, off, nbytes, tuple(shape), dtype, _caller(), kind
        r.segments = [(0, off - band, GUARD_BYTE), (off + nbytes + band, total, GUARD_BYTE)]
        if band:
            r.segments += [(off - band, off, POISON_BYTE), (off + nbytes, off + nbytes + band, POISON_BYTE)]
        self.records.append(r)
        TOTALS["inputs" if kind == "input" else "allocations"] += 1
        TOTALS["bytes"] += nbytes
        payload = buf[off:off + nbytes].view(dtype).view(tuple(shape))
        assert payload.data_ptr() % ALIGN == 0
        return payload

    def empty(self, shape, dtype=torch.float32):
        """A poisoned, guarded tensor (what the patched torch.empty serves)."""
        return self._carve(shape, dtype, 0, "allocation")

    def input(self, t):
        """A guarded copy of `t` on the guard's device, NaN bands on both sides, payload 512-byte aligned."""
        t = t.detach()
        p = self._carve(tuple(t.shape), t.dtype, GUARD, "input")
        p.copy_(t.contiguous())
        return p

    # ---- checks -----------------------------------------------------------------------------------------------------
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def guard_failures(self):
        """[(record, segment, offset of the first changed byte relative to the payload)] for every damaged guard."""
        self._sync()
        if not self.records:
            return []
        counts, index = [], []
        for r in self.records:
            for seg in r.segments:
                lo, hi, byte = seg
                if hi > lo:
                    counts.append((r.buf[lo:hi] != byte).sum())
                    index.append((r, seg))
        bad = torch.stack(counts).cpu().tolist()          # one synchronising copy for all guards
        out = []
        for n, (r, (lo, hi, byte)) in zip(bad, index):
            if n:
                first = lo + int(torch.nonzero(r.buf[lo:hi] != byte)[0])
                out.append((r, (lo, hi, byte), first - r.off, n))
        return out

    def allocations(self):
        return sum(1 for r in self.records if r.kind == "allocation")

    def home_of(self, t):
        """The record whose payload holds the first element of `t`, or None."""
        p = t.data_ptr()
        for r in self.records:
            base = r.buf.data_ptr() + r.off
            if r.nbytes and base <= p < base + r.nbytes:
                return r
        return None

    def check(self, returned=None, require_guarded=False):
        """Synchronise; every guard byte of every allocation and input is intact; no float tensor in `returned` still
        holds a poison word.  `require_guarded`: every non-empty float tensor in `returned` must also lie inside a recorded
        allocation (or input: a buffer updated in place) unless it is wrapped in `Unguarded(tensor, why)` -- otherwise an
        output that came from some other allocator would be held to neither guards nor poison without anyone noticing.
        Returns the number of allocations (inputs not counted) that were served and checked."""
        msgs = []
        for r, (lo, hi, byte), rel, n in self.guard_failures():
            side = "before" if hi <= r.off else "after"
            pos = f"{-rel} bytes before the payload" if rel < 0 else f"{rel - r.nbytes} bytes past its end"
            msgs.append(f"guard {side} {r.kind} {r.shape} {r.dtype} ({r.nbytes} B, made at {r.where}) overwritten: "
                        f"{n} bytes changed, the first {pos} (payload offset {rel}), expected 0x{byte:02X}")
        loose = set()
        for i, t in enumerate(tensors_in(returned, loose)):
            if (require_guarded and id(t) not in loose and t.dtype in _FLOAT_AS_INT and t.numel()
                    and self.home_of(t) is None):
                msgs.append(f"returned tensor #{i} {tuple(t.shape)} {t.dtype} on {t.device} lies in no guarded allocation: "
                            f"neither guards nor poison cover it (wrap it in Unguarded(tensor, why) if that is intended)")
            n = poison_count(t)
            if n:
                it = _FLOAT_AS_INT[t.dtype]
                first = int(torch.nonzero(t.detach().reshape(-1).view(it) == -1)[0]) if t.is_contiguous() else -1
                where = next((r.where for r in self.records if r.kind == "allocation" and r.nbytes and
                              r.buf.data_ptr() + r.off <= t.data_ptr() < r.buf.data_ptr() + r.off + r.nbytes), "?")
                msgs.append(f"returned tensor #{i} {tuple(t.shape)} {t.dtype} (allocated at {where}) has {n} elements "
                            f"never written (poison 0x{POISON_BYTE:02X}), the first at flat index {first}")
        if msgs:
            raise GuardError("\n".join(msgs))
        return self.allocations()


def _itemsize(dtype):
    return _REAL_EMPTY((), dtype=dtype).element_size()


def _shape_of(args):
    """The requested shape as Python ints (numpy integers and the like included), or None if it is not a plain shape."""
    dims = args[0] if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)) else args
    if not dims and not (len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size))):
        return None
    try:
        if any(isinstance(d, bool) for d in dims):
            return None
        return tuple(operator.index(d) for d in dims)
    except TypeError:
        return None


def _numel_hint(args):
    """Best effort: is this request certainly empty?  (Only used to keep zero-size requests out of the fall-through list.)"""
    try:
        dims = args[0] if len(args) == 1 and not isinstance(args[0], int) else args
        return 0 if any(int(d) == 0 for d in dims) else 1
    except Exception:
        return 1


@contextlib.contextmanager
def guarded(device):
    """Replace torch.empty / torch.empty_like so that plain allocations on `device` come from guarded, poisoned buffers.
    Zero-size requests, other devices and exotic keyword arguments (out, layout, pin_memory, memory_format, names, ...)
    go to the real functions, which are restored on exit whatever happens.  A non-empty request on `device` that is not
    served (exotic keywords, dimensions that are no Python ints, a non-contiguous empty_like) is listed in
    `Guard.fallthrough`, so that a caller can assert that nothing left the guards quietly."""
    g = Guard(device)

    def default_device():
        return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")

    def empty(*args, **kw):
        shape = _shape_of(args)
        extra = set(kw) - {"dtype", "device", "requires_grad"}
        dev = kw.get("device")
        here = _same_device(default_device() if dev is None else dev, g.device)
        if shape is None or extra or kw.get("requires_grad") or 0 in shape or not here:
            if here and _numel_hint(args) and (shape is None or 0 not in shape):
                g.fallthrough.append((_caller(), f"torch.empty{args} {sorted(kw)}"))
            return _REAL_EMPTY(*args, **kw)
        dtype = kw.get("dtype")
        return g._carve(shape, torch.get_default_dtype() if dtype is None else dtype, 0, "allocation")

    def empty_like(t, **kw):
        extra = set(kw) - {"dtype", "device"}
        dev = kw.get("device")
        here = _same_device(t.device if dev is None else dev, g.device)
        if extra or t.numel() == 0 or not t.is_contiguous() or t.layout != torch.strided or not here:
            if here and t.numel():
                g.fallthrough.append((_caller(), f"torch.empty_like({tuple(t.shape)}, strides {t.stride()}) {sorted(kw)}"))
            return _REAL_EMPTY_LIKE(t, **kw)
        dtype = kw.get("dtype")
        return g._carve(tuple(t.shape), t.dtype if dtype is None else dtype, 0, "allocation")

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield g
    finally:
        torch.empty, torch.empty_like = _REAL_EMPTY, _REAL_EMPTY_LIKE


def same_bits(a, b):
    """Bit-for-bit equality of two nests of tensors (floats compared as integers, so NaNs and signed zeros count)."""
    ta, tb = list(tensors_in(a)), list(tensors_in(b))
    if len(ta) != len(tb):
        return False, f"{len(ta)} tensors against {len(tb)}"
    for i, (x, y) in enumerate(zip(ta, tb)):
        if x.shape != y.shape or x.dtype != y.dtype:
            return False, f"tensor #{i}: {tuple(x.shape)} {x.dtype} against {tuple(y.shape)} {y.dtype}"
        it = _FLOAT_AS_INT.get(x.dtype)
        xi, yi = (x.detach().contiguous(), y.detach().contiguous())
        if it is not None:
            xi, yi = xi.view(it), yi.view(it)
        if not torch.equal(xi, yi):
            d = (xi != yi).reshape(-1)
            return False, (f"tensor #{i} {tuple(x.shape)} {x.dtype}: {int(d.sum())} elements differ, the first at flat "
                           f"index {int(torch.nonzero(d)[0])}")
    return True, ""
