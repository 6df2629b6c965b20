"""Shared by tests/test_crnn_vgg_train_host.py and tests/test_gpu_crnn_vgg_train.py (not a test file): the case table of
tpspp_crnn_maxpool_bwd (include/tpspp.h) and its reference, restated independently of the kernel as a plain loop over
windows with the scan rule the header states.

Data: integer-valued fp32, so every sum is exact in any order and a comparison is bit for bit.  y is ReLU-like -- values
0..3, more than half of them exact zeros, and a block of whole all-zero windows -- so ties are the common case; dp holds
non-zero integers.  Variants: "pm0" turns every other zero into -0 (ties between +0 and -0), "nonfinite" scatters NaN, +inf
and -inf over y."""
import numpy as np
import torch
import torch.nn.functional as F

P22 = ((2, 2), (2, 2), (0, 0))                 # pooling0, pooling1
RECT = ((2, 2), (2, 1), (0, 1))                # pooling2, pooling3: windows overlap along W

# (N, C, H, W, kernel, stride, padding, tag); tag "off1": y, dp on views one element off 16-byte alignment
CASES = [
    (2, 3, 4, 8, *P22, ""),                    # float4 form
    (2, 1, 4, 6, *P22, ""),                    # W % 4 != 0: scalar form
    (1, 2, 5, 7, *P22, ""),                    # odd H and W: the uncovered row and column are +0
    (2, 3, 4, 8, *P22, "off1"),                # the float4 shape on misaligned views: scalar form
    (1100, 64, 2, 2, *P22, ""),                # 70 400 planes, past any 65 535 grid limit
    (2, 3, 8, 25, *RECT, ""),                  # the VGG's own two rectangular pools at few channels
    (1, 2, 4, 26, *RECT, ""),
    (1, 1, 2, 1, *RECT, ""),                   # every window half padding
    (1, 1, 3, 4, *RECT, ""),                   # odd H
    (1, 2, 5, 5, (3, 3), (1, 1), (1, 1), ""),  # beyond the VGG: up to nine overlapping windows
    (1, 1, 6, 7, (3, 2), (2, 1), (1, 1), ""),
]
VARIANTS = ("plain", "pm0", "nonfinite")


def case_id(c):
    N, C, H, W, k, s, p, tag = c
    return f"{N}x{C}x{H}x{W}-k{k[0]}{k[1]}s{s[0]}{s[1]}p{p[0]}{p[1]}" + (f"-{tag}" if tag else "")


def out_size(H, W, k, s, p):
    return (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1


def make_case(c, variant="plain"):
    """(y (N, C, H, W), dp (N, C, Ho, Wo)) float32 on the CPU."""
    N, C, H, W, k, s, p, _ = c
    g = torch.Generator().manual_seed(1000 * H + 10 * W + VARIANTS.index(variant))
    y = torch.randint(-4, 4, (N, C, H, W), generator=g).clamp_(min=0).float()
    y[:, :, :2, :min(W, 4)] = 0.0                                  # whole all-zero windows in every plane
    if N * C > 1:
        y[0, 0] = 0.0                                              # ... and a whole all-zero plane
    flat = y.view(-1)
    if variant == "pm0":
        zeros = (flat == 0).nonzero().view(-1)
        flat[zeros[::2]] = -0.0
    elif variant == "nonfinite":
        idx = torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 6)]
        special = torch.tensor([float("nan"), float("inf"), float("-inf")]).roll((H + W) % 3)      # small maps differ
        flat[idx] = special.repeat(idx.numel() // 3 + 1)[:idx.numel()]
    Ho, Wo = out_size(H, W, k, s, p)
    dp = torch.randint(1, 6, (N, C, Ho, Wo), generator=g).float()
    dp = dp * (2 * torch.randint(0, 2, dp.shape, generator=g).float() - 1)
    assert (y == 0).float().mean() >= 1 / 3 and (dp != 0).all()
    return y, dp


def restated_backward(y, dp, k, s, p, relu_mask):
    """dy of the max-pool's input y for the output gradient dp: per window, in ascending (oh, ow), the rows and columns
    inside the map are scanned row by row from m = -inf; v replaces m if v > m or v is a NaN; the window's selected element
    is the last one that did, or its first element inside the map if none did; dp is added there.  relu_mask: +0 wherever
    not (y > 0).  Vectorised over the planes only."""
    N, C, H, W = y.shape
    Ho, Wo = out_size(H, W, k, s, p)
    yn = y.numpy().reshape(N * C, H, W)
    g = dp.numpy().reshape(N * C, Ho, Wo)
    dy = np.zeros_like(yn)
    planes = np.arange(N * C)
    with np.errstate(invalid="ignore"):
        for oh in range(Ho):
            for ow in range(Wo):
                rows = [r for r in range(oh * s[0] - p[0], oh * s[0] - p[0] + k[0]) if 0 <= r < H]
                cols = [q for q in range(ow * s[1] - p[1], ow * s[1] - p[1] + k[1]) if 0 <= q < W]
                m = np.full(N * C, -np.inf, np.float32)
                sr = np.full(N * C, rows[0])
                sc = np.full(N * C, cols[0])
                for r in rows:
                    for q in cols:
                        v = yn[:, r, q]
                        take = (v > m) | np.isnan(v)
                        m = np.where(take, v, m)
                        sr = np.where(take, r, sr)
                        sc = np.where(take, q, sc)
                dy[planes, sr, sc] += g[:, oh, ow]
        if relu_mask:
            dy = np.where(yn > 0, dy, np.float32(0.0))
    return torch.from_numpy(dy.reshape(N, C, H, W))


# ---- inputs away from the kinks --------------------------------------------------------------------------------------------
# The gradient of ReLU + max-pool is discontinuous in its input: where a pre-activation sits within rounding of zero, or a
# window's two largest activations within rounding of each other, which element receives the gradient is decided by the
# last bits of the convolution in front, and ONE such element moves a small layer's gradient by ~3e-3 relative L2 -- for any
# fp32 implementation, PyTorch's included.  A comparison against float64 under a 1e-5 bar therefore needs inputs whose
# float64 reference stays away from those kinks.  MARGIN is in units of the map's RMS: the rounding error of an fp32 sum of
# K = 4608 products (the VGG's widest convolution) is about sqrt(K) 2^-24 = 4e-6 of it.  The tests assert the margin on the
# float64 reference alone (never on the code under test) and take the first seed of a fixed sequence that has it.
MARGIN = 1e-5


def relu_margin(z):
    """min |z| / rms(z) of a pre-activation map."""
    return (z.abs().min() / z.pow(2).mean().sqrt()).item()


def pool_margin(a, k, s, p):
    """The smallest gap between the two largest elements of a window whose maximum is positive, over rms(a)."""
    N, C, H, W = a.shape
    ap = F.pad(a, (p[1], p[1], p[0], p[0]), value=float("-inf")).reshape(N * C, 1, H + 2 * p[0], W + 2 * p[1])
    top = F.unfold(ap, k, stride=s).topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1])[top[:, 0] > 0]
    return (gap.min() / a.pow(2).mean().sqrt()).item() if gap.numel() else float("inf")


def vgg_margin(vgg64, img64):
    """The smallest `relu_margin` / `pool_margin` over the seven activations and four pools of a float64 `VeryDeepVgg`
    (leaky_relu=False) on `img64`, in the module's own mode; the module's buffers are left as they were."""
    found, hooks = [], []
    names = [n for n, _ in vgg64.cnn.named_children()]
    for i, n in enumerate(names):
        mod = getattr(vgg64.cnn, n)
        if n.startswith("relu"):                                    # in place: read its input where it is produced
            hooks.append(getattr(vgg64.cnn, names[i - 1]).register_forward_hook(
                lambda m, inp, out: found.append(relu_margin(out))))
        elif n.startswith("pooling"):
            hooks.append(mod.register_forward_hook(lambda m, inp, out: found.append(
                pool_margin(inp[0], _two(m.kernel_size), _two(m.stride), _two(m.padding)))))
    state = {k: v.clone() for k, v in vgg64.state_dict().items()}
    with torch.no_grad():
        vgg64.cnn(img64)
    for h in hooks:
        h.remove()
    vgg64.load_state_dict(state)
    assert len(found) == 11
    return min(found)


def _two(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def off_by_one(t):
    """A contiguous view of `t`'s values that starts one element (4 bytes) into a fresh buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)
