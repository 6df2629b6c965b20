"""Cases and float64 references shared by tests/test_tps_train_host.py and tests/test_gpu_tps_train.py: the fused
BatchNorm + ReLU + 2x2 max-pool kernels of tpspp_bn_pool_train.hip (a helper module, not a test file).

Every case has a channel with a negative gamma (the maximum of the activation sits at the minimum of z), a constant channel
(a tie in every window, beta > 0) and a channel of mean 1e3.  z lies on a dyadic grid (multiples of 1/4, hence of 1/64), so
equal values are equal in every precision; `make_case` checks in float64, for the batch-statistics and the
running-statistics activation alike, that the top two activations of every window are exactly equal or at least 1e-3 apart
and that no selected activation lies in (0, 1e-3), and moves on to the next seed until both hold (at most MAX_SEEDS).  A
flipped arg-max or ReLU mask in fp32 is then the kernel's doing, not rounding's."""
import functools

import torch
import torch.nn.functional as F

CASES = [(1, 3, 2, 2),
         (2, 5, 5, 7),            # odd both ways
         (3, 8, 37, 41),          # M = 4551: two slices, scalar path
         (3, 64, 8, 25),          # the third layer's map: W odd, H*W % 4 == 0
         (2, 128, 16, 50),        # the second layer's map
         (1, 64, 32, 100)]        # the first layer's map
EPS = 1e-5
MOMENTUM = 0.1
GAP = 1e-3
MAX_SEEDS = 256


def case_id(c):
    return "x".join(str(v) for v in c)


def windows(t):
    """(N, C, H, W) -> (N, C, H/2, W/2, 4): each 2x2 window's elements in scan order (row by row from its first)."""
    N, C, H, W = t.shape
    Ho, Wo = H // 2, W // 2
    return t[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)


def unwindows(w, H, W):
    """The inverse of `windows`; the row / column no window covers is zero."""
    N, C, Ho, Wo, _ = w.shape
    out = torch.zeros((N, C, H, W), dtype=w.dtype)
    out[:, :, :2 * Ho, :2 * Wo] = w.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    return out


def vec(v):
    return v.view(1, -1, 1, 1)


def activation(z, mean, rstd, gamma, beta):
    return torch.relu(vec(gamma) * (z - vec(mean)) * vec(rstd) + vec(beta))


def scan(a4):
    """ATen's scan over the last axis (4 window elements): (m, k), v replaces m if v > m or v != v."""
    m = a4[..., 0].clone()
    k = torch.zeros(m.shape, dtype=torch.long)
    for j in range(1, 4):
        v = a4[..., j]
        upd = (v > m) | torch.isnan(v)
        m = torch.where(upd, v, m)
        k = torch.where(upd, torch.full_like(k, j), k)
    return m, k


def batch_stats(z, eps=EPS):
    z = z.double()
    return z.mean((0, 2, 3)), 1 / torch.sqrt(z.var((0, 2, 3), unbiased=False) + eps)


def eval_stats(rm, rv, eps=EPS):
    return rm.double(), 1 / torch.sqrt(rv.double() + eps)


def restated_backward(z, dp, mean, rstd, gamma, beta, train):
    """include/tpspp.h's formulas for tpspp_bn_pool2x2_bwd_reduce / _bwd_data in the dtype of the arguments:
    (p, dz, sum_dr, sum_dr_x)."""
    N, C, H, W = z.shape
    m, k = scan(windows(activation(z, mean, rstd, gamma, beta)))
    g = torch.where(m > 0, dp, torch.zeros_like(dp))
    dr = unwindows(F.one_hot(k, 4).to(z.dtype) * g.unsqueeze(-1), H, W)
    xhat = (z - vec(mean)) * vec(rstd)
    sum_dr, sum_dr_x = dr.sum((0, 2, 3)), (dr * xhat).sum((0, 2, 3))
    M = N * H * W
    if train:
        dz = vec(gamma * rstd) * (dr - vec(sum_dr) / M - xhat * vec(sum_dr_x) / M)
    else:
        dz = vec(gamma * rstd) * dr
    return m, dz, sum_dr, sum_dr_x


def _well_separated(z, mean, rstd, gamma, beta):
    a4 = windows(activation(z.double(), mean, rstd, gamma.double(), beta.double()))
    top = a4.sort(-1, descending=True).values
    gap = top[..., 0] - top[..., 1]
    if not bool(((gap == 0) | (gap >= GAP)).all()):
        return False
    m, _ = scan(a4)
    return not bool(((m > 0) & (m < GAP)).any())


def _draw(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.round(1.5 * torch.randn((N, C, H, W), generator=g) * 4) / 4
    sign = torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    gamma = sign * (0.5 + torch.randint(0, 25, (C,), generator=g) / 16)
    beta = torch.randint(-8, 9, (C,), generator=g) / 16
    rm = torch.randint(-8, 9, (C,), generator=g) / 32
    rv = 0.5 + torch.randint(0, 33, (C,), generator=g) / 16
    gamma[0] = -1.25                                                        # the maximum of a sits at the minimum of z
    z[:, 1], gamma[1], beta[1], rm[1] = 0.75, 1.0, 0.5, 0.5                 # constant: a tie in every window
    z[:, 2] = 1e3 + torch.round(torch.randn((N, H, W), generator=g) * 4) / 4
    rm[2] = 1e3
    dp = torch.randn((N, C, H // 2, W // 2), generator=g)
    return dict(z=z, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, dp=dp, seed=seed)


@functools.lru_cache(maxsize=None)
def make_case(N, C, H, W):
    """The first seed whose draw is well separated in both modes: dict(z, gamma, beta, running_mean, running_var, dp,
    seed), fp32 CPU tensors.  Treat them as read-only: the result is shared."""
    for seed in range(MAX_SEEDS):
        c = _draw(N, C, H, W, seed)
        modes = (batch_stats(c["z"]), eval_stats(c["running_mean"], c["running_var"]))
        if all(_well_separated(c["z"], *st, c["gamma"], c["beta"]) for st in modes):
            return c
    raise AssertionError(f"no well-separated draw for {(N, C, H, W)} in {MAX_SEEDS} seeds")


@functools.lru_cache(maxsize=None)
def autograd_reference(N, C, H, W, train, dtype=torch.float64, device="cpu"):
    """max_pool2d(relu(batch_norm(z))) forward and backward with PyTorch's own layers in `dtype` on `device`:
    dict(p, dz, dgamma, dbeta, running_mean, running_var) on the CPU."""
    c = make_case(N, C, H, W)
    to = lambda t: t.to(device).to(dtype)                                    # noqa: E731
    z = to(c["z"]).requires_grad_(True)
    gamma, beta = to(c["gamma"]).requires_grad_(True), to(c["beta"]).requires_grad_(True)
    rm, rv = to(c["running_mean"]).clone(), to(c["running_var"]).clone()
    p = F.max_pool2d(F.relu(F.batch_norm(z, rm, rv, gamma, beta, bool(train), MOMENTUM, EPS)), 2, 2)
    p.backward(to(c["dp"]))
    out = dict(p=p.detach(), dz=z.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)
    return {k: v.cpu() for k, v in out.items()}
