"""CRNNDecoder's reduced-precision arithmetic restated on the CPU in float64, shared by tests/test_crnn_dec_bf16_host.py and
tests/test_gpu_crnn_dec_bf16.py (a helper module, not a test file).  Written like `crnn_bf16_cases.vgg64`:

  x3    every operand of a wide product split into hi = bf16(v), lo = bf16(v - hi) (`ops._hi_lo`'s rule); a product is
        hi*hi + hi*lo + lo*hi; float64 sums;
  bf16  the operands of both wide products rounded to bf16 (x and w_ih; h_{t-1} and w_hh); float64 sums;
  None  the exact float64 LSTM: nothing is rounded anywhere.

In the two reduced routes xg, c and h are rounded to fp32 where the kernels store them (xg in memory, c in registers, h in
`out` -- the h that is stored is unrounded fp32, only the copy that feeds the next step is rounded or split), and the
embeddings are exact products of the fp32 values they read.  The bars hang on

  restatement_error = rel(restatement, exact)          (relative L2, `rel` of tests/test_gpu_train_primitives.py)

  bf16x3   rel(kernel, exact)        <= max(2e-5, 2 x restatement_error)      (2e-5: the x3 bar of tests/test_gpu_conv_bf16.py)
  bf16     rel(kernel, exact)        <= 2 x restatement_error
  bf16     rel(kernel, restatement)  <= 0.25 x restatement_error

(bf16 cannot be compared value by value: an fp32-level difference in h can flip a bf16 rounding.  What the 0.25 x bar tells
apart, on the CPU at T = 26 with PyTorch-init weights, where the restatement sits 2.2-2.4e-3 from exact: an fp32-accumulating
variant with another summation order sits 1e-7 to 5e-5 from the restatement, flips included, at least 10 x inside the bar;
truncation in place of round-to-nearest-even sits 5.7e-3 away, outside it.)  References are cached:
each is computed once and shared by the tests that need it."""
import functools

import torch
import torch.nn as nn

import crnn_bf16_cases as BC

CC = BC.CC
H = 256
MODES = ["bf16x3", torch.bfloat16]
MODE_IDS = ["bf16x3", "bf16"]


def rel(got, want):
    want = want.detach().cpu().double()
    n = want.norm()
    d = (got.detach().cpu().double() - want).norm()
    return (d / n).item() if n > 0 else d.item()


def rb(x):
    """Rounded to bf16 (round to nearest even), as fp32."""
    return x.float().to(torch.bfloat16).float()


def split(x):
    hi = rb(x)
    return hi, rb(x.float() - hi)


def product64(a, w, mode):
    """a (R, K) times w (O, K)^T in float64 along one route.  The reduced routes read fp32 operands."""
    if mode is None:
        return a.double() @ w.double().t()
    if mode == "bf16x3":
        ah, al = split(a)
        wh, wl = split(w)
        return ah.double() @ wh.double().t() + al.double() @ wh.double().t() + ah.double() @ wl.double().t()
    return rb(a).double() @ rb(w).double().t()


def stored(x, mode):
    """A value as the route keeps it: fp32 where a kernel stores it, float64 in the exact route."""
    return x if mode is None else x.float()


def proj64(x, w, b, mode):
    """x (..., K) tokens -> x w^T + b, (..., O): the input projection (and, mode None on fp32 inputs, an embedding)."""
    y = product64(x.reshape(-1, x.shape[-1]), w, mode) + b.double()
    return stored(y.reshape(x.shape[:-1] + (w.shape[0],)), mode)


def lstm64(xg, w_hh, mode):
    """The recurrence: xg (T, N, 2, 4H), w_hh (2, 4H, H) -> (T, N, 2H)."""
    T, N = xg.shape[:2]
    out = torch.zeros((T, N, 2 * H), dtype=torch.float64 if mode is None else torch.float32)
    for d in range(2):
        h = torch.zeros((N, H), dtype=out.dtype)
        c = torch.zeros((N, H), dtype=torch.float64)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = xg[t, :, d].double() + product64(h, w_hh[d], mode)
            i, f, g, o = a.chunk(4, dim=1)
            c = stored(torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g), mode).double()
            h = stored(torch.sigmoid(o) * torch.tanh(c), mode)
            out[t, :, d * H:(d + 1) * H] = h
    return out


def lstm_weights(rnn):
    """(w_ih (8H, K), b (8H), w_hh (2, 4H, H)) fp32 of an nn.LSTM, as `BidirectionalLSTM._hip_weights` lays them out."""
    return (torch.cat([rnn.weight_ih_l0, rnn.weight_ih_l0_reverse]).detach().float(),
            torch.cat([rnn.bias_ih_l0 + rnn.bias_hh_l0, rnn.bias_ih_l0_reverse + rnn.bias_hh_l0_reverse]).detach().float(),
            torch.stack([rnn.weight_hh_l0, rnn.weight_hh_l0_reverse]).detach().float())


def layer64(x, weights, mode):
    """Input projection + recurrence of one layer: x (T, N, K) -> (T, N, 2H)."""
    w_ih, b, w_hh = weights
    T, N = x.shape[:2]
    return lstm64(proj64(x, w_ih, b, mode).view(T, N, 2, 4 * H), w_hh, mode)


def decoder64(decoder, feat, mode):
    """CRNNDecoder(rnn_flag=True) on (N, C, 1, W) features -> (N, W, classes) float64 logits along one route; the two
    embeddings exact (float64 products of what they read, stored fp32 between the layers in the reduced routes)."""
    x = feat[:, :, 0, :].permute(2, 0, 1).contiguous()                  # (W, N, C)
    x = x.double() if mode is None else x.float()
    for layer in decoder.decoder:
        rec = layer64(x, lstm_weights(layer.rnn), mode)
        e = layer.embedding
        y = proj64(rec.double(), e.weight.detach().float(), e.bias.detach().float(), None)
        x = stored(y, mode)
    return y.permute(1, 0, 2).contiguous()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


@functools.lru_cache(maxsize=None)
def pytorch_lstm(K):
    """The weights of nn.LSTM(K, 256, bidirectional=True) as PyTorch initialises it (seeded)."""
    torch.manual_seed(1000 + K)
    return lstm_weights(nn.LSTM(K, H, bidirectional=True))


@functools.lru_cache(maxsize=None)
def layer_case(K, T, N):
    """(x (T, N, K) fp32, {None: exact, "bf16x3": ..., torch.bfloat16: ...} (T, N, 2H)) of one layer with PyTorch-init weights."""
    x = rnd((T, N, K), 7000 + 100 * T + N + K)
    w = pytorch_lstm(K)
    return x, {m: layer64(x, w, m) for m in [None] + MODES}


def bars(kernel, refs, mode, label):
    """Prints every error with its bar and returns the list of misses [(what, error, bar)]."""
    exact, restated = refs[None], refs[mode]
    r_err = rel(restated, exact)
    e_exact = rel(kernel, exact)
    out = []
    if mode == "bf16x3":
        bar = max(2e-5, 2 * r_err)
        print(f"{label} bf16x3: kernel against exact {e_exact:.3e}, bar {bar:.3e} (restatement error {r_err:.3e})")
    else:
        bar = 2 * r_err
        e_rest = rel(kernel, restated)
        print(f"{label} bf16: kernel against exact {e_exact:.3e}, bar {bar:.3e}; against the restatement {e_rest:.3e}, "
              f"bar {0.25 * r_err:.3e} (restatement error {r_err:.3e})")
        if not e_rest <= 0.25 * r_err:
            out.append((f"{label} against the restatement", e_rest, 0.25 * r_err))
    if not e_exact <= bar:
        out.append((f"{label} against exact", e_exact, bar))
    return out


@functools.lru_cache(maxsize=None)
def golden_decoder(name):
    """{mode: float64 logits of model `name`'s decoder on its golden features} and the golden logits."""
    G = BC.golden()
    fk, lk = ("feat", "logits") if name == "crnn_tps" else ("feat32", "logits32")
    dec = BC.build_model(name).decoder
    feat = torch.from_numpy(G[fk]).float()
    with torch.no_grad():
        return {m: decoder64(dec, feat, m) for m in [None] + MODES}, torch.from_numpy(G[lk]).double()
