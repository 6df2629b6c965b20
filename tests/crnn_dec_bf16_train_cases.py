"""The backward of CRNNDecoder's reduced-precision training graph restated on the CPU in float64, shared by
tests/test_crnn_dec_bf16_train_host.py and tests/test_gpu_crnn_dec_bf16_train.py (a helper module, not a test file).  It
extends tests/crnn_dec_bf16_cases.py (`DC`): the same three routes -- None exact float64, "bf16x3" every operand of a wide
product split (`DC.split`) with the terms hi*hi + lo*hi + hi*lo, torch.bfloat16 both operands rounded (`DC.product64`) --
now over the five wide products of a layer's training step: the input projection, the recurrence forward, the recurrence
backward (da W_hh), d w_ih / d w_hh (both operands are activations) and dx.  In the reduced routes a value is rounded to
fp32 (`DC.stored`) exactly where the kernels store it: xg, the gates after their activations, the cell, h, d_xg, dh_rec and
dc; the bias gradient, the embeddings and the loss are exact products and sums of the fp32 values they read.

The bars are `DC.bars`, unchanged, on every gradient tensor with refs = {None: exact, mode: restatement}: for bf16x3
rel(kernel, exact) <= max(2e-5, 2 x restatement error).  A CPU emulation with fp32-accumulated products (K in {256, 512},
(T, N) in {(1, 1), (2, 5), (9, 5), (26, 5), (26, 17)}, PyTorch-init weights) put d_xg, dx, d w_ih and d w_hh at 1.3-6.1e-6
from exact.  Plain bf16 is held at the kernel level only, on identical stored inputs (no chain of flipped roundings builds
up there): over a T = 26 layer the same emulation sits 3.6e-4 from the restatement against a 0.25 x bar of 6.4e-4, under a
factor of two, which is why the module switch refuses it.  References are cached: each is computed once and shared."""
import functools

import torch
import torch.nn as nn

import crnn_dec_bf16_cases as DC

H = DC.H
ROUTES = [None, "bf16x3", torch.bfloat16]


def as_route(x, mode):
    return x.double() if mode is None else x.float()


def train_fwd64(xg, w_hh, mode):
    """The saving recurrence: xg (T, N, 2, 4H), w_hh (2, 4H, H) -> (out (T, N, 2H), gates (T, N, 2, 4H) after their
    activations, cell (T, N, 2, H)), each as the route stores it."""
    T, N = xg.shape[:2]
    dt = torch.float64 if mode is None else torch.float32
    out, gates, cell = torch.zeros((T, N, 2 * H), dtype=dt), torch.zeros((T, N, 2, 4 * H), dtype=dt), torch.zeros((T, N, 2, H), dtype=dt)
    for d in range(2):
        h = torch.zeros((N, H), dtype=dt)
        c = torch.zeros((N, H), dtype=torch.float64)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            a = xg[t, :, d].double() + DC.product64(h, w_hh[d], mode)
            i, f, g, o = a.chunk(4, dim=1)
            act = DC.stored(torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], 1), mode)
            i, f, g, o = act.double().chunk(4, dim=1)
            c = DC.stored(f * c + i * g, mode).double()
            h = DC.stored(o * torch.tanh(c), mode)
            out[t, :, d * H:(d + 1) * H], gates[t, :, d], cell[t, :, d] = h, act, c
    return out, gates, cell


def bwd64(d_out, gates, cell, w_hh, mode):
    """The backward through time (include/tpspp_crnn_train.h:43-47) -> d_xg (T, N, 2, 4H); da W_hh along the route, d_xg,
    dh_rec and dc stored fp32 in the reduced routes."""
    T, N = gates.shape[:2]
    d_xg = torch.zeros((T, N, 2, 4 * H), dtype=torch.float64 if mode is None else torch.float32)
    for d in range(2):
        dc = torch.zeros((N, H), dtype=torch.float64)
        dhr = torch.zeros((N, H), dtype=torch.float64)
        order = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        for s, t in enumerate(order):
            more = s + 1 < T
            i, f, g, o = gates[t, :, d].double().chunk(4, dim=1)
            c = cell[t, :, d].double()
            cprev = cell[order[s + 1], :, d].double() if more else torch.zeros_like(c)
            dh = d_out[t, :, d * H:(d + 1) * H].double() + dhr
            tc = torch.tanh(c)
            dcv = dc + dh * o * (1 - tc * tc)
            da = torch.cat([dcv * g * i * (1 - i), dcv * cprev * f * (1 - f), dcv * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            da = DC.stored(da, mode)
            d_xg[t, :, d] = da
            dc = DC.stored(dcv * f, mode).double()
            if more:
                dhr = DC.stored(DC.product64(da, w_hh[d].t(), mode), mode).double()
    return d_xg


def dweight64(dy, x, mode):
    """dW (O, K) = dy (R, O)^T x (R, K): `DC.product64` of the transposes."""
    return DC.product64(dy.t(), x.t(), mode)


def layer_fwd64(x, weights, mode):
    w_ih, b, w_hh = weights
    T, N = x.shape[:2]
    xg = DC.proj64(as_route(x, mode), w_ih, b, mode).view(T, N, 2, 4 * H)
    return train_fwd64(xg, w_hh, mode)


def layer_bwd64(x, weights, saved, d_out, mode):
    """One layer's backward along a route -> {"d_xg", "dx", "dw_ih" (8H, K), "dw_hh" (2, 4H, H), "db" (8H)}."""
    w_ih, b, w_hh = weights
    out, gates, cell = saved
    T, N, K = x.shape
    d_xg = bwd64(as_route(d_out, mode), gates, cell, w_hh, mode)
    dy, x2 = d_xg.reshape(T * N, 8 * H), as_route(x, mode).reshape(T * N, K)
    g = {"d_xg": d_xg, "dw_ih": dweight64(dy, x2, mode), "db": dy.double().sum(0),
         "dx": DC.stored(DC.product64(dy, w_ih.t(), mode), mode).reshape(T, N, K)}
    if T > 1:
        g["dw_hh"] = torch.stack([dweight64(d_xg[1:, :, 0].reshape(-1, 4 * H), out[:-1, :, :H].reshape(-1, H), mode),
                                  dweight64(d_xg[:-1, :, 1].reshape(-1, 4 * H), out[1:, :, H:].reshape(-1, H), mode)])
    else:
        g["dw_hh"] = torch.zeros((2, 4 * H, H), dtype=torch.float64)
    return g


def lstm_module64(weights):
    """nn.LSTM in float64 carrying `weights` (b_ih = b, b_hh = 0: both receive db)."""
    w_ih, b, w_hh = weights
    m = nn.LSTM(w_ih.shape[1], H, bidirectional=True).double()
    with torch.no_grad():
        for sfx, d in (("", 0), ("_reverse", 1)):
            getattr(m, "weight_ih_l0" + sfx).copy_(w_ih[4 * H * d:4 * H * (d + 1)])
            getattr(m, "weight_hh_l0" + sfx).copy_(w_hh[d])
            getattr(m, "bias_ih_l0" + sfx).copy_(b[4 * H * d:4 * H * (d + 1)])
            getattr(m, "bias_hh_l0" + sfx).zero_()
    return m


def autograd64(x, weights, d_out):
    """Exact float64 autograd of nn.LSTM -> (out, {"dx", "dw_ih", "dw_hh", "db"})."""
    m = lstm_module64(weights)
    xr = x.double().clone().requires_grad_(True)
    out, _ = m(xr)
    out.backward(d_out.double())
    return out.detach(), {"dx": xr.grad, "dw_ih": torch.cat([m.weight_ih_l0.grad, m.weight_ih_l0_reverse.grad]),
                          "dw_hh": torch.stack([m.weight_hh_l0.grad, m.weight_hh_l0_reverse.grad]),
                          "db": torch.cat([m.bias_ih_l0.grad, m.bias_ih_l0_reverse.grad])}


@functools.lru_cache(maxsize=None)
def rec_case(T, N):
    """Stored inputs of the recurrence kernels, identical for every route: (xg, w_hh, d_out, {mode: (out, gates, cell)},
    {mode: d_xg}); the backward of each route reads that route's own stored gates and cell."""
    xg = DC.rnd((T, N, 2, 4 * H), 8100 + 10 * T + N, 2.0)
    w_hh = DC.pytorch_lstm(256)[2]
    d_out = DC.rnd((T, N, 2 * H), 8200 + 10 * T + N)
    fwd = {m: train_fwd64(as_route(xg, m), w_hh, m) for m in ROUTES}
    return xg, w_hh, d_out, fwd


@functools.lru_cache(maxsize=None)
def bwd_case(T, N, mode):
    """(d_out, gates, cell, w_hh, {None: exact, mode: restatement} of d_xg): the backward kernel's stored fp32 inputs --
    the gates and cell of the route's own restated forward -- and both references on exactly those inputs."""
    _, w_hh, d_out, fwd = rec_case(T, N)
    _, gates, cell = fwd[mode]
    return d_out, gates, cell, w_hh, {m: bwd64(as_route(d_out, m), gates, cell, w_hh, m) for m in (None, mode)}


@functools.lru_cache(maxsize=None)
def layer_case(K, T, N):
    """(x, d_out, {route: gradient dict}) of one layer with PyTorch-init weights; route None is float64 autograd of nn.LSTM
    (its d_xg comes from the exact restatement)."""
    x = DC.rnd((T, N, K), 7000 + 100 * T + N + K)
    d_out = DC.rnd((T, N, 2 * H), 7500 + 100 * T + N + K)
    w = DC.pytorch_lstm(K)
    grads = {}
    for m in ROUTES:
        grads[m] = layer_bwd64(x, w, layer_fwd64(x, w, m), d_out, m)
    _, exact = autograd64(x, w, d_out)
    restated_exact = grads[None]
    grads[None] = dict(exact, d_xg=restated_exact["d_xg"])
    return x, d_out, grads, restated_exact


GRAD_KEYS = ("dx", "dw_ih", "dw_hh", "db")


# ---- the decoder: two layers, two embeddings and the CTC loss ------------------------------------------------------------------
def loss_grad64(logits, loss_fn):
    """(loss, d loss / d logits) in float64 of `loss_fn` (logits (N, W, classes) float64 -> scalar), e.g. the CTCLoss module."""
    lg = logits.double().clone().requires_grad_(True)
    loss = loss_fn(lg)
    loss.backward()
    return loss.detach(), lg.grad


def decoder_grads64(decoder, feat, loss_fn, mode):
    """CRNNDecoder(rnn_flag=True) + CTC loss along one route -> (loss, {parameter name: gradient}) in float64: the two layers
    through `layer_fwd64` / `layer_bwd64`, the embeddings and the loss exact on what they read."""
    x0 = feat[:, :, 0, :].permute(2, 0, 1).contiguous()                 # (W, N, C)
    xs, saved, recs = [], [], []
    x = as_route(x0, mode)
    for layer in decoder.decoder:
        w = DC.lstm_weights(layer.rnn)
        xs.append(x)
        sv = layer_fwd64(x, w, mode)
        saved.append(sv)
        e = layer.embedding
        y = DC.proj64(sv[0].double(), e.weight.detach().float(), e.bias.detach().float(), None)
        recs.append(sv[0])
        x = DC.stored(y, mode)
    loss, d_logits = loss_grad64(x.permute(1, 0, 2).contiguous(), loss_fn)
    dy = DC.stored(d_logits.permute(1, 0, 2).contiguous(), mode)        # (W, N, classes)
    grads = {}
    for li in (1, 0):
        layer = decoder.decoder[li]
        e = layer.embedding
        T, N = dy.shape[:2]
        d2, r2 = dy.reshape(T * N, -1).double(), recs[li].reshape(T * N, 2 * H).double()
        grads[f"decoder.{li}.embedding.weight"] = d2.t() @ r2
        grads[f"decoder.{li}.embedding.bias"] = d2.sum(0)
        d_rec = DC.stored((d2 @ e.weight.detach().double()).reshape(T, N, 2 * H), mode)
        g = layer_bwd64(xs[li], DC.lstm_weights(layer.rnn), saved[li], d_rec, mode)
        for sfx, d in (("", 0), ("_reverse", 1)):
            grads[f"decoder.{li}.rnn.weight_ih_l0{sfx}"] = g["dw_ih"][4 * H * d:4 * H * (d + 1)]
            grads[f"decoder.{li}.rnn.weight_hh_l0{sfx}"] = g["dw_hh"][d]
            grads[f"decoder.{li}.rnn.bias_ih_l0{sfx}"] = g["db"][4 * H * d:4 * H * (d + 1)]
            grads[f"decoder.{li}.rnn.bias_hh_l0{sfx}"] = g["db"][4 * H * d:4 * H * (d + 1)]
        dy = g["dx"]
    return loss, grads


def wg_rows(batch, M, O, K):
    """The fixed split of tpspp_linear_bwd_weight_bf16 restated (include/tpspp.h) -> workspace floats."""
    R = batch * M
    if R <= 0:
        return 0
    steps = (R + 31) // 32
    tiles = (O // 128) * (K // 128)
    per = -(-steps // max(1, 512 // tiles))
    slices = -(-steps // per)
    return slices * O * K if slices > 1 else 0
