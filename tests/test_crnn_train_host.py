"""Host side (no GPU) of the CRNN decoder's and the CTC loss's HIP training paths: the argument checks of the entry points of
include/tpspp_crnn_train.h (host pointers: nothing is launched), the workspace query restated, the backend switch, and the
gradient formula the CTC kernels implement restated in float64 against autograd."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import crnn_train_cases as TC
import tps_pp_amd
from tps_pp_amd import _lib, build, build_detector

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import crnn_cases as CC  # noqa: E402

TOL = 1e-6


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "crnn_tps.npz"))


# ---- the entry points of include/tpspp_crnn_train.h ----------------------------------------------------------------------
def host(n, ctype=ctypes.c_float):
    buf = (ctype * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def test_every_entry_point_refuses_bad_arguments_before_any_launch(lib):
    keep, p = host(64)

    def refused(rc, text):
        assert rc == -22 and text.encode() in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())

    def caller(fn, names, **defaults):
        return lambda **k: fn(*[{**defaults, **k}[n] for n in names])

    fwd = caller(lib.tpspp_crnn_lstm_train_fwd, ("xg", "w", "out", "gates", "cell", "T", "N", "hidden", "g", "s"),
                 xg=p, w=p, out=p, gates=p, cell=p, T=2, N=1, hidden=256, g=0, s=None)
    bwd = caller(lib.tpspp_crnn_lstm_bwd, ("d_out", "gates", "cell", "wt", "d_xg", "dir", "T", "N", "hidden", "g", "s"),
                 d_out=p, gates=p, cell=p, wt=p, d_xg=p, dir=p, T=2, N=1, hidden=256, g=0, s=None)
    for call, ptrs in ((fwd, ("xg", "w", "out", "gates", "cell")), (bwd, ("d_out", "gates", "cell", "wt", "d_xg"))):
        for name in ptrs:
            refused(call(**{name: None}), "null pointer")
        refused(call(hidden=128), "hidden must be 256")
        refused(call(hidden=512), "hidden must be 256")
        refused(call(T=0), "T >= 1")
        refused(call(N=-1), "bad sizes")
        for g in (1, 2, 3, 5, 12, 32, -4):
            refused(call(g=g), "images_per_group must be 0, 4, 8 or 16")
        assert call(N=0) == 0 and all(call(N=0, g=g) == 0 for g in (4, 8, 16))
    assert bwd(N=0, dir=None) == 0                                  # the direction-major copy is optional

    need = lib.tpspp_crnn_ctc_loss_workspace_floats(1, 3, 2)
    cf = caller(lib.tpspp_crnn_ctc_loss_fwd, ("lg", "tg", "tl", "il", "N", "T", "C", "Lmax", "blank", "zi", "red", "loss", "lse",
                                              "reduced", "ws", "wsn", "s"),
                lg=p, tg=p, tl=p, il=p, N=1, T=3, C=5, Lmax=2, blank=0, zi=0, red=1, loss=p, lse=p, reduced=p, ws=p, wsn=need,
                s=None)
    cb = caller(lib.tpspp_crnn_ctc_loss_bwd, ("g", "lg", "tg", "tl", "il", "lse", "ws", "N", "T", "C", "Lmax", "blank", "zi", "red",
                                              "d", "s"),
                g=p, lg=p, tg=p, tl=p, il=p, lse=p, ws=p, N=1, T=3, C=5, Lmax=2, blank=0, zi=0, red=1, d=p, s=None)
    for call, ptrs in ((cf, ("lg", "tg", "tl", "il", "loss", "lse", "reduced", "ws")), (cb, ("g", "lg", "tg", "tl", "il", "lse", "ws", "d"))):
        for name in ptrs:
            refused(call(**{name: None}), "null pointer")
        refused(call(C=1), "C must lie in [2, 1024]")
        refused(call(C=1025), "C must lie in [2, 1024]")
        refused(call(blank=5), "blank 5 out of range")
        refused(call(blank=-1), "out of range")
        refused(call(T=0), "T >= 1")
        refused(call(N=-1), "bad sizes")
        refused(call(Lmax=-1), "Lmax must lie in [0, 1024]")
        refused(call(Lmax=1025), "Lmax must lie in [0, 1024]")
        refused(call(red=3), "reduction must be")
        assert call(N=0) == 0
        assert call(N=0, Lmax=0, tg=None) == 0                     # no target position: the targets are never read
    refused(cf(wsn=need - 1), "workspace of")
    assert cf(N=0, red=0, reduced=None) == 0                        # no reduction: no reduced value
    del keep


# (N, T, Lmax) -> floats: the alpha table of N * T * (2 Lmax + 1), then one loss per image
WS_CASES = [((1, 1, 0), 2), ((1, 3, 2), 16), ((3, 26, 8), 3 * 26 * 17 + 3), ((512, 26, 25), 512 * 26 * 51 + 512),
            ((2, 40, 35), 2 * 40 * 71 + 2), ((4, 12, 0), 52), ((0, 26, 8), 0), ((3, 0, 8), 0), ((3, 26, -1), 0), ((-1, 26, 8), 0)]


def test_ctc_workspace_query_follows_its_case_table(lib):
    from tps_pp_amd import ops
    for (N, T, Lmax), want in WS_CASES:
        restated = N * T * (2 * Lmax + 1) + N if N > 0 and T > 0 and Lmax >= 0 else 0
        assert restated == want, (N, T, Lmax)
        assert lib.tpspp_crnn_ctc_loss_workspace_floats(N, T, Lmax) == want, (N, T, Lmax)
        assert ops.crnn_ctc_loss_workspace_floats(N, T, Lmax) == want


# ---- the switch ----------------------------------------------------------------------------------------------------------
def build_model(name):
    m = build_detector(CC.models()[name]).eval()
    sd = CC.state(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


def test_backend_switch_defaults_and_errors():
    from tps_pp_amd.losses import CTCLoss
    m = build_model("crnn_tps")
    keys = list(m.state_dict())
    assert isinstance(m.loss, CTCLoss) and m.decoder.train_backend == "torch" and m.loss.train_backend == "torch"
    for part in (m.decoder, m.loss):
        with pytest.raises(ValueError, match="set_train_backend"):
            part.set_train_backend("cuda")
        assert part.train_backend == "torch"
    with pytest.raises(ValueError, match="decoder must be"):
        m.set_train_backend("torch", decoder="fast", loss="hip")
    assert m.decoder.train_backend == "torch" and m.loss.train_backend == "torch"       # a failed call changes nothing
    with pytest.raises(ValueError, match="no HIP training path"):
        m.set_train_backend("torch", backbone="hip")                                    # the VGG keeps training on PyTorch
    assert m.set_train_backend("torch", decoder="hip", loss="hip") is m
    assert m.decoder.train_backend == "hip" and m.loss.train_backend == "hip"
    assert list(m.state_dict()) == keys and not any("backend" in k for k in keys)
    assert m.decoder.set_train_backend("torch") is m.decoder and m.decoder.train_backend == "torch"
    assert tps_pp_amd.build_decoder(dict(type="CRNNDecoder", in_channels=512, num_classes=37)).train_backend == "torch"


def test_host_batch_still_trains_through_pytorch_with_hip_set(G):
    m = build_model("crnn_tps")
    m.set_train_backend("torch", decoder="hip", loss="hip")
    lg = torch.from_numpy(G["logits"]).clone().requires_grad_(True)
    loss = m.loss(lg, m.label_convertor.str2tensor(CC.TEXTS), CC.img_metas(CC.N))["loss_ctc"]
    loss.backward()
    assert abs(loss.item() - G["loss"].reshape(-1)[0].item()) <= TOL
    assert np.abs(lg.grad.numpy() - G["loss_grad"]).max() <= TOL
    m.decoder.train()
    feat = torch.from_numpy(G["feat"]).requires_grad_(True)
    out = m.decoder(feat, None, None, None, train_mode=True)
    assert out.grad_fn is not None and np.abs(out.detach().numpy() - G["logits"]).max() <= TOL
    out.sum().backward()
    assert feat.grad is not None and all(p.grad is not None for p in m.decoder.parameters())


def test_hip_ops_refuse_host_tensors_and_bad_targets():
    from tps_pp_amd import ops
    logits, padded, tl, il = TC.ctc_case("hello")
    with pytest.raises(_lib.TpsppError, match="GPU tensor"):
        ops.crnn_ctc_loss_autograd(logits, padded, tl, il)
    with pytest.raises(_lib.TpsppError, match="GPU tensor"):
        ops.crnn_lstm_train_fwd(torch.zeros(1, 1, 2, 1024), torch.zeros(2, 1024, 256))
    with pytest.raises(_lib.TpsppError, match="GPU tensor"):
        ops.crnn_bilstm_autograd(torch.zeros(2, 1, 256), (2, 1, 256, 256, 1), 2, 1, torch.nn.LSTM(256, 256, bidirectional=True))
    for bad in (TC.BLANK, 37, -1):                                  # refused where the targets originate, before the device check
        t = padded.clone()
        t[0, 2] = bad
        with pytest.raises(ValueError, match="position 2"):
            ops.crnn_ctc_loss_autograd(logits, t, tl, il)
    with pytest.raises(ValueError, match="reduction"):
        ops.crnn_ctc_loss_autograd(logits, padded, tl, il, reduction="batchmean")


# ---- the formula -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.CTC_CASES))
def test_ctc_cases_are_feasible_and_the_fused_formula_equals_autograd(name):
    logits, padded, tl, il = TC.ctc_case(name)
    for n in range(len(tl)):
        assert TC.feasible(padded[n, :tl[n]].tolist(), int(il[n])), (name, n)
    x = logits.double().requires_grad_(True)
    want = TC.ctc_torch(x, padded, tl, il)
    assert torch.isfinite(want).all()
    want.sum().backward()
    loss, grad = TC.ctc_formula64(logits, padded, tl, il)
    e_loss, e_grad = (loss - want.detach()).abs().max().item(), (grad - x.grad).abs().max().item()
    print(f"ctc formula {name}: loss error {e_loss:.3e}, gradient error {e_grad:.3e} (bar 1e-12)")
    assert e_loss <= 1e-12 * max(1.0, want.abs().max().item()) and e_grad <= 1e-12
    rows = torch.arange(logits.shape[1])[None, :] >= il[:, None]
    assert not grad[rows].any() and not x.grad[rows].any()          # PyTorch's rows past the input length are zeros


def test_the_infeasible_image_is_infeasible_and_pytorchs_mean_rule():
    target, input_len = TC.INFEASIBLE
    assert not TC.feasible(target, input_len)
    logits, padded, tl, il = TC.ctc_case("mixed", extra=TC.INFEASIBLE)
    x = logits.double()
    per = TC.ctc_torch(x, padded, tl, il)
    assert torch.isinf(per[1]) and torch.isfinite(per[[0, 2, 3, 4]]).all()
    assert TC.ctc_formula64(logits, padded, tl, il)[0][1] == np.inf
    zi = TC.ctc_torch(x, padded, tl, il, zero_infinity=True)
    assert zi[1] == 0 and torch.equal(zi[[0, 2, 3, 4]], per[[0, 2, 3, 4]])
    mean = TC.ctc_torch(x, padded, tl, il, reduction="mean", zero_infinity=True)
    assert abs(mean.item() - (zi / tl.clamp(min=1)).mean().item()) <= 1e-12
