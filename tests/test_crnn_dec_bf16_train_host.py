"""Host side (no GPU) of CRNNDecoder's reduced-precision training graph (`set_train_compute_dtype("bf16x3")`): the argument
checks of tpspp_crnn_lstm_bf16_train_fwd, tpspp_crnn_lstm_bf16_bwd and tpspp_linear_bwd_weight_bf16 (include/tpspp.h; host
pointers: nothing is launched), the workspace query against its restated formula, the switches, and the float64
restatement of the backward (tests/crnn_dec_bf16_train_cases.py) against exact float64 autograd of nn.LSTM."""
import copy
import ctypes

import pytest
import torch

import crnn_dec_bf16_cases as DC
import crnn_dec_bf16_train_cases as TC
from tps_pp_amd import _lib, build, build_detector, ops
from tps_pp_amd.crnn import CRNNDecoder

BC = DC.BC


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def refuser(lib):
    def refused(rc, text):
        assert rc == -22 and text.encode() in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())
    return refused


def host_pointer(keep):
    return (ctypes.addressof(keep) + 15) & ~15                     # host memory, 16-byte aligned: never dereferenced


def lstm_checks(refused, call, pointers):
    for split3 in (0, 1):
        for ptr in pointers:
            refused(call(split3=split3, **{ptr: None}), "null pointer")
        for hidden in (0, 128, 255, 512):
            refused(call(split3=split3, hidden=hidden), "hidden must be 256")
        refused(call(split3=split3, T=0), "bad sizes")
        refused(call(split3=split3, N=-1), "bad sizes")
        for g in (1, 2, 3, 5, 12, 32, -4):
            refused(call(split3=split3, g=g), "images_per_group must be 0, 4, 8 or 16")
        refused(call(split3=split3, T=1 << 16, N=1 << 15), "T * N too large")
        for g in (0, 4, 8, 16):
            assert call(split3=split3, N=0, g=g) == 0               # nothing launched
    for split3 in (2, -1, 3):
        refused(call(split3=split3), "split3 must be 0 or 1")


def test_train_fwd_refuses_bad_arguments_before_any_launch(lib):
    keep = (ctypes.c_float * 80)()
    p = host_pointer(keep)
    names = ("xg", "w", "out", "gates", "cell", "T", "N", "hidden", "g", "split3", "s")
    base = dict(xg=p, w=p, out=p, gates=p, cell=p, T=3, N=2, hidden=256, g=0, split3=0, s=None)

    def call(**k):
        return lib.tpspp_crnn_lstm_bf16_train_fwd(*[{**base, **k}[n] for n in names])
    lstm_checks(refuser(lib), call, ("xg", "w", "out", "gates", "cell"))
    refuser(lib)(call(w=p + 4), "16-byte aligned")
    del keep


def test_bwd_refuses_bad_arguments_before_any_launch(lib):
    keep = (ctypes.c_float * 80)()
    p = host_pointer(keep)
    names = ("d_out", "gates", "cell", "w", "d_xg", "T", "N", "hidden", "g", "split3", "s")
    base = dict(d_out=p, gates=p, cell=p, w=p, d_xg=p, T=3, N=2, hidden=256, g=0, split3=0, s=None)

    def call(**k):
        return lib.tpspp_crnn_lstm_bf16_bwd(*[{**base, **k}[n] for n in names])
    lstm_checks(refuser(lib), call, ("d_out", "gates", "cell", "w", "d_xg"))
    refuser(lib)(call(w=p + 4), "16-byte aligned")
    del keep


def test_weight_gradient_refuses_bad_arguments_before_any_launch(lib):
    keep = (ctypes.c_float * 80)()
    p = host_pointer(keep)
    refused = refuser(lib)
    sd, sx = ops._i64(5 * 2048, 2048, 1), ops._i64(1, 512 * 27, 27)
    names = ("batch", "M", "O", "K", "DY", "sd", "X", "sx", "dW", "ws", "n", "split3", "s")
    base = dict(batch=26, M=5, O=2048, K=512, DY=p, sd=ops._vp(sd), X=p, sx=ops._vp(sx), dW=p, ws=p, n=1 << 30, split3=0, s=None)

    def wg(**k):
        return lib.tpspp_linear_bwd_weight_bf16(*[{**base, **k}[n] for n in names])

    for split3 in (0, 1):
        for ptr in ("DY", "sd", "X", "sx", "dW"):
            refused(wg(split3=split3, **{ptr: None}), "null pointer")
        for O in (64, 100, 192, 2047):
            refused(wg(split3=split3, O=O), "O and K multiples of 128")
        for K in (32, 64, 200, 513):
            refused(wg(split3=split3, K=K), "O and K multiples of 128")
        refused(wg(split3=split3, K=0), "bad sizes")
        refused(wg(split3=split3, M=-1), "bad sizes")
        refused(wg(split3=split3, batch=-1), "bad sizes")
        refused(wg(split3=split3, batch=1 << 16, M=1 << 15), "batch * M too large")
        neg = ops._i64(1, -512, 27)
        refused(wg(split3=split3, sd=ops._vp(neg)), "strides must be >= 0")
        refused(wg(split3=split3, sx=ops._vp(neg)), "strides must be >= 0")
        need = lib.tpspp_linear_bwd_weight_bf16_workspace_floats(1000, 5, 2048, 512)
        assert need > 0
        refused(wg(split3=split3, batch=1000, n=need - 1), "workspace of")
        refused(wg(split3=split3, batch=1000, n=need, ws=None), "null pointer")
    for split3 in (2, -1):
        refused(wg(split3=split3), "split3 must be 0 or 1")
    del keep


WS_CASES = [(0, 5, 128, 128), (5, 0, 2048, 512), (1, 1, 128, 128), (1, 5, 128, 256), (3, 17, 256, 128), (9, 17, 1024, 256),
            (26, 5, 2048, 512), (26, 512, 2048, 512), (26, 512, 2048, 256), (25, 512, 1024, 256), (1, 33, 128, 128),
            (4, 8, 128, 128), (1000, 5, 2048, 512), (7, 64, 4096, 2048)]


@pytest.mark.parametrize("batch,M,O,K", WS_CASES)
def test_workspace_query_against_the_restated_formula(lib, batch, M, O, K):
    got = ops.linear_bwd_weight_bf16_workspace_floats(batch, M, O, K)
    assert got == TC.wg_rows(batch, M, O, K), (batch, M, O, K)
    if batch * M == 0:
        assert got == 0
    # the split depends on the rows through batch * M alone
    assert got == ops.linear_bwd_weight_bf16_workspace_floats(1, batch * M, O, K) == \
        ops.linear_bwd_weight_bf16_workspace_floats(batch * M, 1 if batch * M else 0, O, K)


def test_decoder_train_switch_semantics():
    m = BC.build_model("crnn_tps")
    dec = m.decoder
    keys = list(m.state_dict())
    assert dec.train_lstm_dtype is None and dec.lstm_dtype is None and not hasattr(dec, "compute_dtype")
    assert dec.set_train_compute_dtype("bf16x3") is dec and dec.train_lstm_dtype == "bf16x3"
    assert dec.lstm_dtype is None and all(layer.lstm_dtype is None for layer in dec.decoder)
    assert list(m.state_dict()) == keys and not hasattr(dec, "compute_dtype")
    for bad in (torch.bfloat16, "bf16", 1):
        with pytest.raises(ValueError, match="set_train_compute_dtype"):
            dec.set_train_compute_dtype(bad)
        assert dec.train_lstm_dtype == "bf16x3"                     # a call that fails changes nothing
    with pytest.raises(ValueError, match="follow-up"):
        dec.set_train_compute_dtype(torch.bfloat16)
    assert dec.set_train_compute_dtype(None).train_lstm_dtype is None
    # neither switch touches the other
    dec.set_compute_dtype(torch.bfloat16)
    assert dec.train_lstm_dtype is None
    dec.set_train_compute_dtype("bf16x3")
    assert dec.lstm_dtype == torch.bfloat16
    m.set_compute_dtype(None, decoder=None)
    assert dec.train_lstm_dtype == "bf16x3"
    # the recogniser's pass-through
    assert m.set_train_compute_dtype() is m and dec.train_lstm_dtype is None
    assert m.set_train_compute_dtype(decoder="bf16x3") is m and dec.train_lstm_dtype == "bf16x3"
    with pytest.raises(ValueError, match="set_train_compute_dtype"):
        m.set_train_compute_dtype(decoder=torch.bfloat16)
    assert dec.train_lstm_dtype == "bf16x3"
    # the train backend's signature and behaviour stay
    assert m.set_train_backend("torch", decoder="hip", loss="hip") is m and dec.train_backend == "hip"
    assert dec.train_lstm_dtype == "bf16x3"
    with pytest.raises(ValueError):
        m.set_train_backend("torch", backbone="hip")
    assert list(m.state_dict()) == keys
    assert not any("train_lstm_dtype" in k for k in m.state_dict())
    assert len(list(m.parameters())) == len(list(BC.build_model("crnn_tps").parameters()))
    flat = CRNNDecoder(in_channels=512, num_classes=37, rnn_flag=False)
    assert flat.set_train_compute_dtype("bf16x3").train_lstm_dtype == "bf16x3"


def test_a_recogniser_whose_decoder_has_no_training_switch_raises_naming_it():
    m = build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                       strides=[2, 1, 2, 1, 2]),
                            tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                            decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                            label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True), max_seq_len=8))
    with pytest.raises(ValueError, match=type(m.decoder).__name__):
        m.set_train_compute_dtype(decoder="bf16x3")
    with pytest.raises(ValueError, match=type(m.decoder).__name__):
        m.set_train_compute_dtype()
    assert not hasattr(m.decoder, "train_lstm_dtype")


def test_a_host_batch_with_the_mode_set_still_trains_through_pytorch():
    dec = BC.build_model("crnn").decoder
    dec.set_train_backend("hip").set_train_compute_dtype("bf16x3")
    twin = copy.deepcopy(dec).set_train_compute_dtype(None)
    feat = torch.from_numpy(BC.golden()["feat32"]).float()
    dec.train()
    twin.train()
    got = dec(feat.clone().requires_grad_(True), None, None, None, train_mode=True)
    want = twin._forward_torch(feat.clone().requires_grad_(True))
    assert got.grad_fn is not None and torch.equal(got.detach().view(torch.int32), want.detach().view(torch.int32))
    got.square().mean().backward()
    want.square().mean().backward()
    for (n, a), (_, b) in zip(dec.named_parameters(), twin.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), n
    with pytest.raises(ValueError, match="mode"):                   # the op refuses what the switch refuses
        ops.crnn_bilstm_autograd(torch.zeros(2, 1, 256), (2, 1, 256, 256, 1), 2, 1, torch.nn.LSTM(256, 256, bidirectional=True),
                                 mode=torch.bfloat16)


@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("T", [1, 2, 26])
def test_the_restatement_against_float64_autograd(K, T):
    N = 5 if T < 26 else 3
    x, d_out, grads, restated_exact = TC.layer_case(K, T, N)
    for key in TC.GRAD_KEYS:                                         # the exact route of the restatement IS nn.LSTM's autograd
        e = DC.rel(restated_exact[key], grads[None][key])
        print(f"K={K} T={T} N={N} {key}: exact restatement against float64 autograd {e:.3e}")
        assert e <= 1e-12, (key, e)
    for mode, mid in zip(DC.MODES, DC.MODE_IDS):
        for key in ("d_xg",) + TC.GRAD_KEYS:
            e = DC.rel(grads[mode][key], grads[None][key])
            print(f"K={K} T={T} N={N} {key}: {mid} restatement error {e:.3e}")
            assert e <= (2e-5 if mode == "bf16x3" else 2e-2), (mid, key, e)            # 2e-5: the x3 bar of DC.bars
