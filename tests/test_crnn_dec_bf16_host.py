"""Host side (no GPU) of CRNNDecoder's reduced-precision modes: the argument checks of tpspp_crnn_lstm_bf16_fwd and
tpspp_mm_bf16 (include/tpspp.h; host pointers: nothing is launched), the arranged weight layout, the switches, and the
arithmetic of the two modes restated in float64 (tests/crnn_dec_bf16_cases.py) on the golden features: the three-term split
must reach the module's 1e-4 bar by its arithmetic alone, and both modes must leave every arg-max of the golden logits where
it is."""
import copy
import ctypes

import pytest
import torch

import crnn_dec_bf16_cases as DC
from tps_pp_amd import _lib, build, build_detector, ops
from tps_pp_amd.crnn import BidirectionalLSTM, CRNNDecoder

BC, CC = DC.BC, DC.CC


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def refuser(lib):
    def refused(rc, text):
        assert rc == -22 and text.encode() in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())
    return refused


def test_lstm_bf16_refuses_bad_arguments_before_any_launch(lib):
    keep = (ctypes.c_float * 80)()
    p = (ctypes.addressof(keep) + 15) & ~15                        # host memory, 16-byte aligned: never dereferenced
    refused = refuser(lib)
    names = ("xg", "w", "out", "T", "N", "hidden", "g", "split3", "s")
    base = dict(xg=p, w=p, out=p, T=3, N=2, hidden=256, g=0, split3=0, s=None)

    def lstm(**k):
        return lib.tpspp_crnn_lstm_bf16_fwd(*[{**base, **k}[n] for n in names])

    for split3 in (0, 1):
        for ptr in ("xg", "w", "out"):
            refused(lstm(split3=split3, **{ptr: None}), "null pointer")
        refused(lstm(split3=split3, w=p + 4), "16-byte aligned")
        for hidden in (0, 128, 255, 512):
            refused(lstm(split3=split3, hidden=hidden), "hidden must be 256")
        refused(lstm(split3=split3, T=0), "bad sizes")
        refused(lstm(split3=split3, N=-1), "bad sizes")
        for g in (1, 2, 3, 5, 12, 32, -4):
            refused(lstm(split3=split3, g=g), "images_per_group must be 0, 4, 8 or 16")
        refused(lstm(split3=split3, T=1 << 16, N=1 << 15), "T * N too large")
        for g in (0, 4, 8, 16):
            assert lstm(split3=split3, N=0, g=g) == 0               # nothing launched
    for split3 in (2, -1, 3):
        refused(lstm(split3=split3), "split3 must be 0 or 1")
    del keep


def test_mm_bf16_refuses_bad_arguments_before_any_launch(lib):
    keep = (ctypes.c_float * 80)()
    p = (ctypes.addressof(keep) + 15) & ~15
    refused = refuser(lib)
    sa, sc = ops._i64(512 * 4, 512, 1), ops._i64(4 * 2048, 2048, 1)
    names = ("batch", "M", "N", "K", "A", "sa", "B", "C", "sc", "bias", "split3", "s")
    base = dict(batch=3, M=4, N=2048, K=512, A=p, sa=ops._vp(sa), B=p, C=p, sc=ops._vp(sc), bias=None, split3=0, s=None)

    def mm(**k):
        return lib.tpspp_mm_bf16(*[{**base, **k}[n] for n in names])

    for split3 in (0, 1):
        for ptr in ("A", "sa", "B", "C", "sc"):
            refused(mm(split3=split3, **{ptr: None}), "null pointer")
        refused(mm(split3=split3, B=p + 4), "16-byte aligned")
        for K in (16, 48, 500, 513):
            refused(mm(split3=split3, K=K), "K a multiple of 32")
        for N in (64, 100, 192, 2047):
            refused(mm(split3=split3, N=N), "N a multiple of 128")
        refused(mm(split3=split3, K=0), "bad sizes")
        refused(mm(split3=split3, M=-1), "bad sizes")
        refused(mm(split3=split3, batch=-1), "bad sizes")
        refused(mm(split3=split3, batch=1 << 16, M=1 << 15), "batch * M too large")
        neg = ops._i64(1, -512, 27)
        refused(mm(split3=split3, sa=ops._vp(neg)), "strides must be >= 0")
        refused(mm(split3=split3, sc=ops._vp(neg)), "strides must be >= 0")
        assert mm(split3=split3, batch=0) == 0 and mm(split3=split3, M=0) == 0 and mm(split3=split3, N=0) == 0
    for split3 in (2, -1):
        refused(mm(split3=split3), "split3 must be 0 or 1")
    del keep


@pytest.mark.parametrize("shape", [(1024 * 2, 512), (2, 1024, 256), (128, 32)])
def test_arranged_weights_dearrange_exactly(shape):
    w = DC.rnd(shape, 5 + len(shape), 0.1)
    rows, K = shape[-2:]
    for x3 in (False, True):
        mw = ops.arrange_mfma16(w, x3=x3)
        assert mw.arranged.dtype == torch.bfloat16 and (mw.rows, mw.k, mw.x3) == (rows, K, x3)
        assert tuple(mw.arranged.shape) == shape[:-2] + (2 if x3 else 1, rows // 16, K // 32, 64, 8)
        back = ops.dearrange_mfma16(mw)
        want = torch.stack(ops._hi_lo(w) if x3 else (w.to(torch.bfloat16),), dim=-3)
        assert torch.equal(back.view(torch.int16), want.view(torch.int16))
        if x3:                                                      # the helper's rule is ops._hi_lo's
            hi, lo = DC.split(w)
            assert torch.equal(back.select(-3, 0).float(), hi) and torch.equal(back.select(-3, 1).float(), lo)
    # the documented lane map, element by element on one tile: lane l of tile (ct, ks) holds W[16 ct + (l & 15)][32 ks + 8 (l >> 4) + j]
    w2 = w.reshape(-1, rows, K)[0]
    a = ops.arrange_mfma16(w2).arranged[0]
    for ct, ks, lane, j in ((0, 0, 0, 0), (rows // 16 - 1, K // 32 - 1, 63, 7), (1, 0, 17, 3), (2, 0, 40, 5)):
        assert a[ct, ks, lane, j] == w2[16 * ct + (lane & 15), 32 * ks + 8 * (lane >> 4) + j].to(torch.bfloat16)
    for bad in ((8, 32), (16, 16), (3, 16, 48), (16,)):
        with pytest.raises(ValueError, match="arrange_mfma16"):
            ops.arrange_mfma16(torch.zeros(bad))


def test_decoder_switch_semantics(monkeypatch):
    monkeypatch.setenv("TPSPP_COMPUTE_DTYPE", "bf16x3")             # no environment variable reaches the decoder
    m = BC.build_model("crnn_tps")
    dec = m.decoder
    keys = list(m.state_dict())
    assert dec.lstm_dtype is None and not hasattr(dec, "compute_dtype")
    for mode in ("bf16x3", torch.bfloat16, None):
        assert dec.set_compute_dtype(mode) is dec and dec.lstm_dtype == mode
        assert all(layer.lstm_dtype == mode for layer in dec.decoder)
        assert list(m.state_dict()) == keys and not hasattr(dec, "compute_dtype")
    for bad in ("fp16", "bf16", torch.float16, torch.float32, 0):
        with pytest.raises(ValueError, match="set_compute_dtype"):
            dec.set_compute_dtype(bad)
    assert dec.lstm_dtype is None
    # the recogniser's switch without the keyword: exactly as before, the decoder stays where it is
    for mode in ("bf16x3", torch.bfloat16, None):
        assert m.set_compute_dtype(mode) is m and m.backbone.compute_dtype == mode and dec.lstm_dtype is None
    dec.set_compute_dtype("bf16x3")
    m.set_compute_dtype(None)
    assert dec.lstm_dtype == "bf16x3"                               # ... in either direction
    # with the keyword: the decoder follows it, independently of the other stages
    for mode, d in (("bf16x3", "bf16x3"), (torch.bfloat16, torch.bfloat16), (None, torch.bfloat16), ("bf16x3", None)):
        assert m.set_compute_dtype(mode, decoder=d) is m
        assert m.backbone.compute_dtype == mode and dec.lstm_dtype == d
    with pytest.raises(ValueError, match="decoder"):
        m.set_compute_dtype(torch.bfloat16, decoder="fp16")
    assert m.backbone.compute_dtype == "bf16x3" and dec.lstm_dtype is None      # a call that fails changes nothing
    assert list(m.state_dict()) == keys
    # rnn_flag=False has the switch and nothing to set
    flat = CRNNDecoder(in_channels=512, num_classes=37, rnn_flag=False)
    assert flat.set_compute_dtype(torch.bfloat16).lstm_dtype == torch.bfloat16


def test_a_recogniser_whose_decoder_has_no_switch_raises_naming_it():
    m = build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                       strides=[2, 1, 2, 1, 2]),
                            tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                            decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                            label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True), max_seq_len=8))
    before = m.backbone.compute_dtype
    with pytest.raises(ValueError, match=type(m.decoder).__name__):
        m.set_compute_dtype("bf16x3", decoder="bf16x3")
    assert m.backbone.compute_dtype == before
    assert m.set_compute_dtype("bf16x3") is m                       # without the keyword it works as it always did


@pytest.mark.parametrize("mode", DC.MODES, ids=DC.MODE_IDS)
def test_train_mode_and_host_tensors_take_the_pytorch_composition(mode):
    dec = BC.build_model("crnn").decoder.set_compute_dtype(mode)
    feat = torch.from_numpy(BC.golden()["feat32"]).float()
    twin = copy.deepcopy(dec).set_compute_dtype(None)
    with torch.no_grad():
        want = twin.train()._forward_torch(feat)
        got = dec.train()(feat, None, None, None, train_mode=True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        dec.eval()
        with pytest.raises(_lib.TpsppError, match="GPU tensor"):    # eval on the host: no CPU path in any mode
            dec(feat, None, None, None, train_mode=False)
    x = feat.clone().requires_grad_(True)                           # an input that requires grad: the graph-building forward
    y = dec(x, None, None, None, train_mode=False)
    want = twin.eval()._forward_torch(feat.clone().requires_grad_(True))       # (PyTorch's own bits differ with a graph)
    assert y.grad_fn is not None and torch.equal(y.detach().view(torch.int32), want.detach().view(torch.int32))
    layer = dec.decoder[1]
    assert isinstance(layer, BidirectionalLSTM) and layer.lstm_dtype == mode
    tok = DC.rnd((4, 2, 256), 3)
    with torch.no_grad():
        assert torch.equal(layer.train()(tok), layer._forward_torch(tok))
    layer.eval()


def test_prepared_weights_have_keys_of_their_own():
    """Host tensors suffice: `prepared` and the arrangement are plain torch."""
    layer = BC.build_model("crnn").decoder.decoder[0]
    f32 = layer._hip_weights()
    a = layer._hip_weights_bf16(False)
    b = layer._hip_weights_bf16(True)
    assert layer._hip_weights() is f32 and layer._hip_weights_bf16(False) is a and layer._hip_weights_bf16(True) is b
    assert {"lstm", "lstm_bf16", "lstm_bf16x3"} <= set(layer.__dict__["_tpspp_prepared"])
    w_ih, w_hh = b
    assert w_ih.x3 and w_hh.x3 and not a[0].x3 and w_ih.bias is not None and w_hh.bias is None
    assert tuple(w_hh.arranged.shape) == (2, 2, 64, 8, 64, 8) and tuple(a[1].arranged.shape) == (2, 1, 64, 8, 64, 8)
    assert torch.equal(ops.dearrange_mfma16(a[1])[:, 0].float(), DC.rb(f32[2]))
    assert not any("prepared" in k or "lstm_dtype" in k for k in layer.state_dict())


@pytest.mark.parametrize("name,positions,margin", [("crnn_tps", 78, 3.6e-3), ("crnn", 18, 4.0e-3)])
def test_the_bars_are_reachable_in_float64_on_the_golden_features(name, positions, margin):
    routes, golden = DC.golden_decoder(name)
    top2 = golden.topk(2, dim=2).values
    gap = (top2[..., 0] - top2[..., 1]).min().item()
    e0 = (routes[None] - golden).abs().max().item()
    e3 = (routes["bf16x3"] - golden).abs().max().item()
    e16 = (routes[torch.bfloat16] - golden).abs().max().item()
    r3, r16 = DC.rel(routes["bf16x3"], routes[None]), DC.rel(routes[torch.bfloat16], routes[None])
    print(f"{name}: float64 restatement of the decoder on the golden features, logits against the golden: exact {e0:.3e}, "
          f"bf16x3 {e3:.3e} max abs (module bar 1e-4), bf16 {e16:.3e} max abs (smallest top-2 margin {gap:.3e}); "
          f"relative L2 against the exact route: bf16x3 {r3:.3e}, bf16 {r16:.3e}")
    assert golden.shape[0] * golden.shape[1] == positions and gap >= margin
    assert e0 <= 1e-4 and e3 <= 1e-4
    assert 2 * e16 < gap                                            # ... so no arg-max can move
    for mode in DC.MODES:
        assert torch.equal(routes[mode].argmax(2), golden.argmax(2))
