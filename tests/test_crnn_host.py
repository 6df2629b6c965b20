"""Host side (no GPU) of the CRNN recogniser: the mirrors' state-dict keys and PyTorch paths against the reference's outputs
(tests/golden/crnn_tps.npz), both config dicts, the argument checks of every entry point of include/tpspp_crnn.h (host
pointers: nothing is launched) and the LSTM launch planner restated from a case table."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

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


def build_model(name):
    m = build_detector(CC.models()[name]).eval()
    sd = CC.state(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m


@pytest.fixture(scope="module")
def model():
    return build_model("crnn_tps")


def ragged(idx, score):
    """The fixture's padded (idx, score) rows -> lists."""
    return [r[r >= 0].tolist() for r in idx], [s[r >= 0].tolist() for r, s in zip(idx, score)]


# ---- the mirrors -------------------------------------------------------------------------------------------------------
def test_state_dict_keys_equal_the_references():
    with open(os.path.join(HERE, "golden", "crnn_state_dict_keys.json")) as f:
        want = json.load(f)
    for name in ("crnn_tps", "crnn"):
        m = build_detector(CC.models()[name])
        assert isinstance(m, tps_pp_amd.CRNNNet)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == want[f"CRNNNet({name})"]
        assert list(m.state_dict()) == list(want[f"CRNNNet({name})"])
    assert (m.preprocessor is None) and build_detector(CC.models()["crnn_tps"]).preprocessor is not None
    vgg = tps_pp_amd.build_backbone(dict(type="VeryDeepVgg", leaky_relu=False, input_channels=1))
    assert {k: list(v.shape) for k, v in vgg.state_dict().items()} == want["VeryDeepVgg"] and len(want["VeryDeepVgg"]) == 29
    assert vgg.out_channels() == 512
    dec = tps_pp_amd.build_decoder(dict(type="CRNNDecoder", in_channels=512, num_classes=37, rnn_flag=True))
    assert {k: list(v.shape) for k, v in dec.state_dict().items()} == want["CRNNDecoder"] and len(want["CRNNDecoder"]) == 20
    assert "decoder.0.rnn.weight_ih_l0_reverse" in want["CRNNDecoder"] and "decoder.0.embedding.weight" in want["CRNNDecoder"]
    cnn = tps_pp_amd.build_decoder(dict(type="CRNNDecoder", in_channels=512, num_classes=37, rnn_flag=False))
    assert list(cnn.state_dict()) == ["decoder.weight", "decoder.bias"]


def test_torch_paths_reproduce_the_reference(model, G):
    with torch.no_grad():
        feat = model.backbone._forward_torch(torch.from_numpy(G["rect"]))
        logits = model.decoder._forward_torch(feat)
    assert tuple(feat.shape) == (CC.N, 512, 1, 26) and tuple(logits.shape) == (CC.N, 26, 37)
    assert np.abs(feat.numpy() - G["feat"]).max() <= TOL
    assert np.abs(logits.numpy() - G["logits"]).max() <= TOL
    plain = build_model("crnn")
    with torch.no_grad():
        feat32 = plain.backbone._forward_torch(torch.from_numpy(CC.images32()))
        logits32 = plain.decoder._forward_torch(feat32)
    assert np.abs(feat32.numpy() - G["feat32"]).max() <= TOL and np.abs(logits32.numpy() - G["logits32"]).max() <= TOL
    # the decoder's calling convention, in eval mode on a tensor that carries gradients: the PyTorch composition
    out = model.decoder(torch.from_numpy(G["feat"]).requires_grad_(True), None, None, None, train_mode=False)
    assert out.grad_fn is not None and np.abs(out.detach().numpy() - G["logits"]).max() <= TOL


def test_eval_forward_on_the_host_raises(model, G):
    with torch.no_grad(), pytest.raises(_lib.TpsppError, match="GPU tensor"):
        model.backbone(torch.from_numpy(G["rect"]))
    with torch.no_grad(), pytest.raises(_lib.TpsppError, match="GPU tensor"):
        model.decoder(torch.from_numpy(G["feat"]), None, None, None, train_mode=False)


def test_convertor_reproduces_the_reference(model, G):
    conv = model.label_convertor
    assert conv.num_classes() == 37 and conv.blank_idx == 0 and conv.idx2char[0] == "<BLK>" and conv.unknown_idx is None
    assert conv.lower and conv.str2idx(["Ab0"]) == [[11, 12, 1]]
    with pytest.raises(Exception, match="not in dict"):
        conv.str2idx(["a-b"])
    ukn = tps_pp_amd.build_convertor(dict(type="CTCConvertor", dict_type="DICT90", with_unknown=True))
    assert ukn.num_classes() == 92 and ukn.unknown_idx == 91 and ukn.str2idx(["aé"]) == [[11, 91]]
    td = conv.str2tensor(["hello", "tps"])
    assert td["flatten_targets"].dtype == torch.int32 and td["target_lengths"].tolist() == [5, 3]
    assert [x.tolist() for x in td["targets"]] == conv.str2idx(["hello", "tps"])
    logits = torch.from_numpy(G["logits"])
    for metas, ki, ks in ((CC.img_metas(CC.N, CC.VALID_RATIOS), "idx", "score"), (CC.img_metas(CC.N), "idx_full", "score_full")):
        idx, score = conv.tensor2idx(logits, metas)
        wi, ws = ragged(G[ki], G[ks])
        assert idx == wi
        assert all(len(a) == len(b) and np.abs(np.array(a) - np.array(b)).max(initial=0) <= TOL for a, b in zip(score, ws))
        assert conv.tensor2str(logits, metas)[0] == conv.idx2str(wi)
    idxk, scorek = conv.tensor2idx(logits, CC.img_metas(CC.N, CC.VALID_RATIOS), topk=CC.TOPK, return_topk=True)
    for n in range(CC.N):
        keep = G["idx_topk"][n, :, 0] >= 0
        assert idxk[n] == G["idx_topk"][n][keep].tolist()
        assert np.abs(np.array(scorek[n]).reshape(-1, CC.TOPK) - G["score_topk"][n][keep]).max(initial=0) <= TOL
    i3, s3 = conv.tensor2idx(logits, CC.img_metas(CC.N, CC.VALID_RATIOS), topk=CC.TOPK)
    assert i3 == ragged(G["idx"], G["score"])[0]
    i1, s1 = conv.tensor2idx(logits, CC.img_metas(CC.N, CC.VALID_RATIOS), return_topk=True)
    assert i1 == [[[i] for i in r] for r in ragged(G["idx"], G["score"])[0]]
    # the scan itself, on logits whose arg-max is written down: runs collapse, blanks separate, decode_len cuts
    seq = [3, 3, 0, 3, 0, 0, 5, 5, 5, 2]
    lg = torch.full((2, len(seq), 37), -4.0)
    for t_, c in enumerate(seq):
        lg[:, t_, c] = 4.0
    idx, _ = conv.tensor2idx(lg, [dict(valid_ratio=1.0), dict(valid_ratio=0.75)])
    assert idx == [[3, 3, 5, 2], [3, 3, 5]]                       # ceil(10 * 0.75) = 8 positions


def test_ctc_loss_and_gradient(model, G):
    from tps_pp_amd.losses import CTCLoss
    assert isinstance(model.loss, CTCLoss) and model.loss.flatten and model.loss.blank == 0
    lg = torch.from_numpy(G["logits"]).clone().requires_grad_(True)
    loss = model.loss(lg, model.label_convertor.str2tensor(CC.TEXTS), CC.img_metas(CC.N))["loss_ctc"]
    loss.backward()
    assert abs(loss.item() - G["loss"].reshape(-1)[0].item()) <= TOL
    assert np.abs(lg.grad.numpy() - G["loss_grad"]).max() <= TOL
    # padded targets and input lengths from the valid ratios
    padded = CTCLoss(flatten=False, reduction="sum", zero_infinity=True)
    out = padded(torch.from_numpy(G["logits"]), model.label_convertor.str2tensor(CC.TEXTS), CC.img_metas(CC.N, (1.0, 0.9, 1.0)))
    assert torch.isfinite(out["loss_ctc"])


def test_train_mode_forward_builds_a_graph_on_the_host():
    """`.train()` is PyTorch throughout behind the rectifier: without a preprocessor the whole step runs on the host."""
    m = build_model("crnn").train()
    metas = [dict(resize_shape=(32, 32, 1), text=s) for s in ("ab", "c")]
    losses = m(torch.from_numpy(CC.images32()), metas, return_loss=True)
    loss, log_vars = m._parse_losses(losses)
    loss.backward()
    assert set(losses) == {"loss_ctc"} and np.isfinite(log_vars["loss"])
    assert all(p.grad is not None for p in m.parameters())


# ---- the entry points of include/tpspp_crnn.h ----------------------------------------------------------------------------
def host(n, ctype=ctypes.c_float):
    buf = (ctype * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def test_every_entry_point_refuses_bad_arguments_before_any_launch(lib):
    keep, p = host(64)

    def refused(rc, text):
        assert rc == -22 and text.encode() in lib.tpspp_last_error(), (rc, lib.tpspp_last_error())

    pool = lambda **k: lib.tpspp_crnn_maxpool_fwd(*[{**dict(a=p, N=1, C=1, H=4, W=6, kh=2, kw=2, sh=2, sw=1, ph=0, pw=1, out=p,  # noqa: E731
                                                             Ho=2, Wo=7, s=None), **k}[n] for n in
                                                    ("a", "N", "C", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "out", "Ho", "Wo", "s")])
    refused(pool(a=None), "null pointer")
    refused(pool(out=None), "null pointer")
    refused(pool(ph=2), "padding")                                 # ph > kh / 2
    refused(pool(pw=2), "padding")
    refused(pool(pw=-1), "padding")
    refused(pool(sh=0), "stride")
    refused(pool(kw=0), "kernel")
    refused(pool(Ho=3), "Ho x Wo must be 2 x 7")
    refused(pool(Wo=6), "Ho x Wo must be 2 x 7")
    refused(pool(H=1, ph=0, Ho=1), "smaller than the kernel")
    refused(pool(C=0), "bad sizes")
    assert pool(N=0) == 0                                          # nothing launched

    lstm = lambda **k: lib.tpspp_crnn_lstm_fwd(*[{**dict(xg=p, w=p, out=p, T=2, N=1, hidden=256, g=0, s=None), **k}[n]  # noqa: E731
                                                 for n in ("xg", "w", "out", "T", "N", "hidden", "g", "s")])
    for name in ("xg", "w", "out"):
        refused(lstm(**{name: None}), "null pointer")
    refused(lstm(hidden=128), "hidden must be 256")
    refused(lstm(hidden=512), "hidden must be 256")
    refused(lstm(T=0), "T >= 1")
    refused(lstm(N=-1), "bad sizes")
    for g in (1, 2, 3, 5, 12, 32, -4):
        refused(lstm(g=g), "images_per_group must be 0, 4, 8 or 16")
    assert lstm(N=0) == 0 and all(lstm(N=0, g=g) == 0 for g in (4, 8, 16))

    dec = lambda **k: lib.tpspp_crnn_ctc_decode(*[{**dict(lg=p, dl=p, N=1, T=3, C=5, blank=0, idx=p, sc=p, s=None), **k}[n]  # noqa: E731
                                                  for n in ("lg", "dl", "N", "T", "C", "blank", "idx", "sc", "s")])
    for name in ("lg", "dl", "idx", "sc"):
        refused(dec(**{name: None}), "null pointer")
    refused(dec(C=1), "C must be >= 2")
    refused(dec(blank=5), "blank 5 out of range")
    refused(dec(blank=-1), "out of range")
    refused(dec(T=0), "T >= 1")
    refused(dec(N=-1), "bad sizes")
    assert dec(N=0) == 0
    del keep


# (N, images_per_group, CUs) -> images per workgroup; the branch each row takes
PLAN_CASES = [
    ((512, 0, 256), 4, "g4 fills"),          # 2 * 128 = 256 workgroups
    ((1024, 0, 256), 8, "g8 fills"),         # 2 * 128
    ((2048, 0, 256), 16, "g16 fills"),
    ((100000, 0, 256), 16, "g16 fills"),
    ((2047, 0, 256), 16, "g16 fills"),       # ceil(2047 / 16) = 128
    ((2032, 0, 256), 8, "g8 fills"),         # ceil(2032 / 16) = 127
    ((1017, 0, 256), 8, "g8 fills"),         # ceil(1017 / 8) = 128
    ((1016, 0, 256), 4, "g4 fills"),         # ceil(1016 / 8) = 127: the next smaller group
    ((3, 0, 256), 4, "small batch"),
    ((1, 0, 256), 4, "small batch"),
    ((0, 0, 256), 4, "small batch"),
    ((3, 0, 2), 16, "g16 fills"),            # a two-CU device: one workgroup per direction is enough
    ((3, 16, 256), 16, "explicit"),
    ((3, 8, 256), 8, "explicit"),
    ((5000, 4, 256), 4, "explicit"),
    ((3, 5, 256), -22, "refused"),
    ((3, 1, 256), -22, "refused"),
    ((-1, 0, 256), -22, "refused"),
]


def plan(N, g, cus):
    """The planner of include/tpspp_crnn.h restated: -> (images per workgroup, branch)."""
    if N < 0 or g not in (0, 4, 8, 16):
        return -22, "refused"
    if g:
        return g, "explicit"
    for cand in (16, 8):
        if 2 * -(-N // cand) >= cus:
            return cand, f"g{cand} fills"
    return 4, "g4 fills" if 2 * -(-N // 4) >= cus else "small batch"


def test_lstm_planner_follows_its_case_table(lib):
    seen = set()
    for args, want, branch in PLAN_CASES:
        assert plan(*args) == (want, branch), args
        assert lib.tpspp_crnn_lstm_plan(*args) == want, args
        seen.add(branch)
    assert seen == {"g16 fills", "g8 fills", "g4 fills", "small batch", "explicit", "refused"}
    g = lib.tpspp_crnn_lstm_plan(512, 0, 0)                        # the current device's CU count, 256 without a device
    assert g in (4, 8, 16)
    from tps_pp_amd import ops
    assert ops.CRNN_LSTM_GROUPS == (4, 8, 16) and ops.crnn_lstm_plan(512, 0, 256) == 4
    with pytest.raises(_lib.TpsppError, match="images_per_group"):
        ops.crnn_lstm_plan(3, 7, 256)
