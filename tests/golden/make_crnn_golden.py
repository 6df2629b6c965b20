"""Writes tests/golden/crnn_tps.npz, crnn_state_dict_keys.json and crnn_models.json from the reference (BUILD CONTAINER
ONLY: needs /root/reference).

    python tests/golden/make_crnn_golden.py

Executes the reference's own files by path under the stubs of `_ref_loader.py` plus a few of its own (below):
backbones/very_deep_vgg.py, layers/lstm_layer.py, decoders/crnn_decoder.py, convertors/ctc.py, losses/ctc_loss.py and
recognizer/crnn.py's wiring restated as the four calls `EncodeDecodeRecognizer` makes (preprocessor -> backbone ->
decoder -> convertor / loss: its base classes need mmdet).  Inputs and weights are crnn_cases.py's; only outputs are stored.

The smallest top-2 logit margin over all positions must be >= crnn_cases.MARGIN (ten times the score bar), otherwise
"identical strings" would be a coin toss on random weights: the script searches the seeds from 0 for the first that holds
and refuses to write unless it is crnn_cases.SEED.  The archive is written with fixed zip time stamps: a second run
reproduces it byte for byte.
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import _ref_loader as RL  # noqa: E402
import crnn_cases as CC  # noqa: E402

torch.manual_seed(0)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def load_crnn_reference():
    R = RL.load_reference()
    base = "mmocr/models/textrecog"
    for p in ("decoders", "layers", "convertors", "losses"):
        RL._pkg(f"mmocr.models.textrecog.{p}")
    builder = sys.modules["mmocr.models.builder"]
    builder.LOSSES = RL._Registry("loss")
    trans = types.ModuleType("mmocr.models.textrecog.decoders.Trans")      # never released; crnn_decoder.py only imports it
    trans.TFCommonDecoderLayer = type("TFCommonDecoderLayer", (nn.Module,), {})
    sys.modules[trans.__name__] = trans
    vgg = RL._load("mmocr.models.textrecog.backbones.very_deep_vgg", f"{base}/backbones/very_deep_vgg.py")
    lstm = RL._load("mmocr.models.textrecog.layers.lstm_layer", f"{base}/layers/lstm_layer.py")
    sys.modules["mmocr.models.textrecog.layers"].BidirectionalLSTM = lstm.BidirectionalLSTM
    dec = RL._load("mmocr.models.textrecog.decoders.crnn_decoder", f"{base}/decoders/crnn_decoder.py")
    ctc = RL._load("mmocr.models.textrecog.convertors.ctc", f"{base}/convertors/ctc.py")
    loss = RL._load("mmocr.models.textrecog.losses.ctc_loss", f"{base}/losses/ctc_loss.py")
    return dict(R, very_deep_vgg=vgg, crnn_decoder=dec, ctc=ctc, ctc_loss=loss)


def config_models():
    out = {}
    for name, rel in (("crnn_tps", "configs/_base_/recog_models/crnn_tps.py"), ("crnn", "configs/_base_/recog_models/crnn.py")):
        ns = {}
        exec(compile(open(os.path.join(RL.REF, rel)).read(), rel, "exec"), ns)
        out[name] = ns["model"]
    return out


class Model(nn.Module):
    """The sub-modules `EncodeDecodeRecognizer.__init__` builds from the model dict, under its attribute names."""

    def __init__(self, R, cfg):
        super().__init__()
        self.label_convertor = R["ctc"].CTCConvertor(**{k: v for k, v in cfg["label_convertor"].items() if k != "type"})
        pre = cfg["preprocessor"]
        self.preprocessor = None if pre is None else R["tps_preprocessor"].TPSPreprocessor(
            **{k: v for k, v in pre.items() if k != "type"})
        self.backbone = R["very_deep_vgg"].VeryDeepVgg(**{k: v for k, v in cfg["backbone"].items() if k != "type"})
        self.decoder = R["crnn_decoder"].CRNNDecoder(num_classes=self.label_convertor.num_classes(),
                                                     **{k: v for k, v in cfg["decoder"].items() if k != "type"})
        self.loss = R["ctc_loss"].CTCLoss(**{k: v for k, v in cfg["loss"].items() if k != "type"})

    def load(self, seed):
        sd = CC.state(self.state_dict(), seed)
        missing = self.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
        assert set(missing.missing_keys) <= set(CC.KEEP) | {k for k in self.state_dict() if k.endswith("num_batches_tracked")}
        return self

    def run(self, img):
        rect = img if self.preprocessor is None else self.preprocessor(img)
        feat = self.backbone(rect)
        return rect, feat, self.decoder(feat, None, None, None, train_mode=False)


def margin(logits):
    top = logits.topk(2, dim=2).values
    return float((top[..., 0] - top[..., 1]).min())


def padded(lists, T, width=None, fill=-1, dtype=np.int32):
    out = np.full((len(lists), T) + (() if width is None else (width,)), fill, dtype=dtype)
    for i, row in enumerate(lists):
        if len(row):
            out[i, :len(row)] = np.asarray(row, dtype=dtype)
    return out


def write_npz(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"  wrote {os.path.basename(path)}  {os.path.getsize(path) / 1024:.0f} KiB  "
          f"[{', '.join(f'{k}{tuple(np.shape(v))}' for k, v in arrs.items())}]")


def main():
    R = load_crnn_reference()
    cfgs = config_models()
    with open(os.path.join(HERE, "crnn_models.json"), "w") as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write("\n")
    img, img32 = t(CC.images()), t(CC.images32())
    full, plain = Model(R, cfgs["crnn_tps"]).eval(), Model(R, cfgs["crnn"]).eval()
    with open(os.path.join(HERE, "crnn_state_dict_keys.json"), "w") as f:
        json.dump({"CRNNNet(crnn_tps)": {k: list(v.shape) for k, v in full.state_dict().items()},
                   "CRNNNet(crnn)": {k: list(v.shape) for k, v in plain.state_dict().items()},
                   "VeryDeepVgg": {k: list(v.shape) for k, v in full.backbone.state_dict().items()},
                   "CRNNDecoder": {k: list(v.shape) for k, v in full.decoder.state_dict().items()}}, f, indent=1)
        f.write("\n")
    assert len(full.backbone.state_dict()) == 29 and len(full.decoder.state_dict()) == 20

    def outputs(seed):
        with torch.no_grad():
            return full.load(seed).run(img), plain.load(seed).run(img32)

    seed = 0
    while True:
        (rect, feat, logits), (_, feat32, logits32) = outputs(seed)
        m = min(margin(logits), margin(logits32))
        print(f"  seed {seed}: smallest top-2 logit margin {m:.3e}")
        if m >= CC.MARGIN:
            break
        seed += 1
        assert seed < 64, "no seed with a usable margin"
    assert seed == CC.SEED, f"crnn_cases.SEED must be {seed}"
    assert tuple(feat.shape) == (CC.N, 512, 1, 26) and tuple(logits.shape) == (CC.N, 26, 37)
    assert tuple(feat32.shape) == (CC.N32, 512, 1, 9) and tuple(logits32.shape) == (CC.N32, 9, 37)
    assert float(full.preprocessor.LocalizationNetwork.localization_fc2.weight.detach().abs().max()) > 0

    conv = full.label_convertor
    T = logits.shape[1]
    metas = CC.img_metas(CC.N, CC.VALID_RATIOS)
    idx, score = conv.tensor2idx(logits, metas)
    idx1, score1 = conv.tensor2idx(logits, CC.img_metas(CC.N))
    idxk, scorek = conv.tensor2idx(logits, metas, topk=CC.TOPK, return_topk=True)
    idx32, score32 = conv.tensor2idx(logits32, CC.img_metas(CC.N32))
    # the loss and its gradient with respect to the logits, as EncodeDecodeRecognizer.forward_train calls it
    lg = logits.clone().requires_grad_(True)
    loss = full.loss(lg, conv.str2tensor(CC.TEXTS), CC.img_metas(CC.N))["loss_ctc"]
    loss.backward()
    write_npz(os.path.join(HERE, "crnn_tps.npz"), dict(
        rect=rect.numpy(), feat=feat.numpy(), logits=logits.numpy(),
        idx=padded(idx, T), score=padded(score, T, fill=0, dtype=np.float64),
        idx_full=padded(idx1, T), score_full=padded(score1, T, fill=0, dtype=np.float64),
        idx_topk=padded(idxk, T, CC.TOPK), score_topk=padded(scorek, T, CC.TOPK, fill=0, dtype=np.float64),
        loss=loss.detach().numpy(), loss_grad=lg.grad.numpy(),
        feat32=feat32.numpy(), logits32=logits32.numpy(),
        idx32=padded(idx32, logits32.shape[1]), score32=padded(score32, logits32.shape[1], fill=0, dtype=np.float64)))
    print("  strings:", conv.idx2str(idx1), conv.idx2str(idx32))


if __name__ == "__main__":
    main()
