"""The CRNN recogniser the classic TPS rectifier was written for (reference: configs/_base_/recog_models/crnn_tps.py):
`CRNNNet` = `TPSPreprocessor` -> `VeryDeepVgg` -> `CRNNDecoder(rnn_flag=True)` (two `BidirectionalLSTM`) ->
`CTCConvertor`, trained with `CTCLoss` (tps_pp_amd/losses.py).

Mirrors of `backbones/very_deep_vgg.py`, `layers/lstm_layer.py`, `decoders/crnn_decoder.py`, `convertors/ctc.py` and
`recognizer/crnn.py`: the same registry names, constructor arguments, sub-module names and hence `state_dict` keys.

Which path a call takes is `LocalizationNetwork`'s rule.  `.eval()` on a GPU tensor that carries no gradient runs the HIP
kernels: the 3x3 convolutions (BatchNorm folded) on `ops.conv2d`, the pools, the LSTM recurrence and the CTC decode on
the kernels of include/tpspp_crnn.h, every Linear on `tpspp_mm_f32`; a CPU tensor raises.  `.train()`, or an input
that requires grad, runs the PyTorch composition of the same layers (`nn.LSTM`, `nn.Linear`, `nn.Conv2d`): the model
trains through PyTorch plus the HIP warp forward and backward of the preprocessor.  `CRNNDecoder.set_train_backend("hip")`
(and `CTCLoss.set_train_backend("hip")`, tps_pp_amd/losses.py) moves the recurrent half of that training graph onto the
kernels of include/tpspp_crnn_train.h, and `TPSPreprocessor.set_train_backend("hip")` the preprocessor's localisation network
onto HIP kernels (`CRNNNet.set_train_backend("torch", preprocessor="hip", decoder="hip", loss="hip")` sets all three).
`VeryDeepVgg.set_vgg_train_backend("hip")` (`CRNNNet.set_vgg_train_backend`; opt-in, default "torch") moves the VGG with its
pools: the convolutions on the fp32 forward / backward kernels, the max-pools' backward with the ReLU mask on
`tpspp_crnn_maxpool_bwd` (include/tpspp.h), the BatchNorms on the backbone's training kernels.
`CRNNDecoder.set_train_compute_dtype("bf16x3")` (opt-in) runs that HIP training
graph's LSTM layers on the bf16 matrix cores, forward and backward, as three-term splits (include/tpspp.h).

Precision: `set_compute_dtype` of the recogniser (None | "bf16x3" | torch.bfloat16) means for the VGG what it means for
the NRTR backbone, and keeps its meaning for the preprocessor (its localisation network).  None, the default, is the
exact fp32 path.  In a reduced mode the seven convolutions run on the bf16 matrix cores (`ops.conv2d_bf16`: plain bf16
operands and maps, or the three-term split on fp32 maps), the feature maps stay in the blocked layout from conv0's output
to conv6's input, and the four pools run on it (include/tpspp_crnn_bf16.h); the features leave as fp32.  The decoder
stays exact fp32 unless it is asked: `set_compute_dtype(mode, decoder=mode)` of the recogniser, or
`CRNNDecoder.set_compute_dtype(mode)`, moves the two LSTM input projections and the two recurrences of the eval path onto
the bf16 matrix cores (`tpspp_mm_bf16`, `tpspp_crnn_lstm_bf16_fwd`, include/tpspp.h: operands rounded or split, fp32
accumulation, fp32 cell state and outputs).  The embeddings and the CTC decode stay exact fp32 in every mode, as NRTR's
per-step projections do.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from . import ops
from ._prepared import prepared
from .nrtr_head import BaseConvertor, EncodeDecodeRecognizer
from .precision import default_compute_dtype
from .registry import BACKBONES, CONVERTORS, DECODERS, DETECTORS, TrainBackendMixin


def _hip_path(module, x):
    """LocalizationNetwork's rule: the HIP kernels unless the module trains or the input carries gradients."""
    return not (module.training or (torch.is_grad_enabled() and x.requires_grad))


@BACKBONES.register_module()
class VeryDeepVgg(nn.Module):
    """`backbones/very_deep_vgg.py`: seven convolutions (BatchNorm after 2, 4, 6), four max-pools, (N, C, 32, W) ->
    (N, 512, 1, W / 4 + 1).

    `leaky_relu=True` (the reference's default; crnn_tps.py sets False) has no HIP path: the convolution kernel's
    epilogues are ReLU and GELU, so such a module always takes the PyTorch composition.

    `compute_dtype` (not in the reference; `precision.default_compute_dtype()` when constructed) selects the arithmetic
    of the HIP path: None the exact fp32 kernels; "bf16x3" fp32 maps and every convolution as the three-term bf16 split;
    torch.bfloat16 bf16 operands and bf16 maps.  In the reduced modes the maps stay in the blocked layout between the
    layers (`_forward_hip_bf16`).  `.train()`, an input that requires grad and `leaky_relu=True` take the PyTorch
    composition whatever it says."""

    def __init__(self, leaky_relu=True, input_channels=3, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg
        ks, ps = [3, 3, 3, 3, 3, 3, 2], [1, 1, 1, 1, 1, 1, 0]
        nm = [64, 128, 256, 256, 512, 512, 512]
        self.channels = nm
        self.leaky_relu = leaky_relu
        self.compute_dtype = default_compute_dtype()   # None: exact fp32; "bf16x3" / torch.bfloat16: `_forward_hip_bf16`
        cnn = nn.Sequential()

        def conv_relu(i, batch_normalization=False):
            n_in = input_channels if i == 0 else nm[i - 1]
            cnn.add_module(f"conv{i}", nn.Conv2d(n_in, nm[i], ks[i], 1, ps[i]))
            if batch_normalization:
                cnn.add_module(f"batchnorm{i}", nn.BatchNorm2d(nm[i]))
            cnn.add_module(f"relu{i}", nn.LeakyReLU(0.2, inplace=True) if leaky_relu else nn.ReLU(True))

        conv_relu(0)
        cnn.add_module("pooling0", nn.MaxPool2d(2, 2))
        conv_relu(1)
        cnn.add_module("pooling1", nn.MaxPool2d(2, 2))
        conv_relu(2, True)
        conv_relu(3)
        cnn.add_module("pooling2", nn.MaxPool2d((2, 2), (2, 1), (0, 1)))
        conv_relu(4, True)
        conv_relu(5)
        cnn.add_module("pooling3", nn.MaxPool2d((2, 2), (2, 1), (0, 1)))
        conv_relu(6, True)
        self.cnn = cnn

    def init_weights(self):
        pass

    def out_channels(self):
        return self.channels[-1]

    def _hip_weights(self):
        """conv0-5 as they are (bias; BatchNorm of 2 and 4 folded) and conv6, the 2x2 valid convolution, as a 3x3 kernel
        whose first row and first column are zero: at stride (2, 1) on the two-row map its "same" padding reads rows 0, 1
        and columns x, x + 1 under the four real taps (`conv6`)."""
        c = self.cnn
        bns = {2: c.batchnorm2, 4: c.batchnorm4, 6: c.batchnorm6}
        convs = [getattr(c, f"conv{i}") for i in range(7)]

        def build():
            out = []
            for i, conv in enumerate(convs):
                w, bn = conv.weight, bns.get(i)
                if i == 6:
                    w = Fn.pad(w.detach(), (1, 0, 1, 0))
                out.append(ops.prep_conv_weight(w, bn=None if bn is None else ops.bn_tensors(bn), conv_bias=conv.bias,
                                                eps=1e-5 if bn is None else bn.eps))
            return out
        return prepared(self, "vgg", convs + list(bns.values()), build)

    def _hip_weights_bf16(self, x3):
        """`_hip_weights` for the bf16 matrix cores: the same folding in fp32 (bias; BatchNorm of 2, 4, 6; conv6
        zero-extended to 3x3), then rounded to bf16 or, `x3`, split into the hi and lo slabs of the three-term product."""
        c = self.cnn
        bns = {2: c.batchnorm2, 4: c.batchnorm4, 6: c.batchnorm6}
        convs = [getattr(c, f"conv{i}") for i in range(7)]

        def build():
            out = []
            for i, conv in enumerate(convs):
                w, bn = conv.weight, bns.get(i)
                if i == 6:
                    w = Fn.pad(w.detach(), (1, 0, 1, 0))
                out.append(ops.prep_conv_weight_bf16(w, bn=None if bn is None else ops.bn_tensors(bn), conv_bias=conv.bias,
                                                     eps=1e-5 if bn is None else bn.eps, x3=x3))
            return out
        return prepared(self, "vgg_bf16x3" if x3 else "vgg_bf16", convs + list(bns.values()), build)

    @staticmethod
    def conv6(x, cw):
        """The 2x2 valid convolution + folded BatchNorm + ReLU of a (N, 512, 2, W) map -> (N, 512, 1, W - 1), a view of
        the (N, 512, 1, W) map the zero-extended 3x3 kernel gives (its last column reads the right padding)."""
        if x.shape[2] != 2:
            raise ValueError(f"VeryDeepVgg: the HIP path needs an image height of 32 (a two-row map before conv6), got "
                             f"{x.shape[2]} rows")
        return ops.conv2d([x], cw, (2, 1), True)[:, :, :, :x.shape[3] - 1]

    VGG_TRAIN_BACKENDS = ("torch", "hip")
    vgg_train_backend = "torch"                     # `set_vgg_train_backend`; a plain attribute, never in the state_dict

    def set_vgg_train_backend(self, mode):
        """Which kernels the graph-building forward (`.train()`, or an input that carries gradients) runs on: "torch"
        (default) -- the PyTorch composition `self.cnn`; "hip" -- `_forward_train_hip`, HIP forward and backward for every
        layer, taken for a GPU tensor (a host tensor keeps the PyTorch composition).  `leaky_relu=True` refuses "hip": the
        kernels' activation is ReLU.  Touches neither the parameters, the buffers, the state_dict nor the eval path.
        (Its own name, not `set_train_backend`: the recogniser's `set_train_backend(..., backbone=)` tells a backbone with
        a HIP training path by that attribute, and goes on refusing this one.)"""
        if mode not in self.VGG_TRAIN_BACKENDS:
            raise ValueError(f'set_vgg_train_backend: "torch" or "hip", got {mode!r}')
        if mode == "hip" and self.leaky_relu:
            raise ValueError('set_vgg_train_backend: "hip" needs leaky_relu=False (the HIP kernels\' activation is ReLU)')
        self.vgg_train_backend = mode
        return self

    def _train_weights(self):
        """The forward's weight layouts for `_forward_train_hip` (no BatchNorm folded; conv6 with its zero-extended 3x3
        kernel: `ops.conv6_extend`), cached and rebuilt on the device when a parameter changes (`_prepared`)."""
        convs = [getattr(self.cnn, f"conv{i}") for i in range(7)]
        return prepared(self, "vgg_train", convs, lambda: [
            ops.conv6_extend(c) if i == 6 else ops.prep_conv_weight_device(c.weight, c.bias) for i, c in enumerate(convs)])

    def _forward_train_hip(self, x):
        """`self.cnn` on the HIP kernels inside an autograd graph (`set_vgg_train_backend("hip")`): conv0, conv1, conv3 and
        conv5 with the pool behind them each one `ops.conv_relu_pool_autograd` (the pool's backward carries the ReLU mask:
        `tpspp_crnn_maxpool_bwd`), conv2 and conv4 `ops.bn_stem_autograd`, conv6 `ops.conv6_bn_autograd`.  Exact fp32
        whatever `compute_dtype` says; every BatchNorm follows its own mode."""
        c, cw = self.cnn, self._train_weights()
        x = x.float().contiguous()
        x = ops.conv_relu_pool_autograd(x, c.conv0, 2, 2, 0, cw[0], name="conv0")
        x = ops.conv_relu_pool_autograd(x, c.conv1, 2, 2, 0, cw[1], name="conv1")
        x = ops.bn_stem_autograd(x, c.conv2, c.batchnorm2, cw[2], name="conv2")
        x = ops.conv_relu_pool_autograd(x, c.conv3, (2, 2), (2, 1), (0, 1), cw[3], name="conv3")
        x = ops.bn_stem_autograd(x, c.conv4, c.batchnorm4, cw[4], name="conv4")
        x = ops.conv_relu_pool_autograd(x, c.conv5, (2, 2), (2, 1), (0, 1), cw[5], name="conv5")
        return ops.conv6_bn_autograd(x, c.conv6, c.batchnorm6, cw[6], name="conv6")

    def forward(self, x):
        if self.leaky_relu or not _hip_path(self, x):
            if self.vgg_train_backend == "hip" and not self.leaky_relu and x.is_cuda:
                return self._forward_train_hip(x)
            return self.cnn(x)
        ops.require_gpu(x, "VeryDeepVgg")
        ops.warn_detached_once(self, "VeryDeepVgg")
        if self.compute_dtype is not None:
            return self._forward_hip_bf16(x, self.compute_dtype == "bf16x3")
        cw = self._hip_weights()
        x = x.float().contiguous()
        x = ops.crnn_maxpool(ops.conv2d([x], cw[0], 1, True), 2, 2, 0)
        x = ops.crnn_maxpool(ops.conv2d([x], cw[1], 1, True), 2, 2, 0)
        x = ops.conv2d([ops.conv2d([x], cw[2], 1, True)], cw[3], 1, True)
        x = ops.crnn_maxpool(x, (2, 2), (2, 1), (0, 1))
        x = ops.conv2d([ops.conv2d([x], cw[4], 1, True)], cw[5], 1, True)
        x = ops.crnn_maxpool(x, (2, 2), (2, 1), (0, 1))
        return self.conv6(x, cw[6])

    def _forward_hip_bf16(self, x, x3):
        """The reduced modes: every convolution on `tpspp_conv2d_bf16_fwd` -- plain bf16 operands and bf16 maps, or, `x3`,
        the three-term split on fp32 maps --, the maps blocked (`Blocked` / `Blocked32`) from conv0's output to conv6's
        input, the pools on `tpspp_crnn_maxpool_blk_fwd`; no NCHW copy of an intermediate map.  The image is taken as it
        comes, fp32 or bf16 NCHW; the result is fp32 (N, 512, 1, W / 4 + 1) as in the exact mode."""
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        cw = self._hip_weights_bf16(x3)
        dt = torch.float32 if x3 else torch.bfloat16

        def conv(t, i):
            return ops.conv2d_bf16([t], cw[i], 1, True, out_dtype=dt, out_blocked=True)
        x = ops.crnn_maxpool_blocked(conv(x.contiguous(), 0), 2, 2, 0)
        x = ops.crnn_maxpool_blocked(conv(x, 1), 2, 2, 0)
        x = ops.crnn_maxpool_blocked(conv(conv(x, 2), 3), (2, 2), (2, 1), (0, 1))
        x = ops.crnn_maxpool_blocked(conv(conv(x, 4), 5), (2, 2), (2, 1), (0, 1))
        if x.shape[2] != 2:
            raise ValueError(f"VeryDeepVgg: the HIP path needs an image height of 32 (a two-row map before conv6), got "
                             f"{x.shape[2]} rows")
        return ops.conv2d_bf16([x], cw[6], (2, 1), True, out_dtype=torch.float32)[:, :, :, :x.shape[3] - 1]

    def _forward_torch(self, x):
        """TEST HOOK: the PyTorch composition whatever the mode."""
        return self.cnn(x)


class BidirectionalLSTM(nn.Module):
    """`layers/lstm_layer.py`: nn.LSTM(nIn, nHidden, bidirectional=True) and a Linear over its 2 nHidden outputs,
    (T, N, nIn) -> (T, N, nOut).  The HIP path (nHidden = 256) is driven by `CRNNDecoder`, which also chooses the layouts."""

    def __init__(self, nIn, nHidden, nOut):
        super().__init__()
        self.lstm_dtype = None                      # the HIP path's arithmetic: `CRNNDecoder.set_compute_dtype` sets it
        self.rnn = nn.LSTM(nIn, nHidden, bidirectional=True)
        self.embedding = nn.Linear(nHidden * 2, nOut)

    def _hip_weights(self):
        """(w_ih of both directions (8 H, nIn), b_ih + b_hh of both (8 H), w_hh of both (2, 4 H, H))."""
        r = self.rnn
        return prepared(self, "lstm", [r], lambda: (
            torch.cat([r.weight_ih_l0, r.weight_ih_l0_reverse]).detach().float().contiguous(),
            torch.cat([r.bias_ih_l0 + r.bias_hh_l0, r.bias_ih_l0_reverse + r.bias_hh_l0_reverse]).detach().float().contiguous(),
            torch.stack([r.weight_hh_l0, r.weight_hh_l0_reverse]).detach().float().contiguous()))

    def _hip_weights_bf16(self, x3):
        """`_hip_weights` for the bf16 matrix cores: (w_ih of both directions with b_ih + b_hh, w_hh of both), each an
        `ops.MfmaWeight` -- rounded to bf16 or, `x3`, split into the hi and lo slabs of the three-term product.  Keys of
        its own: the fp32 set stays prepared next to it."""
        r = self.rnn

        def build():
            w_ih, b, w_hh = self._hip_weights()
            return ops.arrange_mfma16(w_ih, b, x3=x3), ops.arrange_mfma16(w_hh, x3=x3)
        return prepared(self, "lstm_bf16x3" if x3 else "lstm_bf16", [r], build)

    def recurrent_hip(self, x, desc, T, N, images_per_group=0, mode=None):
        """The LSTM of the token operand x (`desc` = (batch = T, rows = N, batch stride, row stride, k stride), as
        `ops.linear_fwd` takes it) -> (T, N, 2 H): one product for the input pre-activations of all tokens and both
        directions, then the recurrence kernel.  `mode`: None the exact fp32 kernels; "bf16x3" / torch.bfloat16 both
        products on the bf16 matrix cores (`tpspp_mm_bf16`, `tpspp_crnn_lstm_bf16_fwd`)."""
        if self.rnn.hidden_size != ops.CRNN_HIDDEN or self.rnn.num_layers != 1:
            raise ValueError("BidirectionalLSTM: the HIP recurrence serves one layer of 256 hidden units")
        if mode is not None:
            w_ih, w_hh = self._hip_weights_bf16(mode == "bf16x3")
            xg = ops.linear_bf16_fwd(x, desc, w_ih)
            return ops.crnn_lstm_bf16(xg.view(T, N, 2, 4 * ops.CRNN_HIDDEN), w_hh, images_per_group)
        w_ih, b, w_hh = self._hip_weights()
        xg = ops.linear_fwd(x, desc, w_ih, b)                                  # (T N, 2 * 4 H)
        return ops.crnn_lstm(xg.view(T, N, 2, 4 * ops.CRNN_HIDDEN), w_hh, images_per_group)

    def forward(self, input):
        if not _hip_path(self, input):
            return self._forward_torch(input)
        ops.require_gpu(input, "BidirectionalLSTM")
        x = input.float().contiguous()
        T, N, K = x.shape
        rec = self.recurrent_hip(x, (T, N, N * K, K, 1), T, N, mode=self.lstm_dtype)
        emb = self.embedding
        return ops.linear_fwd(rec, ops._dense(T * N, rec.shape[2]), emb.weight.detach(), emb.bias.detach()).view(T, N, -1)

    def _forward_torch(self, input):
        recurrent, _ = self.rnn(input)
        T, b, h = recurrent.size()
        return self.embedding(recurrent.view(T * b, h)).view(T, b, -1)


@DECODERS.register_module()
class CRNNDecoder(TrainBackendMixin, nn.Module):
    """`decoders/crnn_decoder.py`: (N, C, 1, W) features -> (N, W, num_classes) raw logits, through two
    `BidirectionalLSTM` (rnn_flag=True) or one 1x1 convolution.  Called as the mirror's decoders are:
    `decoder(feat, out_enc, targets_dict, img_metas, train_mode)`."""

    def set_train_backend(self, mode):
        """ "torch" (default): the training graph is the PyTorch composition; "hip": with rnn_flag and features on the GPU
        it runs on HIP kernels, forward and backward (`_forward_train_hip`).  A host tensor, rnn_flag=False and the eval
        path are not affected."""
        return super().set_train_backend(mode)

    def set_compute_dtype(self, mode):
        """Opt-in precision of the eval fast path (`_forward_hip`, rnn_flag=True; not in the reference).  None (the
        default): the exact fp32 kernels.  "bf16x3" / torch.bfloat16: both LSTM layers' input projections and recurrences
        on the bf16 matrix cores (`tpspp_mm_bf16`, `tpspp_crnn_lstm_bf16_fwd`: three-term split, or plain bf16 operands
        with fp32 accumulation, fp32 cell state and fp32 outputs); the two embeddings and the CTC decode stay exact fp32.
        Kept in `lstm_dtype` (the recogniser's own switch does not reach it unless asked to: `decoder=`).  `.train()`, an
        input that requires grad, a host tensor, rnn_flag=False and `set_train_backend("hip")` are not affected."""
        if not (mode is None or mode == "bf16x3" or mode == torch.bfloat16):
            raise ValueError('set_compute_dtype: None, "bf16x3" or torch.bfloat16')
        self.lstm_dtype = mode
        if self.rnn_flag:
            for layer in self.decoder:
                layer.lstm_dtype = mode
        return self

    def set_train_compute_dtype(self, mode):
        """Opt-in precision of the HIP training graph (`_forward_train_hip`; not in the reference).  None (the default):
        the exact fp32 kernels.  "bf16x3": in both LSTM layers the input projection, the recurrence forward and backward,
        d w_ih, d w_hh and dx run on the bf16 matrix cores as three-term splits with fp32 accumulation
        (`ops.crnn_bilstm_autograd(mode="bf16x3")`); the bias gradients, the embeddings and the CTC loss stay exact fp32.
        It acts only where `_forward_train_hip` runs: `set_train_backend("hip")`, rnn_flag, features on the GPU, not the
        eval fast path.  Kept in `train_lstm_dtype`; `lstm_dtype` (the eval path's) is not touched.  Plain bf16 operands
        are refused: over 26 steps their flipped roundings leave under a factor of two of margin to the bar the tests
        hold a reduced mode to, so plain-bf16 training is a follow-up."""
        if isinstance(mode, torch.dtype) and mode == torch.bfloat16:
            raise ValueError('set_train_compute_dtype: plain-bf16 training is a follow-up; None or "bf16x3"')
        if not (mode is None or (isinstance(mode, str) and mode == "bf16x3")):
            raise ValueError('set_train_compute_dtype: None or "bf16x3"')
        self.train_lstm_dtype = mode
        return self

    def __init__(self, in_channels=None, num_classes=None, rnn_flag=False, init_cfg=None, **kwargs):
        super().__init__()
        self.lstm_dtype = None                      # None: exact fp32; "bf16x3" / torch.bfloat16: `set_compute_dtype`
        self.train_lstm_dtype = None                # None: exact fp32; "bf16x3": `set_train_compute_dtype`
        self.init_cfg = init_cfg
        self.num_classes = num_classes
        self.rnn_flag = rnn_flag
        if rnn_flag:
            self.decoder = nn.Sequential(BidirectionalLSTM(in_channels, 256, 256), BidirectionalLSTM(256, 256, num_classes))
        else:
            self.decoder = nn.Conv2d(in_channels, num_classes, kernel_size=1, stride=1)

    def init_weights(self):
        pass

    def _forward_torch(self, feat):
        """crnn_decoder.py:50-63 (einops' 'b c h w -> b c (h w)' is a reshape)."""
        feat = feat.reshape(feat.size(0), feat.size(1), -1).unsqueeze(2)
        if self.rnn_flag:
            x = feat.squeeze(2).permute(2, 0, 1)                       # (W, N, C)
            for layer in self.decoder:                                  # (Sequential.__call__ would apply each layer's own rule)
                x = layer._forward_torch(x)
            return x.permute(1, 0, 2).contiguous()
        x = self.decoder(feat).permute(0, 3, 1, 2).contiguous()
        n, w, c, h = x.size()
        return x.view(n, w, c * h)

    def _forward_hip(self, feat):
        """No layout pass: the first input projection reads the (W, N, C) tokens out of the NCHW feature map through
        tpspp_mm_f32's strides (a sliced map included), the last embedding writes (N, W, C) through them.  With a reduced
        mode set (`set_compute_dtype`) the two input projections and the two recurrences run on the bf16 matrix cores
        (`tpspp_mm_bf16` reads the same strides); the embeddings stay on tpspp_mm_f32."""
        N, C, H, W = feat.shape
        if H != 1:
            raise ValueError(f"CRNNDecoder: feature height must be 1, got {H}")
        feat = feat.float()
        if not self.rnn_flag:
            conv = self.decoder
            cw = prepared(self, "conv", [conv], lambda: ops.prep_conv_weight(conv.weight, conv_bias=conv.bias))
            y = ops.conv2d([feat.contiguous()], cw, 1, False)          # (N, num_classes, 1, W)
            return y.view(N, -1, W).permute(0, 2, 1).contiguous()
        l0, l1 = self.decoder[0], self.decoder[1]
        if N == 0 and l0.lstm_dtype is not None:    # an empty batch has no device pointer to hand over
            return torch.empty((0, W, l1.embedding.weight.shape[0]), device=feat.device, dtype=torch.float32)
        sn, sc, _, sw = feat.stride()
        rec = l0.recurrent_hip(feat, (W, N, sw, sn, sc), W, N, mode=l0.lstm_dtype)     # token (t, n, c) = feat[n, c, 0, t]
        e0 = l0.embedding
        x = ops.linear_fwd(rec, ops._dense(W * N, rec.shape[2]), e0.weight.detach(), e0.bias.detach())     # (W N, 256)
        K = x.shape[1]
        rec = l1.recurrent_hip(x, (W, N, N * K, K, 1), W, N, mode=l1.lstm_dtype)
        e1 = l1.embedding
        O, K = e1.weight.shape
        out = torch.empty((N, W, O), device=feat.device, dtype=torch.float32)
        ops.mm(rec, (N * K, K, 1), e1.weight.detach(), (0, K, 1), out, (O, W * O, 1), W, N, O, K, bias=e1.bias.detach())
        return out

    def _forward_train_hip(self, feat):
        """The training graph on HIP kernels: per layer the input projection (`tpspp_mm_f32`; the first reads its tokens
        out of the NCHW feature map through its strides), the recurrence that keeps its gates
        (`tpspp_crnn_lstm_train_fwd` / `tpspp_crnn_lstm_bwd`) and the embedding; the last embedding writes (N, W, C).
        With `set_train_compute_dtype("bf16x3")` both LSTM layers run on the bf16 matrix cores, forward and backward."""
        N, C, H, W = feat.shape
        if H != 1:
            raise ValueError(f"CRNNDecoder: feature height must be 1, got {H}")
        feat = feat.float()
        l0, l1 = self.decoder[0], self.decoder[1]
        sn, sc, _, sw = feat.stride()
        kw = {} if self.train_lstm_dtype is None else {"mode": self.train_lstm_dtype}
        rec = ops.crnn_bilstm_autograd(feat, (W, N, sw, sn, sc), W, N, l0.rnn, **kw)
        x = ops.linear_autograd(rec, l0.embedding)                      # (W, N, 256)
        K = x.shape[2]
        rec = ops.crnn_bilstm_autograd(x, (W, N, N * K, K, 1), W, N, l1.rnn, **kw)
        return ops.linear_nwc_autograd(rec, l1.embedding)

    def forward_train(self, feat, out_enc, targets_dict, img_metas):
        if not _hip_path(self, feat):
            if self.train_backend == "hip" and self.rnn_flag and feat.is_cuda:
                return self._forward_train_hip(feat)
            return self._forward_torch(feat)
        ops.require_gpu(feat, "CRNNDecoder")
        ops.warn_detached_once(self, "CRNNDecoder")
        return self._forward_hip(feat)

    def forward_test(self, feat, out_enc, img_metas):
        return self.forward_train(feat, out_enc, None, img_metas)

    def forward(self, feat, out_enc=None, targets_dict=None, img_metas=None, train_mode=True):
        self.train_mode = train_mode
        if train_mode:
            return self.forward_train(feat, out_enc, targets_dict, img_metas)
        return self.forward_test(feat, out_enc, img_metas)


@CONVERTORS.register_module()
class CTCConvertor(BaseConvertor):
    """`convertors/ctc.py`: <BLK> is class 0, <UKN> (with_unknown) the last; `tensor2idx` takes the per-position arg-max,
    collapses runs and drops blanks over the first ceil(T valid_ratio) positions."""

    def __init__(self, dict_type="DICT90", dict_file=None, dict_list=None, with_unknown=True, lower=False, **kwargs):
        super().__init__(dict_type, dict_file, dict_list)
        assert isinstance(with_unknown, bool)
        assert isinstance(lower, bool)
        self.with_unknown = with_unknown
        self.lower = lower
        self.update_dict()

    def update_dict(self):
        self.blank_idx = 0
        self.idx2char.insert(0, "<BLK>")
        self.unknown_idx = None
        if self.with_unknown:
            self.idx2char.append("<UKN>")
            self.unknown_idx = len(self.idx2char) - 1
        self.char2idx = {ch: i for i, ch in enumerate(self.idx2char)}

    def str2tensor(self, strings):
        assert isinstance(strings, list) and all(isinstance(s, str) for s in strings)
        tensors = [torch.IntTensor(index) for index in self.str2idx(strings)]
        return {"targets": tensors, "flatten_targets": torch.cat(tensors),
                "target_lengths": torch.IntTensor([len(t) for t in tensors])}

    @staticmethod
    def _decode_lens(img_metas, T):
        return [min(T, math.ceil(T * m.get("valid_ratio", 1.0))) for m in img_metas]

    def _scan(self, output, img_metas):
        """-> (idx (N, T) int with -1 at dropped positions, score (N, T) float32) on the host.  A GPU tensor: arg-max,
        softmax probability and the scan in one kernel and ONE device->host copy; a CPU tensor: ctc.py:110-129 with
        torch's softmax and topk."""
        lens = self._decode_lens(img_metas, output.size(1))
        output = output.detach()
        if output.is_cuda:
            return ops.crnn_ctc_decode(output.float(), lens, self.blank_idx)
        value, index = Fn.softmax(output, dim=2).topk(1, dim=2)
        pred, value = index[:, :, 0].numpy(), value[:, :, 0].numpy()
        prev = np.concatenate([np.full((pred.shape[0], 1), self.blank_idx, pred.dtype), pred[:, :-1]], 1)
        keep = (pred != prev) & (pred != self.blank_idx) & (np.arange(pred.shape[1])[None, :] < np.asarray(lens)[:, None])
        return np.where(keep, pred, -1), np.where(keep, value, np.float32(0))

    def tensor2idx(self, output, img_metas, topk=1, return_topk=False):
        """ctc.py:86-143 -> (indexes, scores), or their top-k lists with `return_topk`.  topk == 1 on a GPU tensor runs
        the HIP kernel; topk > 1 follows the reference on the host."""
        assert isinstance(img_metas, list) and all(isinstance(m, dict) for m in img_metas)
        assert len(img_metas) == output.size(0)
        assert isinstance(topk, int) and topk >= 1
        if topk == 1:
            idx, val = self._scan(output, img_metas)
            indexes = [row[row >= 0].tolist() for row in idx]
            scores = [v[row >= 0].astype(np.float64).tolist() for row, v in zip(idx, val)]
            if return_topk:
                return [[[i] for i in r] for r in indexes], [[[s] for s in r] for r in scores]
            return indexes, scores
        lens = self._decode_lens(img_metas, output.size(1))
        prob = Fn.softmax(output.detach().float(), dim=2).cpu()
        batch_value, batch_idx = prob.topk(topk, dim=2)
        indexes_topk, scores_topk = [], []
        for b, decode_len in enumerate(lens):
            pred = batch_idx[b, :, 0].tolist()
            select, prev = [], self.blank_idx
            for t in range(decode_len):
                if pred[t] not in (prev, self.blank_idx):
                    select.append(t)
                prev = pred[t]
            select = torch.LongTensor(select)
            indexes_topk.append(batch_idx[b].index_select(0, select).numpy().tolist())
            scores_topk.append(batch_value[b].index_select(0, select).numpy().tolist())
        if return_topk:
            return indexes_topk, scores_topk
        return [[x[0] for x in r] for r in indexes_topk], [[x[0] for x in r] for r in scores_topk]

    def tensor2str(self, output, img_metas=None):
        """`idx2str(tensor2idx(output, img_metas)[0])` and the scores -> (strings, scores): what `simple_test` needs."""
        if img_metas is None:
            img_metas = [{} for _ in range(output.size(0))]
        indexes, scores = self.tensor2idx(output, img_metas)
        return self.idx2str(indexes), scores


@DETECTORS.register_module()
class CRNNNet(EncodeDecodeRecognizer):
    """`recognizer/crnn.py`: the CTC-loss based recogniser."""

    def set_vgg_train_backend(self, mode):
        """`VeryDeepVgg.set_vgg_train_backend(mode)` of the backbone ("torch" | "hip"): the VGG's training graph on HIP
        kernels, next to `set_train_backend("torch", preprocessor="hip", decoder="hip", loss="hip")` for the other stages.
        A backbone of another type raises.  A call that fails changes nothing."""
        if not isinstance(self.backbone, VeryDeepVgg):
            raise ValueError(f"set_vgg_train_backend: {type(self.backbone).__name__} is not a VeryDeepVgg")
        self.backbone.set_vgg_train_backend(mode)
        return self
