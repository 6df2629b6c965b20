"""The recognition losses the NRTR / TPS++ configs name (`loss=dict(type='TFLoss')`, configs/textrecog/nrtr/nrtr_tps++.py:40),
buildable from the same config dicts (reference: `mmocr/models/textrecog/losses/ce_loss.py`, built by
`encode_decode_recognizer.py:68-70` with `ignore_index = label_convertor.padding_idx`).

Only `EncodeDecodeRecognizer.forward_train` -- the training graph of round 5 -- needs them; the cross-entropy itself is
`torch.nn.functional.cross_entropy`, or with `set_train_backend("hip")` the kernels of include/tpspp_train_dec.h
(`ops.seq_cross_entropy_autograd`).  One function does the work; the two registered classes only fix how outputs and
targets are aligned.  Everything else under the reference's `losses/` stays out of scope.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as Fn

from .registry import Registry, TrainBackendMixin

LOSSES = Registry("loss")
_REDUCTIONS = ("none", "mean", "sum")


def sequence_cross_entropy(logits, targets, ignore_index, reduction, shift, flatten):
    """Cross-entropy of (N, T, C) logits against (N, T) class indices.
    shift:   position t is scored against target t + 1 (the targets start with <SOS>: the last output and the first
             target are dropped);
    flatten: score (N T', C) rows against N T' targets, else (N, C, T') against (N, T') -- this only changes the shape of
             an unreduced loss."""
    targets = targets.to(logits.device)
    if shift:
        logits, targets = logits[:, :-1, :], targets[:, 1:]
    if flatten:
        return Fn.cross_entropy(logits.reshape(-1, logits.size(-1)), targets.reshape(-1), ignore_index=ignore_index,
                                reduction=reduction)
    return Fn.cross_entropy(logits.permute(0, 2, 1).contiguous(), targets.contiguous(), ignore_index=ignore_index,
                            reduction=reduction)


class _SequenceLoss(TrainBackendMixin, nn.Module):
    shift_default = False

    def __init__(self, ignore_index, reduction, shift, flatten):
        super().__init__()
        if not isinstance(ignore_index, int) or reduction not in _REDUCTIONS:
            raise AssertionError("ignore_index must be an int, reduction one of " + ", ".join(_REDUCTIONS))
        self.ignore_index, self.reduction, self.shift, self.flatten = ignore_index, reduction, bool(shift), bool(flatten)

    def set_train_backend(self, mode):
        """ "torch" (default): `F.cross_entropy`; "hip": `tpspp_seq_ce_fwd` / `_bwd` for logits on the GPU (logits on the
        host keep PyTorch's)."""
        return super().set_train_backend(mode)

    def forward(self, outputs, targets_dict, img_metas=None):
        """-> {'loss_ce': tensor}; `targets_dict['padded_targets']` (N, T) as `AttnConvertor.str2tensor` builds it."""
        if self.train_backend == "hip" and outputs.is_cuda:
            from . import ops
            return {"loss_ce": ops.seq_cross_entropy_autograd(outputs.float(), targets_dict["padded_targets"],
                                                              self.ignore_index, self.reduction, self.shift, self.flatten)}
        return {"loss_ce": sequence_cross_entropy(outputs, targets_dict["padded_targets"], self.ignore_index,
                                                  self.reduction, self.shift, self.flatten)}


@LOSSES.register_module()
class CELoss(_SequenceLoss):
    """`ignore_first_char=True` aligns output t with target t + 1."""

    def __init__(self, ignore_index=-1, reduction="none", ignore_first_char=False):
        assert isinstance(ignore_first_char, bool)
        super().__init__(ignore_index, reduction, shift=ignore_first_char, flatten=False)


@LOSSES.register_module()
class TFLoss(_SequenceLoss):
    """The transformer recognisers' loss: always shifted; `flatten` (default) scores all positions as one batch."""

    def __init__(self, ignore_index=-1, reduction="none", flatten=True, **kwargs):
        assert isinstance(flatten, bool)
        super().__init__(ignore_index, reduction, shift=True, flatten=flatten)


def build_loss(cfg):
    return LOSSES.build(cfg)


@LOSSES.register_module()
class CTCLoss(TrainBackendMixin, nn.Module):
    """`losses/ctc_loss.py`: `log_softmax` over the classes and `nn.CTCLoss` on (T, N, C); flattened targets by default,
    else targets padded with `blank` and input lengths from the valid ratios; target lengths clamped to 1 .. T.
    -> {'loss_ctc': tensor}.  PyTorch's kernels, or with `set_train_backend("hip")` and logits on the GPU the kernels of
    include/tpspp_crnn_train.h (the `ignore_index` that `EncodeDecodeRecognizer` adds to every loss config is accepted
    and unused, as in the reference)."""

    def __init__(self, flatten=True, blank=0, reduction="mean", zero_infinity=False, **kwargs):
        super().__init__()
        assert isinstance(flatten, bool)
        assert isinstance(blank, int)
        assert isinstance(reduction, str)
        assert isinstance(zero_infinity, bool)
        self.flatten = flatten
        self.blank = blank
        self.ctc_loss = nn.CTCLoss(blank=blank, reduction=reduction, zero_infinity=zero_infinity)

    def set_train_backend(self, mode):
        """ "torch" (default): `log_softmax` + `nn.CTCLoss`; "hip": `tpspp_crnn_ctc_loss_fwd` / `_bwd` on the raw logits
        when they are on the GPU (logits on the host keep PyTorch's)."""
        return super().set_train_backend(mode)

    def _lengths(self, targets_dict, bsz, seq_len, valid_ratios):
        """(target lengths, input lengths) as the reference computes them: int64 on the host."""
        target_lengths = torch.clamp(targets_dict["target_lengths"], min=1, max=seq_len).long()
        input_lengths = torch.full(size=(bsz,), fill_value=seq_len, dtype=torch.long)
        if not self.flatten and valid_ratios is not None:
            input_lengths = torch.Tensor([math.ceil(valid_ratio * seq_len) for valid_ratio in valid_ratios]).long()
        return target_lengths, input_lengths

    def _forward_hip(self, outputs, targets_dict, valid_ratios):
        """The same loss from the raw logits on HIP kernels.  Targets are padded to the longest clamped length; flattened
        targets are cut at the running sums of the clamped lengths, which is how `nn.CTCLoss` reads them."""
        from . import ops
        bsz, seq_len = outputs.size(0), outputs.size(1)
        target_lengths, input_lengths = self._lengths(targets_dict, bsz, seq_len, valid_ratios)
        lens = target_lengths.tolist()
        padded = torch.full((bsz, max(lens, default=0)), self.blank, dtype=torch.int32)
        if self.flatten:
            flat = targets_dict["flatten_targets"].cpu()
            if sum(lens) > flat.numel():
                raise ValueError(f"CTCLoss: the target lengths add up to {sum(lens)}, flatten_targets holds {flat.numel()}")
            start = 0
            for idx, n in enumerate(lens):
                padded[idx, :n] = flat[start:start + n]
                start += n
        else:
            for idx, tensor in enumerate(targets_dict["targets"]):
                valid_len = min(tensor.size(0), seq_len, padded.size(1))
                padded[idx, :valid_len] = tensor[:valid_len]
        return ops.crnn_ctc_loss_autograd(outputs.float(), padded, target_lengths, input_lengths, self.blank,
                                          self.ctc_loss.reduction, self.ctc_loss.zero_infinity)

    def forward(self, outputs, targets_dict, img_metas=None):
        valid_ratios = None
        if img_metas is not None:
            valid_ratios = [img_meta.get("valid_ratio", 1.0) for img_meta in img_metas]
        if self.train_backend == "hip" and outputs.is_cuda:
            return dict(loss_ctc=self._forward_hip(outputs, targets_dict, valid_ratios))
        outputs = torch.log_softmax(outputs, dim=2)
        bsz, seq_len = outputs.size(0), outputs.size(1)
        outputs_for_loss = outputs.permute(1, 0, 2).contiguous()          # (T, N, C)
        if self.flatten:
            targets = targets_dict["flatten_targets"]
        else:
            targets = torch.full(size=(bsz, seq_len), fill_value=self.blank, dtype=torch.long)
            for idx, tensor in enumerate(targets_dict["targets"]):
                valid_len = min(tensor.size(0), seq_len)
                targets[idx, :valid_len] = tensor[:valid_len]
        target_lengths, input_lengths = self._lengths(targets_dict, bsz, seq_len, valid_ratios)
        # (the targets follow the logits' device: PyTorch's own GPU kernel wants them there; a no-op on the host)
        return dict(loss_ctc=self.ctc_loss(outputs_for_loss, targets.to(outputs.device), input_lengths, target_lengths))
