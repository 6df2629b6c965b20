"""Classic RARE TPS-STN rectifier behind the reference's PREPROCESSOR API.

Mirror of `mmocr/models/textrecog/preprocessor/tps_preprocessor.py` (reference): same registry name,
constructor signature and assertion behaviour (`:37-49`), same sub-module / buffer names, hence the same
`state_dict` keys (`LocalizationNetwork.conv.{0,1,4,5,8,9,12,13}.*`, `LocalizationNetwork.
localization_fc1.0.*`, `LocalizationNetwork.localization_fc2.*`, `GridGenerator.inv_delta_C`,
`GridGenerator.P_hat`), same `forward(batch_img) -> Tensor`.

What differs is underneath: `GridGenerator.build_P_prime` + `F.grid_sample` (`:71-83`) run as ONE
hand-written HIP kernel (`tps_pp_amd/csrc/tpspp_warp.hip` through the C ABI of `include/tpspp.h`), and
the localisation network's convolutions (BatchNorm folded), pooling and FCs run on the hand-written
fp32 MFMA conv / pooling kernels when the module is in eval mode on a GPU.  In the graph-building
forward (`.train()`, or an input that carries gradients) the warp runs on the HIP forward / backward
kernels and the localisation network on PyTorch's layers ("torch", the default) or, with
`set_train_backend("hip")`, on HIP kernels forward and backward (`LocalizationNetwork._forward_train_hip`,
`tps_pp_amd/csrc/tpspp_bn_pool_train.hip`).
There is no PyTorch / CPU fallback for the rectification path: CPU tensors raise.
"""
import numpy as np
import torch
import torch.nn as nn

from . import constants, ops
from ._prepared import invalidate_prepared, prepared
from .precision import default_compute_dtype
from .registry import PREPROCESSOR, TrainBackendMixin


class BasePreprocessor(nn.Module):
    """`preprocessor/base_preprocessor.py:8-13`: identity preprocessor with an `init_cfg` slot."""

    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg

    def init_weights(self):
        pass

    def forward(self, x, **kwargs):
        return x


class LocalizationNetwork(nn.Module):
    """Predicts the fiducial points C' (N, F, 2) from the image (`tps_preprocessor.py:88-156`)."""

    def __init__(self, num_fiducial, num_img_channel):
        super().__init__()
        self.num_fiducial = num_fiducial
        self.num_img_channel = num_img_channel
        self.conv = nn.Sequential(
            nn.Conv2d(num_img_channel, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU(True),
            nn.MaxPool2d(2, 2),
            nn.Conv2d(64, 128, 3, 1, 1, bias=False), nn.BatchNorm2d(128), nn.ReLU(True),
            nn.MaxPool2d(2, 2),
            nn.Conv2d(128, 256, 3, 1, 1, bias=False), nn.BatchNorm2d(256), nn.ReLU(True),
            nn.MaxPool2d(2, 2),
            nn.Conv2d(256, 512, 3, 1, 1, bias=False), nn.BatchNorm2d(512), nn.ReLU(True),
            nn.AdaptiveAvgPool2d(1))
        self.localization_fc1 = nn.Sequential(nn.Linear(512, 256), nn.ReLU(True))
        self.localization_fc2 = nn.Linear(256, num_fiducial * 2)
        # fc2 starts as "weight 0, bias = initial fiducials" (tps_preprocessor.py:130-140)
        self.localization_fc2.weight.data.fill_(0)
        self.localization_fc2.bias.data = torch.from_numpy(
            constants.classic_initial_ctrl(num_fiducial)).float().view(-1)

    def _hip_weights(self, prep=ops.prep_conv_weight, **kw):
        """The four convolutions with their eval-mode BatchNorms folded in, by `ops.prep_conv_weight` (fp32 kernels) or
        `ops.prep_conv_weight_bf16` (kw: x3), rebuilt when a parameter or running statistic changes."""
        pairs = [(self.conv[i], self.conv[i + 1]) for i in (0, 4, 8, 12)]
        return prepared(self, prep.__name__, [m for pair in pairs for m in pair],
                        lambda: [prep(conv.weight, bn=ops.bn_tensors(bn), eps=bn.eps, **kw) for conv, bn in pairs],
                        tuple(kw.items()))

    def _fc_weights(self):
        """The two fully connected layers as 1x1 ConvWeights (`ops.linear`)."""
        fcs = [self.localization_fc1[0], self.localization_fc2]
        return prepared(self, "fc", fcs, lambda: [ops.prep_conv_weight(
            fc.weight.view(fc.out_features, fc.in_features, 1, 1), conv_bias=fc.bias) for fc in fcs])

    def forward(self, batch_img):
        """fp32 MFMA convolutions with BatchNorm folded in, HIP pooling kernels, the two FCs as 1x1
        convolutions over the batch.  No CPU / library-kernel path."""
        ops.require_gpu(batch_img, "LocalizationNetwork", self.training)
        n = batch_img.size(0)
        mode = getattr(self, "compute_dtype", None)
        if mode is None and not hasattr(self, "compute_dtype"):
            mode = default_compute_dtype()
        # (a bf16 image goes to the plain-bf16 convolution as it is: the kernel rounds an fp32 source to bf16 as it stages
        # it, so the widened copy would give the same bits)
        as_is = mode == torch.bfloat16 and batch_img.dtype == torch.bfloat16
        x = batch_img.contiguous() if as_is else batch_img.float().contiguous()
        if mode == torch.bfloat16 or mode == "bf16x3":
            # bf16 configuration: the four convolutions on the bf16 matrix cores (fp32 maps in and out: operands are
            # rounded as they are staged, accumulation / bias / ReLU fp32); pooling and the two FCs stay fp32.
            # "bf16x3": the three-term split of the fp32 operands instead of a plain rounding (within the 1e-4 bar).
            cw = self._hip_weights(ops.prep_conv_weight_bf16, x3=mode == "bf16x3")
            conv = lambda t, w: ops.conv2d_bf16([t], w, 1, True, out_dtype=torch.float32)      # noqa: E731
        else:
            cw = self._hip_weights()
            conv = lambda t, w: ops.conv2d([t], w, 1, True)                                    # noqa: E731
        fc1, fc2 = self._fc_weights()
        for i in range(3):
            x = ops.maxpool2x2(conv(x, cw[i]))
        x = ops.global_avgpool(conv(x, cw[3]))
        x = ops.linear(x, fc1, relu=True)
        return ops.linear(x, fc2, relu=False).view(n, self.num_fiducial, 2)

    def _train_cw(self, i):
        """The forward's weight layouts of convolution `self.conv[i]`, cached and rebuilt on the device when the parameter
        changes (`_prepared`, which also names the blind spot `invalidate_train_cache()` is for)."""
        w = self.conv[i].weight
        return prepared(self, ("train", i), [w], lambda: ops.prep_conv_weight_device(w))

    def invalidate_train_cache(self):
        """Drop the cached weight layouts of this module's HIP paths (needed only after edits through `param.data`)."""
        return invalidate_prepared(self)

    def _forward_train_hip(self, batch_img):
        """`_forward_torch` on the HIP kernels inside an autograd graph (TPSPreprocessor.set_train_backend("hip")): the three
        pooled layers each one `ops.bn_pool_autograd` (convolution, then BatchNorm + ReLU + max-pool in one pass), the
        fourth `ops.bn_stem_autograd`, `ops.global_avgpool_autograd`, and the two FCs on the fp32 GEMM.  Exact fp32
        whatever `compute_dtype` says; every BatchNorm follows its own mode."""
        ops.require_gpu(batch_img, "LocalizationNetwork")
        n = batch_img.size(0)
        x = batch_img.float().contiguous()
        for i in (0, 4, 8):
            x = ops.bn_pool_autograd(x, self.conv[i], self.conv[i + 1], self._train_cw(i), name=f"conv.{i}")
        x = ops.bn_stem_autograd(x, self.conv[12], self.conv[13], self._train_cw(12), name="conv.12")
        x = ops.global_avgpool_autograd(x)
        return ops.two_linear_autograd(x, self.localization_fc1[0], self.localization_fc2).view(n, self.num_fiducial, 2)

    def _forward_torch(self, batch_img):
        """The "torch" train backend and the tests' reference: plain PyTorch composition of the same layers."""
        n = batch_img.size(0)
        feat = self.conv(batch_img).view(n, -1)
        return self.localization_fc2(self.localization_fc1(feat)).view(n, self.num_fiducial, 2)


class GridGenerator(nn.Module):
    """Holds inv_delta_C / P_hat and expands the sampling grid (`tps_preprocessor.py:159-282`)."""

    def __init__(self, num_fiducial, rectified_img_size):
        super().__init__()
        self.eps = constants.EPS
        self.rectified_img_height = rectified_img_size[0]
        self.rectified_img_width = rectified_img_size[1]
        self.num_fiducial = num_fiducial
        k = constants.classic(num_fiducial, rectified_img_size)
        self.C, self.P = k["C"], k["P"]
        self.register_buffer("inv_delta_C", torch.from_numpy(k["inv_delta_C"]))
        self.register_buffer("P_hat", torch.from_numpy(k["P_hat"]))

    def prepared_table(self):
        """(P_hat_t, table_flags) for the current P_hat buffer: the transposed copy the coalesced
        kernels read (with the packed copy of the image-pair kernel behind it when the geometry has one:
        `ops.prepare_mirror_table`), and whether the table has the reference's mirror symmetry (checked
        bitwise, once per buffer version; a checkpoint that loads a different table simply gets 0)."""
        p = self.P_hat

        def build():
            hw = (self.rectified_img_height, self.rectified_img_width)
            if ops.table_mirror_symmetry(p, hw, self.num_fiducial):
                P_hat_t, flags = ops.prepare_mirror_table(p, hw)
                return P_hat_t, flags | ops.TABLE_MIRROR4
            return ops.transpose_p_hat(p), 0

        return prepared(self, "table", [p], build)

    def build_P_prime(self, batch_C_prime, device="cuda"):
        """(N, F, 2) -> (N, n, 2): `bmm(P_hat, bmm(inv_delta_C, [C'; 0]))` as two HIP kernels with the
        reference's summation order (`tps_preprocessor.py:270-282`)."""
        T = ops.solve_T(self.inv_delta_C, batch_C_prime)
        return ops.build_grid(self.P_hat, T)


@PREPROCESSOR.register_module()
class TPSPreprocessor(TrainBackendMixin, BasePreprocessor):
    """Rectification network of RARE (TPS-based STN), `tps_preprocessor.py:24-85`.

    Args:
        num_fiducial (int): number of fiducial points.
        img_size (tuple(int, int)): (H, W) of the input image.
        rectified_img_size (tuple(int, int)): (H_r, W_r) of the rectified image.
        num_img_channel (int): input channels.
        init_cfg (dict or list[dict], optional): kept for config compatibility.
    """

    train_io_dtype = None        # set_train_io_dtype

    def __init__(self, num_fiducial=20, img_size=(32, 100), rectified_img_size=(32, 100),
                 num_img_channel=1, init_cfg=None):
        super().__init__(init_cfg=init_cfg)
        assert isinstance(num_fiducial, int)
        assert num_fiducial > 0
        assert isinstance(img_size, tuple)
        assert isinstance(rectified_img_size, tuple)
        assert isinstance(num_img_channel, int)
        self.num_fiducial = num_fiducial
        self.img_size = img_size
        self.rectified_img_size = rectified_img_size
        self.num_img_channel = num_img_channel
        self.LocalizationNetwork = LocalizationNetwork(num_fiducial, num_img_channel)
        self.GridGenerator = GridGenerator(num_fiducial, rectified_img_size)

    def set_compute_dtype(self, mode):
        """Opt-in precision switch of the eval path (not in the reference: its modules are fp32).
        None (the default): a bf16 input is widened, the output is fp32.
        torch.bfloat16: `forward` returns bf16 -- the image reaches the warp as bf16 (an fp32 input is cast once; T, grid
        and interpolation stay fp32, one rounding at the store) and the localisation network runs its bf16 convolutions.
        "bf16x3": the localisation network's three-term bf16 split only; image in and out stay fp32.
        The training / gradient path stays fp32 in every mode."""
        if not (mode is None or mode == "bf16x3" or mode == torch.bfloat16):
            raise ValueError('set_compute_dtype: None, "bf16x3" or torch.bfloat16')
        self.io_dtype = torch.bfloat16 if mode == torch.bfloat16 else None
        self.LocalizationNetwork.compute_dtype = mode
        return self

    def set_train_io_dtype(self, dtype):
        """Opt-in dtype of the image in the graph-building forward (`.train()`, or an input that carries gradients).
        None (the default): fp32, as before.  torch.bfloat16: the image reaches `ops.warp_autograd` as bf16, the rectified
        image comes back bf16 and the warp's backward reads and writes bf16 (TPSPP_IO_BF16 of tpspp_warp_fwd /
        tpspp_warp_bwd); the localisation network still gets the fp32 image and produces fp32 control points.  A
        geometry the bf16 kernels do not serve raises at forward with the library's message."""
        if dtype is not None and dtype != torch.bfloat16:
            raise ValueError("set_train_io_dtype: None or torch.bfloat16")
        self.train_io_dtype = dtype
        return self

    def set_train_backend(self, mode):
        """Which kernels the localisation network runs on in the graph-building forward (`.train()`, or an input that
        carries gradients): "torch" (default) -- the PyTorch composition of its layers; "hip" --
        `LocalizationNetwork._forward_train_hip`, HIP forward and backward for every layer.  The warp is on the HIP
        kernels either way.  Touches neither the parameters, the buffers, the state_dict nor the eval path."""
        return super().set_train_backend(mode)

    def rectify(self, batch_img, batch_C_prime, want_grid=False, want_idx=False):
        """The hot path alone: control points -> rectified image (fused HIP kernel).  A bfloat16 image gives a bfloat16
        result (needs the prepared table, i.e. a mirror-symmetric P_hat and a geometry that has one)."""
        gg = self.GridGenerator
        P_hat_t, flags = gg.prepared_table()
        out, _, grid, idx = ops.warp(batch_img, batch_C_prime, gg.inv_delta_C, gg.P_hat,
                                     self.rectified_img_size, want_grid=want_grid,
                                     want_idx=want_idx, P_hat_t=P_hat_t, table_flags=flags)
        if want_grid or want_idx:
            return out, grid, idx
        return out

    def forward(self, batch_img):
        """(N, C, H, W) -> (N, C, H_r, W_r)."""
        if self.training or (torch.is_grad_enabled() and batch_img.requires_grad):
            # training graph, or an eval-mode module whose input carries gradients
            # (saliency / adversarial gradients w.r.t. the image: the reference is differentiable in eval mode too):
            # HIP warp forward + backward; the localisation network (fp32) is the plain PyTorch composition or, on the
            # "hip" train backend, its HIP training graph: autograd reaches its parameters either way.  Plain eval
            # inference takes the HIP kernels (no autograd graph).
            ops.require_gpu(batch_img, "TPSPreprocessor")
            hip = self.train_backend == "hip"
            if not hip and not getattr(self, "_logged_autograd", False):
                import logging
                logging.getLogger("tps_pp_amd").warning(
                    "TPSPreprocessor.train(): localisation network as a PyTorch composition (library kernels, fp32); "
                    "warp forward / backward on the HIP kernels. Call .eval() for the all-HIP inference path, "
                    "set_train_backend(\"hip\") for the localisation network's HIP training graph.")
                self._logged_autograd = True
            gg = self.GridGenerator
            P_hat_t, flags = gg.prepared_table()
            loc = self.LocalizationNetwork
            ctrl = loc._forward_train_hip(batch_img) if hip else loc._forward_torch(batch_img.float())
            io = self.train_io_dtype
            return ops.warp_autograd(batch_img.float() if io is None else batch_img.to(io), ctrl.float(), gg.inv_delta_C, gg.P_hat,
                                     self.rectified_img_size, P_hat_t=P_hat_t, table_flags=flags)
        if getattr(self, "io_dtype", None) == torch.bfloat16:
            ops.require_gpu(batch_img, "TPSPreprocessor")
            img = batch_img if batch_img.dtype == torch.bfloat16 else batch_img.to(torch.bfloat16)
            batch_C_prime = self.LocalizationNetwork(img)
            return self.rectify(img, batch_C_prime.float())
        batch_C_prime = self.LocalizationNetwork(batch_img)
        return self.rectify(batch_img.float(), batch_C_prime.float())
