"""TPS++ (attention-enhanced TPS) rectifier behind the reference's BACKBONES API.

Mirror of `mmocr/models/textrecog/backbones/tps_pp/tps_pp.py` + `DGAB.py` (reference): registry
name `TPS_PP` (`tps_pp.py:499-500`; also `TPS_PPv2` in PREPROCESSOR, the name
`preprocessor/__init__.py:6` expects), constructor signature and assertions (`:505-516`), call
contract `forward(batch_img, outs) -> dict(output, logits=None, mp_img, pc_score)` (`:564-625`) and
the 60-entry `state_dict` (58 parameters + buffers `atten_tps.hat_C`, `atten_tps.P_hat`), so
released checkpoints load unchanged.

Every stage of `forward` in eval mode runs on the hand-written HIP kernels of libtpspp_hip.so:
  * the transformation stage -- `Attention_Enhanced_TPS.build_P_prime` + both `F.grid_sample` calls
    (`:597-615`) -- is ONE kernel (T in LDS, grid in registers, arithmetic identical to the reference's
    CPU run);
  * the control-point regressor (MSFA / TPE / DGAB, `:84-325`): MFMA convolutions with everything around
    them fused, the DGAB chain, the score and the per-point FC stacks.
In training mode (`module.train()`) the transformation stage still runs on the HIP kernels in both
directions while the regressor is the plain PyTorch composition of the same layers, so that autograd
reaches its parameters (logged once); `set_train_backend("hip")` puts its convolutions on the HIP forward / backward
kernels (tpspp_conv_bwd.hip), `set_train_backend("hip_all")` every layer of it (tpspp_regressor_bwd.hip for CBAM, DGAB,
the score and the localization FCs).  No CPU fallback: CPU tensors raise.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .precision import default_compute_dtype
from . import constants, ops
from ._prepared import invalidate_prepared, prepared
from .registry import BACKBONES, PREPROCESSOR, TrainBackendMixin


class ConvModule(nn.Module):
    """mmcv.cnn.ConvModule as the reference uses it: `conv` (Conv2d, bias because there is no norm
    layer) followed by `activate` (ReLU, in place on the conv's own output)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride,
                              padding=padding, bias=True)
        self.activate = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.activate(self.conv(x))


class ChannelAttentionModule(nn.Module):
    """`tps_pp.py:27-50` (ratio > 0 branch; the only one instantiated)."""

    def __init__(self, channel, ratio=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.shared_MLP = nn.Sequential(
            nn.Conv2d(channel, channel // ratio, 1, bias=False), nn.ReLU(),
            nn.Conv2d(channel // ratio, channel, 1, bias=False))
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return self.sigmoid(self.shared_MLP(self.avg_pool(x)) + self.shared_MLP(self.max_pool(x)))


class SpatialAttentionModule(nn.Module):
    """`tps_pp.py:53-65`."""

    def __init__(self):
        super().__init__()
        self.conv2d = nn.Conv2d(2, 1, kernel_size=3, stride=1, padding=1)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        avgout = torch.mean(x, dim=1, keepdim=True)
        maxout, _ = torch.max(x, dim=1, keepdim=True)
        return self.sigmoid(self.conv2d(torch.cat([avgout, maxout], dim=1)))


class CBAM(nn.Module):
    """`tps_pp.py:68-82`."""

    def __init__(self, channel, ratio=16):
        super().__init__()
        self.ratio = ratio
        self.channel_attention = ChannelAttentionModule(channel, ratio)
        self.spatial_attention = SpatialAttentionModule()

    def forward(self, x):
        out = self.channel_attention(x) * x
        return self.spatial_attention(out) * out


class Encoder_Decoder_Feature_Extractor(nn.Module):
    """U-Net of `tps_pp.py:84-169`: 4 strided 3x3 encoders, CBAM bottleneck, 4 nearest-upsample +
    3x3 decoders with skip additions."""

    def __init__(self, in_channels=512, num_channels=64, attn_mode="nearest", stride=2,
                 ratio=(1, 1, 1), u_channel=2):
        super().__init__()
        self.stride = stride
        nc = num_channels
        self.k_encoder = nn.Sequential(
            ConvModule(in_channels * u_channel, nc * ratio[0], 3, stride=1, padding=1),
            ConvModule(nc * ratio[0], nc * ratio[1], 3, stride=2, padding=1),
            ConvModule(nc * ratio[1], nc * ratio[2], 3, stride=stride, padding=1),
            ConvModule(nc, nc, 3, stride=(2, 1), padding=1))
        self.atten = CBAM(nc * ratio[2])

        def dec(cin, cout, scale):
            return nn.Sequential(nn.Upsample(scale_factor=scale, mode=attn_mode),
                                 ConvModule(cin, cout, 3, stride=1, padding=1))
        self.k_decoder = nn.Sequential(
            dec(nc, nc, (2, 1)),
            dec(nc * ratio[2], nc * ratio[1], stride),
            dec(nc * ratio[1], nc * ratio[0], 2),
            dec(nc * ratio[0], in_channels, 1))

    def forward(self, k):
        features = []
        for layer in self.k_encoder:
            k = layer(k)
            features.append(k)
        point = features[-1]
        k = self.atten(point)
        n = len(self.k_decoder)
        for i in range(n - 1):
            k = self.k_decoder[i](k)
            k = k + features[n - 2 - i]
        k = self.k_decoder[-1](k)
        return {"decoded_feature": k, "encoded_feature": point}


class Multi_Scale_Fearue_Aggregation(nn.Module):
    """`tps_pp.py:172-229` (class name spelt as in the reference: it is a state_dict-visible name
    only through its attribute `MSFA`, but configs/tools may import it)."""

    def __init__(self, num_img_channel, point_size, p_stride, num_map=2):
        super().__init__()
        self.num_img_channel = num_img_channel
        self.point_x = point_size[1]
        self.point_y = point_size[0]
        self.tf_ratio = 4
        self.conv = Encoder_Decoder_Feature_Extractor(in_channels=num_img_channel, num_channels=64,
                                                      stride=p_stride, u_channel=num_map)
        self.num_fiducial = self.point_y * self.point_x

    def forward(self, batch_img):
        logits = self.conv(batch_img)
        return {"de_feat": logits["decoded_feature"], "en_feat": logits["encoded_feature"]}


class Mlp(nn.Module):
    """`DGAB.py:7-23` (dropout p = 0 is the identity and is omitted)."""

    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class DGAB_Block(nn.Module):
    """Dynamic gated attention of `DGAB.py:25-55`.  `proj` is an nn.Linear applied to a (b,c,h,w)
    tensor, i.e. along W -- valid only because W == dim (kept as is)."""

    def __init__(self, dim, point=8, qkv_bias=False, height=1, width=63):
        super().__init__()
        self.mlp_h = nn.Sequential(nn.Linear(height + point, height + 1, bias=qkv_bias))
        self.mlp_w = nn.Sequential(nn.Linear(width + point, width + 1, bias=qkv_bias))
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, y):
        y = y.transpose(1, 2)                                   # b t c -> b c t
        w = self.mlp_w(torch.cat([x.mean(2), y], 2))
        v_w = w[:, :, :-1].softmax(dim=-1).unsqueeze(2)
        h = self.mlp_h(torch.cat([x.mean(3), y], 2))
        v_h = h[:, :, :-1].softmax(dim=-1).unsqueeze(3)
        x = v_h * x * h[:, :, -1].unsqueeze(-1).unsqueeze(-1) + \
            v_w * x * w[:, :, -1].unsqueeze(-1).unsqueeze(-1)
        return self.proj(x)


class DGAB(nn.Module):
    """`DGAB.py:58-77`: LayerNorm over (H, W), gated attention, MLP along W; drop_path = identity."""

    def __init__(self, dim, mlp_ratio=4.0, width=128, high=32, point=16, qkv_bias=False,
                 skip_lam=1.0):
        super().__init__()
        self.norm1 = nn.LayerNorm([high, width])
        self.attn = DGAB_Block(dim, point=point, width=width, height=high, qkv_bias=qkv_bias)
        self.drop_path = nn.Identity()
        self.norm2 = nn.LayerNorm([high, width])
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio))
        self.skip_lam = skip_lam

    def forward(self, x, y):
        x = x + self.drop_path(self.attn(self.norm1(x), y)) / self.skip_lam
        x = x + self.drop_path(self.mlp(self.norm2(x))) / self.skip_lam
        return x


class Transformation_Parameter_Estimation(nn.Module):
    """`tps_pp.py:231-325`: DGAB, control-point FCs, attention score."""

    def __init__(self, img_channel, point_channel, num_img_channel, point_size, img_size):
        super().__init__()
        self.num_img_channel = num_img_channel
        self.point_x = point_size[1]
        self.point_y = point_size[0]
        self.tf_layers = 1
        self.scale = num_img_channel ** -0.5
        self.without_as = False
        self.num_fiducial = self.point_y * self.point_x
        self.p_linear = nn.Sequential(nn.Linear(point_channel, 32), nn.Linear(32, 64 * 2))
        self.feat_linear = nn.Sequential(nn.Linear(img_channel, 32), nn.Linear(32, 64 * 2))
        self.atten = nn.ModuleList([
            DGAB(dim=num_img_channel, point=self.num_fiducial, width=img_size[1], high=img_size[0])
            for _ in range(self.tf_layers)])
        self.localization_fc1 = nn.Sequential(nn.Linear(num_img_channel, 256), nn.ReLU(True),
                                              nn.Linear(256, 2), nn.ReLU(True))
        self.localization_fc2 = nn.Linear(2 * self.num_fiducial, self.num_fiducial * 2)
        # fc2 starts as "weight 0, bias = initial lattice" (tps_pp.py:277-285)
        self.localization_fc2.weight.data.fill_(0)
        self.localization_fc2.bias.data = torch.from_numpy(
            constants.tpspp_initial_ctrl(point_size)).float().view(-1)

    def atten_score(self, a, b):
        # same dot products as the reference's einsum('bmc,bnc->bmn'), but the result buffer is laid
        # out (N, F, n) and returned as its (N, n, F) transposed VIEW: same shape and values for
        # every consumer, and the warp kernel reads it coalesced (ops.warp detects the stride)
        attn = torch.einsum("bnc,bmc->bnm", b, a)
        attn = attn.mul(self.scale)
        return torch.tanh(attn).transpose(1, 2)

    def get_score(self, point, feat):
        feat = feat.flatten(2).transpose(1, 2)                  # b c h w -> b (h w) c
        pc_score = self.atten_score(self.feat_linear(feat), self.p_linear(point))
        if self.without_as:
            pc_score = torch.zeros_like(pc_score)
        return pc_score

    def forward(self, en_feat, de_feat):
        batch_size = en_feat.size(0)
        en_feat = en_feat.flatten(2).transpose(1, 2)            # b c h w -> b (h w) c
        for atten_layer in self.atten:
            de_feat = atten_layer(de_feat, en_feat)
        control_point = self.localization_fc2(
            self.localization_fc1(en_feat).view(batch_size, -1)).view(batch_size,
                                                                      self.num_fiducial, 2)
        return control_point, self.get_score(en_feat, de_feat)


class Attention_Enhanced_TPS(nn.Module):
    """Constants and grid expansion of `tps_pp.py:328-496`.  `hat_C` IS the inverse of delta_C (the
    reference's buffer name is kept); the per-image `build_inv_delta_C` (:408-435) is dead code there
    and is not reproduced."""

    def __init__(self, rectified_img_size, point_size):
        super().__init__()
        self.eps = constants.EPS
        self.thela = 0.5
        self.point_size = point_size
        self.point_y, self.point_x = point_size[0], point_size[1]
        self.num_fiducial = self.point_y * self.point_x
        self.rectified_img_height = rectified_img_size[0]
        self.rectified_img_width = rectified_img_size[1]
        k = constants.tpspp(rectified_img_size, point_size)
        self.C, self.P = k["C"], k["P"]
        self.register_buffer("hat_C", torch.from_numpy(k["hat_C"]))
        self.register_buffer("P_hat", torch.from_numpy(k["P_hat"]))
        self._P_xy_host = k["P_xy"]

    def device_constants(self, device):
        """(P_xy, P_hat_t) on `device`; P is not a registered buffer in the reference (it does a
        per-call `torch.tensor(self.P).float().to(device)`, tps_pp.py:472): cached here instead."""
        p = self.P_hat
        return prepared(self, "constants", [p],
                        lambda: (torch.from_numpy(self._P_xy_host).to(device), ops.transpose_p_hat(p)), str(device))

    def build_P_prime(self, batch_C_prime, pc_score, device="cuda"):
        """(N,F,2), (N,n,F) -> (N,n,2) sampling grid (`tps_pp.py:481-496`), HIP kernels."""
        P_xy, _ = self.device_constants(batch_C_prime.device)
        T = ops.solve_T(self.hat_C, batch_C_prime)
        return ops.build_grid(self.P_hat, T, P_xy=P_xy, score=pc_score)


@BACKBONES.register_module()
class TPS_PP(TrainBackendMixin, nn.Module):
    """TPS++ rectifier (`tps_pp.py:499-625`).

    Args (as the reference): img_size, rectified_img_size (tuples), num_img_channel, point_size,
        p_stride, visual_point, init_cfg.
    Extra: variant -- the reference has two wirings and hard-codes the one its shipped config cannot run
        (SURVEY.md section 0, fact 4): 'ResNet45v2' (:522: both `outs` at 2x the resolution of `batch_img`) and
        'ResNet45' (:549-552,574-579: `outs[0]` at 2x, `outs[1]` at 1x -- the geometry the backbone strides
        [2,1,2,1,2] of configs/textrecog/nrtr/nrtr_tps++.py produce).  None (default) = pick by geometry: the
        module is built with the reference's hard-coded wiring and re-wires itself
          * when the recogniser that owns it knows its backbone's strides (`EncodeDecodeRecognizer.__init__`),
          * when a checkpoint is loaded (`down0.conv.weight` is (64,32,1,1) in one wiring, (64,32,3,3) in the other),
          * at the first forward whose feature maps have the other geometry, if nothing was loaded yet;
        an explicit value is never overridden.
    """

    def __init__(self, img_size=(16, 64), rectified_img_size=(16, 64), num_img_channel=64,
                 point_size=(2, 16), p_stride=2, visual_point=False, init_cfg=None,
                 variant=None):
        super().__init__()
        assert isinstance(img_size, tuple)
        assert isinstance(rectified_img_size, tuple)
        assert variant in (None, "ResNet45v2", "ResNet45")
        self.init_cfg = init_cfg
        self.heads = 16
        self.variant_explicit = variant is not None
        self._weights_loaded = False
        variant = variant or "ResNet45v2"                     # the reference's hard-coded choice (:522)
        self.type = variant
        # None: follow the input dtype (fp32 -> exact fp32 kernels); torch.bfloat16: bf16 convolutions;
        # "bf16x3": fp32 tensors, three-term bf16 split in the convolutions
        _d = default_compute_dtype()
        self.compute_dtype = _d if _d == "bf16x3" else None      # (bf16: TPS_PP follows its input's dtype)
        self.visual_point = visual_point
        self.num_fiducial = point_size[0] * point_size[1]
        self.img_size = img_size
        self.point_size = point_size
        self.rectified_img_size = rectified_img_size
        self.num_img_channel = num_img_channel
        self.point_channel = num_img_channel
        self.img_channel = num_img_channel
        ic = self.img_channel
        self.MSFA = Multi_Scale_Fearue_Aggregation(num_img_channel, point_size, p_stride, num_map=3)
        # (the reference passes point_channel / img_channel swapped, :240 vs :534; both are 64)
        self.TPE = Transformation_Parameter_Estimation(self.point_channel, self.img_channel,
                                                       num_img_channel, point_size, img_size)
        self.down1 = ConvModule(32, ic, 1)
        self.down2 = ConvModule(64, ic, 1)
        self._wire(variant)
        self.atten_tps = Attention_Enhanced_TPS(rectified_img_size, point_size)
        self._register_load_state_dict_pre_hook(self._variant_from_state_dict)

    def _wire(self, variant):
        """The layers that differ between the two wirings (`tps_pp.py:537-552`); registration order as the reference."""
        ic = self.img_channel
        ref = self.down1.conv.weight
        for name in ("down0", "down0_1", "down1_1", "up_sample", "down_feat"):
            if name in self._modules:
                del self._modules[name]
        if variant == "ResNet45v2":
            new = dict(down0=ConvModule(32, ic, 1), down0_1=ConvModule(ic, ic, 3, stride=2, padding=1),
                       down1_1=ConvModule(ic, ic, 3, stride=2, padding=1),
                       up_sample=nn.Upsample(scale_factor=2, mode="nearest"), down_feat=ConvModule(3 * ic, ic, 1))
        else:
            new = dict(down0=ConvModule(32, ic, 3, stride=2, padding=1))
        for name, mod in new.items():
            setattr(self, name, mod.to(device=ref.device, dtype=ref.dtype))
        # keep the reference's module order (state_dict order): down0, down1, down2, down0_1, down1_1, up_sample, down_feat
        order = ["down0", "down1", "down2", "down0_1", "down1_1", "up_sample", "down_feat"]
        head = [k for k in self._modules if k not in order]        # MSFA, TPE (registered before), atten_tps (after)
        rest = [k for k in order if k in self._modules]
        tail = [k for k in head if k == "atten_tps"]
        head = [k for k in head if k != "atten_tps"]
        for k in head + rest + tail:
            self._modules[k] = self._modules.pop(k)           # re-insert: dicts keep insertion order
        self.type = variant
        invalidate_prepared(self)

    def set_variant(self, variant, explicit=True):
        """Switch the wiring ('ResNet45v2' / 'ResNet45'); the layers the two do not share are re-created with a fresh
        default initialisation (load a checkpoint afterwards)."""
        assert variant in ("ResNet45v2", "ResNet45")
        if variant != self.type:
            self._wire(variant)
        self.variant_explicit = self.variant_explicit or explicit
        return self

    @staticmethod
    def variant_for_strides(strides):
        """The wiring whose feature-map geometry the backbone's first two stage strides produce
        (`resnet_v2_large.py:183-191`: outs[0] = stage-0 input, outs[1] = stage-1 input, x = stage-1 output)."""
        s = [v if isinstance(v, int) else v[0] for v in list(strides)[:2]]
        return {(1, 2): "ResNet45v2", (2, 1): "ResNet45"}.get(tuple(s))

    def _variant_from_state_dict(self, state_dict, prefix, *args):
        w = state_dict.get(prefix + "down0.conv.weight")
        if w is not None and w.dim() == 4:
            want = "ResNet45" if tuple(w.shape[-2:]) == (3, 3) else "ResNet45v2"
            if want != self.type:
                if self.variant_explicit:
                    raise ValueError(f"TPS_PP(variant={self.type!r}): the checkpoint holds the {want!r} wiring "
                                     f"(down0.conv.weight {tuple(w.shape)})")
                self._wire(want)
        # any load -- a partial or regressor-only checkpoint included -- ends the period in which forward() may still
        # re-wire the module (that would replace loaded or about-to-be-trained layers by freshly initialised ones)
        if any(k.startswith(prefix) for k in state_dict):
            self._weights_loaded = True

    def init_weights(self):
        pass

    # ---- debug hook: the regressor's named stages, as the reference's forward hooks see them ----------------
    def regress_stages(self, batch_img, outs):
        """DEBUG / TEST HOOK: `regress()` on the HIP kernels (whatever configuration `compute_dtype` / the input dtype
        select) plus a dict of its intermediate maps as fp32 NCHW tensors, named after the reference modules whose
        forward hooks produce the goldens (`tps_pp.py:156-169`, `DGAB.py:58-77`): `feat_cat` (input of MSFA), `enc0..3`
        (k_encoder.i), `cbam` (atten), `dec0..2_sum` (k_decoder.i output PLUS the skip map -- the upsample and the skip
        addition are fused into the convolution here, so the sum is what exists), `dec3` (= de_feat), `dgab`.  Not used by
        forward(); costs a layout conversion per stage."""
        self._stage_tap = {}
        try:
            cp, sc, fg = self.regress(batch_img, outs)
            st = self._stage_tap
        finally:
            self._stage_tap = None
        return cp, sc, fg, st

    def _tap(self, name, t):
        tap = getattr(self, "_stage_tap", None)
        if tap is None:
            return
        if isinstance(t, (list, tuple)):                     # the concat that feeds k_encoder.0
            tap[name] = torch.cat([(x.nchw() if isinstance(x, ops.Blocked) else x).float() for x in t], dim=1)
        else:
            tap[name] = (t.nchw() if isinstance(t, ops.Blocked) else t).float().clone()

    # ---- hand-written conv path (fp32 MFMA kernels, tps_pp_amd/csrc/tpspp_conv.hip) -------------
    def _conv_weights(self, prep=ops.prep_conv_weight, **kw):
        """{layer name: prep(weight, conv_bias=bias, **kw)} of every conv layer: `ops.prep_conv_weight` (fp32 kernels) or
        `ops.prep_conv_weight_bf16` (kw: x3)."""
        convs = {"down0": self.down0, "down1": self.down1, "down2": self.down2}
        if self.type == "ResNet45v2":
            convs.update(down0_1=self.down0_1, down1_1=self.down1_1, down_feat=self.down_feat)
        for i in range(4):
            convs[f"enc{i}"] = self.MSFA.conv.k_encoder[i]
            convs[f"dec{i}"] = self.MSFA.conv.k_decoder[i][1]
        # (the fp32 kernel's tiled form needs to know where the concatenated sources meet)
        cat = {"src_channels": [64, 64, 64]} if prep is ops.prep_conv_weight else {}
        extra = {"down_feat": cat, "enc0": cat}

        def build():
            return {n: prep(m.conv.weight, conv_bias=m.conv.bias, **kw, **extra.get(n, {})) for n, m in convs.items()}

        return prepared(self, prep.__name__, [t for m in convs.values() for t in (m.conv.weight, m.conv.bias)], build,
                        tuple(kw.items()))

    def _msfa_hip(self, feat_srcs, cw):
        """Encoder_Decoder_Feature_Extractor.forward (`tps_pp.py:156-169`) on the fused conv kernel:
        the concat feeding k_encoder.0, every nn.Upsample and every skip addition are folded into
        the convolutions that consume / produce them."""
        p = self.MSFA.conv.stride
        tap = self._tap
        tap("feat_cat", feat_srcs)
        e0 = ops.conv2d(feat_srcs, cw["enc0"], 1); tap("enc0", e0)
        e1 = ops.conv2d([e0], cw["enc1"], 2); tap("enc1", e1)
        e2 = ops.conv2d([e1], cw["enc2"], p); tap("enc2", e2)
        e3 = ops.conv2d([e2], cw["enc3"], (2, 1)); tap("enc3", e3)
        k = ops.cbam(e3, self.MSFA.conv.atten); tap("cbam", k)
        k = ops.conv2d([(k, 2, 1)], cw["dec0"], 1, residual=e2, res_mode=1); tap("dec0_sum", k)
        k = ops.conv2d([(k, p, p)], cw["dec1"], 1, residual=e1, res_mode=1); tap("dec1_sum", k)
        k = ops.conv2d([(k, 2, 2)], cw["dec2"], 1, residual=e0, res_mode=1); tap("dec2_sum", k)
        k = ops.conv2d([k], cw["dec3"], 1); tap("dec3", k)
        return e3, k

    # ---- bf16 path (BASELINE.json configs[2]): bf16 MFMA convolutions, tpspp_conv_bf16.hip ------------
    def _regress_hip_bf16(self, batch_img, outs, x3=False):
        """The regressor with every convolution on the bf16 matrix cores.  Activations between convolutions
        are bf16 in HBM; the three tensors that feed fp32 arithmetic -- `en_feat` (CBAM, control points:
        amplified ~223x by the TPS solve), `de_feat` (DGAB, score) and `feat_grid` (sampled by the warp) --
        leave their convolution in fp32 (fp32 accumulators, never rounded).  Inputs may be bf16 or fp32."""
        cw = self._conv_weights(ops.prep_conv_weight_bf16, x3=x3)
        f32 = torch.float32
        # x3 ("bf16x3", `compute_dtype = "bf16x3"`): every tensor stays fp32 in HBM and every product is the
        # three-term bf16 split (~5e-6 per layer): the convolutions of the parity-bound (1e-4) path at a third of
        # the fp32 matrix time.  DGAB / score / control points then run on their exact fp32 kernels.
        bf = f32 if x3 else torch.bfloat16
        c16 = (lambda *a, **k: ops.conv2d_bf16(*a, **{"out_dtype": f32, **k})) if x3 else ops.conv2d_bf16
        # the maps that only convolutions read (feat0 / feat1 / feat2, the stride-2 results, the encoder maps and the first
        # three decoder maps) live in the BLOCKED layout (ops.Blocked, bf16; ops.Blocked32, fp32, with x3): a convolution
        # stages such a source with 16-byte loads and no transposition and writes it as 8 / 16-byte pieces of its results
        blk = {"out_blocked": True}
        x, o0, o1 = batch_img, outs[0], outs[1]
        if self.type == "ResNet45v2":
            # feat_grid is sampled by the warp: bf16 when the module boundary is bf16 (the warp then moves half
            # the bytes and rounds once at its store), fp32 when the caller's tensors are fp32
            fg_dtype = bf if x.dtype == bf else f32
            if ops.front_bf16_applicable(o0, o1, x, x3):
                # the four pointwise convolutions fused, register-chained (tpspp_front_bf16.hip)
                fw = prepared(self, "front_bf16", [self.down0, self.down1, self.down2, self.down_feat],
                              lambda: ops.FrontWeightsBf16(self, x3), x3)
                # round 4: feat0 / feat1 are not stored where the stride-2 layers can recompute them from outs[0] / outs[1]
                # (tpspp_down_fused.hip)
                fused = (ops.down_fused_bf16_applicable(o0, cw["down0_1"])
                         and ops.down_fused_bf16_applicable(o1, cw["down1_1"]))
                feat0, feat1, feat2, feat_grid = ops.front_bf16(o0, o1, x, fw, fg_dtype, blocked=True, store01=not fused)
                if fused:
                    cat_srcs = [ops.down_fused_bf16(o0, fw.w0, fw.b0, cw["down0_1"]),
                                ops.down_fused_bf16(o1, fw.w1, fw.b1, cw["down1_1"]), feat2]
            else:
                feat0 = c16([o0], cw["down0"], 1)
                feat1 = c16([o1], cw["down1"], 1)
                feat2 = c16([x], cw["down2"], 1)
                feat_grid = c16([feat0, feat1, (feat2, 2, 2)], cw["down_feat"], 1, out_dtype=fg_dtype)
            if feat0 is not None:
                cat_srcs = [c16([feat0], cw["down0_1"], 2, **blk), c16([feat1], cw["down1_1"], 2, **blk), feat2]
        else:
            # (x may carry its blocked twin -- our backbone's second stage ends on the blocked kernel: ops.Blocked.nchw_hip)
            xb = x if x3 else getattr(x, "_tpspp_blocked", x)
            cat_srcs = [c16([o0], cw["down0"], 2, **blk), c16([o1], cw["down1"], 1, **blk), c16([xb], cw["down2"], 1, **blk)]
            feat_grid = x
        p = self.MSFA.conv.stride
        tap = self._tap
        tap("feat_cat", cat_srcs)
        e0 = c16(cat_srcs, cw["enc0"], 1, **blk); tap("enc0", e0)
        e1 = c16([e0], cw["enc1"], 2, **blk); tap("enc1", e1)
        e2 = c16([e1], cw["enc2"], p, **blk); tap("enc2", e2)
        e3 = c16([e2], cw["enc3"], (2, 1), out_dtype=f32); tap("enc3", e3)
        k = ops.cbam(e3, self.MSFA.conv.atten); tap("cbam", k)
        k = c16([(k, 2, 1)], cw["dec0"], 1, residual=e2, res_mode=1, **blk); tap("dec0_sum", k)
        k = c16([(k, p, p)], cw["dec1"], 1, residual=e1, res_mode=1, **blk); tap("dec1_sum", k)
        k = c16([(k, 2, 2)], cw["dec2"], 1, residual=e0, res_mode=1, **blk); tap("dec2_sum", k)
        de_feat = c16([k], cw["dec3"], 1, out_dtype=f32); tap("dec3", de_feat)
        control_point, atten_score = self._tpe_hip(e3, de_feat, bf16=True, x3=x3)
        return control_point, atten_score, feat_grid

    def grid(self, a1, a2, a3):
        return self.down_feat(torch.cat((a1, a2, self.up_sample(a3)), dim=1))

    def regress(self, batch_img, outs):
        """Control points, attention score and the feature map to rectify (`tps_pp.py:572-594`).
        Hand-written kernels only; CPU tensors raise (no fallback)."""
        self._check_geometry(batch_img, outs)
        ops.require_gpu(batch_img, "TPS_PP")
        if self._bf16(batch_img):
            return self._regress_hip_bf16(batch_img, outs)
        if self.compute_dtype == "bf16x3":
            return self._regress_hip_bf16(batch_img.float(), [o.float() for o in outs], x3=True)
        return self._regress_hip(batch_img, outs)

    def _check_geometry(self, batch_img, outs):
        """Pick the wiring by the feature maps' geometry when it was not chosen explicitly and no checkpoint has been
        loaded; otherwise fail with a message that names the way out."""
        h, w = batch_img.shape[-2:]
        g0, g1 = tuple(outs[0].shape[-2:]), tuple(outs[1].shape[-2:])
        want = "ResNet45v2" if (g0, g1) == ((2 * h, 2 * w), (2 * h, 2 * w)) else \
               "ResNet45" if (g0, g1) == ((2 * h, 2 * w), (h, w)) else None
        if want == self.type:
            return
        # never while training (an optimiser / DDP already holds the parameters the re-wiring would orphan) and never
        # after a load: only a fresh, eval-mode module built without `variant` may still follow the feature maps
        if want is not None and not self.variant_explicit and not self._weights_loaded and not self.training:
            import logging
            logging.getLogger("tps_pp_amd").warning(
                "TPS_PP: feature maps %s / %s for a %s input: switching to the %r wiring (freshly initialised layers)",
                g0, g1, (h, w), want)
            self._wire(want)
            return
        raise ValueError(
            f"TPS_PP(variant={self.type!r}) got outs[0], outs[1] at {g0}, {g1} for a {(h, w)} input: 'ResNet45v2' needs "
            f"both at {(2 * h, 2 * w)}, 'ResNet45' needs {(2 * h, 2 * w)} and {(h, w)} (backbone strides [2,1,2,1,2] of "
            "configs/textrecog/nrtr/nrtr_tps++.py produce the latter; the reference itself fails here) -- build with "
            "variant='ResNet45' / call set_variant(), or leave variant unset before loading the checkpoint")

    def accepts_blocked_outs(self):
        """Does this module take `outs[0]` / `outs[1]` as `ops.Blocked` bf16 maps?  Only the 'ResNet45' wiring on the HIP inference
        path, where nothing but the three down convolutions reads them (`_regress_hip_bf16`): our own backbone then keeps its
        first two maps in the layout its convolutions exchange (resnet_v2_large.py: `_run`; round 6).  A foreign backbone hands
        over NCHW tensors as the reference does; both give the same bits."""
        return (self.type == "ResNet45" and not self.training and self.compute_dtype != "bf16x3"
                and getattr(self, "_stage_tap", None) is None)

    def _bf16(self, batch_img):
        """bf16 compute when the caller hands over bf16 activations or sets `compute_dtype`.  The module's
        own parameters and TPS constants stay fp32 (`module.bfloat16()` would round `hat_C`, whose entries
        reach +-223: refused)."""
        if self.atten_tps.hat_C.dtype != torch.float32:
            raise TypeError("TPS_PP: keep the module in float32 (its TPS constants do not survive bf16); bf16 "
                            "compute is selected by a bfloat16 input or `module.compute_dtype = torch.bfloat16`")
        return batch_img.dtype == torch.bfloat16 or self.compute_dtype == torch.bfloat16

    def _regress_torch(self, batch_img, outs):
        """TEST HOOK, never called by forward(): the same layers composed with plain PyTorch ops, so that
        host-side tests can check the mirror's wiring / state_dict against the oracle without a GPU."""
        if self.type == "ResNet45v2":
            feat0 = self.down0(outs[0])
            feat1 = self.down1(outs[1])
            feat2 = self.down2(batch_img)
            feat_cat = torch.cat((self.down0_1(feat0), self.down1_1(feat1), feat2), dim=1)
            feat_grid = self.grid(feat0, feat1, feat2)
        else:
            feat0 = self.down0(outs[0])
            feat1 = self.down1(outs[1])
            feat2 = self.down2(batch_img)
            feat_cat = torch.cat((feat0, feat1, feat2), dim=1)
            feat_grid = batch_img
        logits = self.MSFA(feat_cat)
        control_point, atten_score = self.TPE(logits["en_feat"], logits["de_feat"])
        return control_point, atten_score, feat_grid

    def _regress_hip(self, batch_img, outs):
        cw = self._conv_weights()
        x = batch_img.float().contiguous()
        o0, o1 = outs[0].float().contiguous(), outs[1].float().contiguous()
        if self.type == "ResNet45v2":
            # down0 / down1 / down2 and grid() (cat + Upsample + down_feat) are pointwise: one fused,
            # register-chained MFMA kernel (tpspp_front.hip)
            fw = prepared(self, "front", [self.down0, self.down1, self.down2, self.down_feat],
                          lambda: ops.FrontWeights(self))
            fused = (ops.down_fused_f32_applicable(o0, cw["down0_1"])
                     and ops.down_fused_f32_applicable(o1, cw["down1_1"]))
            feat0, feat1, feat2, feat_grid = ops.front(o0, o1, x, fw, store01=not fused)
            if fused:           # round 4: feat0 / feat1 never reach HBM (tpspp_down_fused.hip, exact-fp32 form)
                d0 = ops.down_fused_f32(o0, fw.w0, fw.b0, cw["down0_1"])
                d1 = ops.down_fused_f32(o1, fw.w1, fw.b1, cw["down1_1"])
            else:
                d0 = ops.conv2d([feat0], cw["down0_1"], 2)
                d1 = ops.conv2d([feat1], cw["down1_1"], 2)
            cat_srcs = [d0, d1, feat2]
        else:
            cat_srcs = [ops.conv2d([o0], cw["down0"], 2), ops.conv2d([o1], cw["down1"], 1),
                        ops.conv2d([x], cw["down2"], 1)]
            feat_grid = x
        en_feat, de_feat = self._msfa_hip(cat_srcs, cw)
        control_point, atten_score = self._tpe_hip(en_feat, de_feat)
        return control_point, atten_score, feat_grid

    def _tpe_hip(self, en_feat, de_feat, bf16=False, x3=False):
        """Transformation_Parameter_Estimation.forward (`tps_pp.py:315-325`) with the DGAB block on the
        fused kernels (tpspp_dgab.hip), the per-point FC stacks on tpspp_points.hip and the score on
        tpspp_score.hip: no library kernel is left on the GPU path of the regressor."""
        T = self.TPE
        blk = T.atten[0]
        n = en_feat.size(0)
        if bf16:          # the three Linear layers of the DGAB chain on the bf16 matrix cores
            dw = prepared(self, "dgab_bf16", blk.parameters(), lambda: ops.DgabWeightsBf16(blk, x3), x3)
            de = ops.dgab_bf16(de_feat, en_feat.reshape(n, en_feat.size(1), -1), dw)
        else:
            dw = prepared(self, "dgab", blk.parameters(), lambda: ops.DgabWeights(blk))
            de = ops.dgab(de_feat, en_feat.reshape(n, en_feat.size(1), -1), dw)
        self._tap("dgab", de)
        control_point, p1 = ops.tpe_points(en_feat, T)
        if T.without_as:
            return control_point, torch.zeros((n, de.shape[2] * de.shape[3], T.num_fiducial), device=de.device)
        # (in the bf16 and bf16x3 configurations the score's three products take the three-term split as well: ~5e-6)
        sw = prepared(self, "score", T.feat_linear.parameters(), lambda: ops.ScoreWeights(T.feat_linear))
        return control_point, ops.score(de, p1, sw, T.scale, x3=bf16)

    def rectify(self, feat_grid, batch_img, control_point, atten_score, want_grid=False):
        """The transformation stage alone (`tps_pp.py:597-615`): one fused HIP kernel."""
        at = self.atten_tps
        P_xy, P_hat_t = at.device_constants(batch_img.device)
        out0, out1, grid, _ = ops.warp(feat_grid, control_point, at.hat_C, at.P_hat,
                                       self.rectified_img_size, P_xy=P_xy, score=atten_score,
                                       in1=batch_img, want_grid=want_grid, P_hat_t=P_hat_t)
        return (out0, out1, grid) if want_grid else (out0, out1)

    # ---- training graph of the regressor's convolutions on the HIP kernels (tpspp_conv_bwd.hip) -------------------
    TRAIN_BACKENDS = ("torch", "hip", "hip_all")

    def set_train_backend(self, mode):
        """Which kernels the control-point regressor uses in the training graph (`.train()`, or eval mode with inputs
        that carry gradients): "torch" (default) -- the PyTorch composition of the layers, as the reference runs them;
        "hip" -- every ConvModule on `ops.conv2d_autograd` (HIP forward and backward, the concatenation and nearest
        upsampling in front of down_feat / k_encoder.0 / k_decoder folded in), CBAM, DGAB, the TPE layers and the score
        PyTorch; "hip_all" -- the convolutions as "hip" and every other layer on HIP as well (`ops.cbam_autograd`,
        `ops.dgab_autograd`, `ops.tpe_points_autograd`, `ops.score_autograd`).  The warp is `ops.warp_autograd` in all
        three.  Touches neither the parameters, the state_dict nor the eval path."""
        return super().set_train_backend(mode)

    def set_train_io_dtype(self, dtype):
        """Opt-in dtype of the transformation stage in the graph-building forward (`.train()`, or inputs that carry
        gradients).  None (the default): fp32 images, outputs and gradients, as before.  torch.bfloat16: `feat_grid` and
        `batch_img` reach `ops.warp_autograd` as bf16, `output` / `mp_img` come back bf16 and the warp's backward reads and
        writes bf16 (TPSPP_IO_BF16 of tpspp_warp_fwd / tpspp_warp_bwd: no fp32 copy of the maps or their gradients); the
        control-point regressor still gets fp32 inputs and produces fp32 control points and score on every train backend.
        A geometry the bf16 backward does not serve raises at forward with the library's message."""
        if dtype is not None and dtype != torch.bfloat16:
            raise ValueError("set_train_io_dtype: None or torch.bfloat16")
        self._train_io_dtype = dtype
        return self

    @property
    def train_io_dtype(self):
        return getattr(self, "_train_io_dtype", None)

    def _train_conv(self, name, mod, srcs, stride):
        """One ConvModule (conv + in-place ReLU) on `ops.conv2d_autograd`; the forward's weight layouts are cached
        per layer and rebuilt on the device when the parameters change (`_prepared`, which also names the blind spot
        `invalidate_train_cache()` is for)."""
        conv = mod.conv
        if tuple(conv.padding) != ((conv.kernel_size[0] - 1) // 2, (conv.kernel_size[1] - 1) // 2):
            raise ValueError(f"TPS_PP.{name}: the HIP training path needs 'same' padding")
        w, b = conv.weight, conv.bias
        chans = tuple((e if isinstance(e, torch.Tensor) else e[0]).shape[1] for e in srcs)
        cw = prepared(self, ("train", name), [w, b], lambda: ops.prep_conv_weight_device(w, b, list(chans)), chans)
        return ops.conv2d_autograd(srcs, w, b, stride, relu=True, cw=cw)

    def invalidate_train_cache(self):
        """Drop the cached weight layouts of this module's HIP paths (needed only after edits through `param.data`)."""
        return invalidate_prepared(self)

    def _regress_train_hip(self, batch_img, outs, all_hip=False):
        """`_regress_torch` with every ConvModule on the HIP forward / backward kernels: the concatenations, the
        `up_sample` in front of down_feat and the decoder's nn.Upsample are folded into the convolutions; the skip
        additions stay plain tensor adds (the ReLU mask needs each convolution's own output).  all_hip (train backend
        "hip_all"): CBAM and the TPE block on the HIP kernels too (`_tpe_train_hip_all`)."""
        cv = self._train_conv
        x, o0, o1 = batch_img.contiguous(), outs[0].contiguous(), outs[1].contiguous()

        def scale(up):
            f = up.scale_factor
            f = f if isinstance(f, (tuple, list)) else (f, f)
            if up.mode != "nearest" or any(float(v) != int(v) for v in f):
                raise ValueError("TPS_PP: the HIP training path folds integer nearest upsampling only")
            return int(f[0]), int(f[1])

        if self.type == "ResNet45v2":
            feat0 = cv("down0", self.down0, [o0], self.down0.conv.stride)
            feat1 = cv("down1", self.down1, [o1], self.down1.conv.stride)
            feat2 = cv("down2", self.down2, [x], self.down2.conv.stride)
            feat_cat = [cv("down0_1", self.down0_1, [feat0], self.down0_1.conv.stride),
                        cv("down1_1", self.down1_1, [feat1], self.down1_1.conv.stride), feat2]
            uh, uw = scale(self.up_sample)
            feat_grid = cv("down_feat", self.down_feat, [feat0, feat1, (feat2, uh, uw)], self.down_feat.conv.stride)
        else:
            feat_cat = [cv("down0", self.down0, [o0], self.down0.conv.stride),
                        cv("down1", self.down1, [o1], self.down1.conv.stride),
                        cv("down2", self.down2, [x], self.down2.conv.stride)]
            feat_grid = batch_img
        E = self.MSFA.conv
        features = []
        k = feat_cat
        for i, layer in enumerate(E.k_encoder):
            k = cv(f"enc{i}", layer, k if i == 0 else [k], layer.conv.stride)
            features.append(k)
        point = features[-1]
        k = ops.cbam_autograd(point, E.atten) if all_hip else E.atten(point)
        n = len(E.k_decoder)
        for i in range(n):
            up, layer = E.k_decoder[i][0], E.k_decoder[i][1]
            uh, uw = scale(up)
            k = cv(f"dec{i}", layer, [(k, uh, uw)], layer.conv.stride)
            if i < n - 1:
                k = k + features[n - 2 - i]
        control_point, atten_score = self._tpe_train_hip_all(point, k) if all_hip else self.TPE(point, k)
        return control_point, atten_score, feat_grid

    def _tpe_train_hip_all(self, en_feat, de_feat):
        """Transformation_Parameter_Estimation.forward (`tps_pp.py:315-325`) in the training graph, every layer on HIP:
        DGAB (`ops.dgab_autograd`), the localization FCs (`ops.tpe_points_autograd`) and the score (`ops.score_autograd`,
        returned as the transposed view of its (N, F, n) buffer, as the eval path does).  The kernels read the layers'
        parameters in PyTorch's own layout: nothing is prepared from them, so there is no cache to go stale."""
        T = self.TPE
        n, c = en_feat.shape[:2]
        de = de_feat
        for blk in T.atten:
            de = ops.dgab_autograd(de, en_feat.reshape(n, c, -1), blk)
        control_point = ops.tpe_points_autograd(en_feat, T)
        if T.without_as:
            return control_point, torch.zeros((n, de.shape[2] * de.shape[3], T.num_fiducial), device=de.device)
        return control_point, ops.score_autograd(de, en_feat, T).transpose(1, 2)

    def _forward_autograd(self, batch_img, outs, warp_img=None):
        """Training graph: the transformation stage runs on the HIP kernels in both
        directions (`ops.warp_autograd`: tpspp_warp_fwd / tpspp_warp_bwd); the control-point regressor is the
        composition of the same layers, its convolutions on PyTorch's kernels (train backend "torch", the default) or
        on the HIP forward / backward kernels (`set_train_backend("hip")`), so autograd reaches its parameters.  GPU
        tensors only.  `warp_img` (set_train_io_dtype(torch.bfloat16)): the caller's image in bf16; the warp then takes it
        and a bf16 `feat_grid`, the regressor above still ran on the fp32 `batch_img`."""
        ops.require_gpu(batch_img, "TPS_PP")
        if self.train_backend in ("hip", "hip_all"):
            control_point, atten_score, feat_grid = self._regress_train_hip(batch_img, outs,
                                                                             all_hip=self.train_backend == "hip_all")
        else:
            control_point, atten_score, feat_grid = self._regress_torch(batch_img, outs)
        at = self.atten_tps
        P_xy, P_hat_t = at.device_constants(batch_img.device)
        if warp_img is not None:
            feat_grid, batch_img = feat_grid.to(warp_img.dtype), warp_img
        else:
            feat_grid, batch_img = feat_grid.float(), batch_img.float()
        output, mp_img = ops.warp_autograd(feat_grid, control_point.float(), at.hat_C, at.P_hat,
                                           self.rectified_img_size, P_xy=P_xy, score=atten_score.float(),
                                           in1=batch_img, P_hat_t=P_hat_t)
        return {"output": output, "logits": None, "mp_img": mp_img, "pc_score": atten_score}

    def _inputs_want_grad(self, batch_img, outs):
        """Eval mode under enabled autograd: do the inputs carry gradients (then the result must too), and if only the
        parameters do, say once that the HIP path returns detached tensors."""
        if not torch.is_grad_enabled():
            return False
        if batch_img.requires_grad or any(o.requires_grad for o in outs):
            return True
        if not getattr(self, "_warned_detached", False) and any(p.requires_grad for p in self.parameters()):
            import logging
            logging.getLogger("tps_pp_amd").warning(
                "TPS_PP in eval mode with autograd enabled: the HIP inference path records no graph, so no gradient will "
                "reach this module's parameters (call .train(), or wrap inference in torch.no_grad())")
            self._warned_detached = True
        return False

    def forward(self, batch_img, outs, **kwargs):
        """batch_img (N,64,16,64), outs = [stage-0 input, stage-1 input] ->
        dict(output, logits=None, mp_img, pc_score)."""
        wants_graph = self.training or self._inputs_want_grad(batch_img, outs)
        if wants_graph:
            # training graph, or an eval-mode module whose inputs carry gradients (frozen-BN fine-tuning of the layers
            # upstream, saliency / adversarial gradients w.r.t. the image): the reference is differentiable in eval mode
            # too.  Plain eval inference takes the HIP kernels (they record no autograd graph).
            if not getattr(self, "_logged_autograd", False):
                import logging
                if self.train_backend == "hip_all":
                    logging.getLogger("tps_pp_amd").warning(
                        "TPS_PP.train(): control-point regressor with every layer on the HIP forward / backward kernels "
                        "(convolutions, CBAM, DGAB, the localization FCs and the score); warp forward / backward on the HIP "
                        "kernels. Call .eval() for the all-HIP inference path.")
                elif self.train_backend == "hip":
                    logging.getLogger("tps_pp_amd").warning(
                        "TPS_PP.train(): control-point regressor with its convolutions on the HIP forward / backward "
                        "kernels (CBAM, DGAB, TPE and the score as PyTorch compositions); warp forward / backward on the "
                        "HIP kernels. Call .eval() for the all-HIP inference path.")
                else:
                    logging.getLogger("tps_pp_amd").warning(
                        "TPS_PP.train(): control-point regressor as a PyTorch composition (library kernels, fp32) so that "
                        "autograd reaches its parameters; warp forward / backward on the HIP kernels. Call .eval() for the "
                        "all-HIP inference path (or set_train_backend(\"hip\") for the convolutions of training).")
                self._logged_autograd = True
            self._check_geometry(batch_img, outs)
            if self.train_io_dtype is not None:
                return self._forward_autograd(batch_img.float(), [o.float() for o in outs],
                                              warp_img=batch_img.to(self.train_io_dtype))
            return self._forward_autograd(batch_img.float(), [o.float() for o in outs])
        control_point, atten_score, feat_grid = self.regress(batch_img, outs)
        # (the score stays the transposed view of its (N, F, n) buffer: ops.warp reads it in place)
        if batch_img.dtype == torch.bfloat16:
            # bf16 module boundary: the warp reads and writes bf16 planes
            output, mp_img = self.rectify(feat_grid, batch_img, control_point.float(), atten_score.float())
        else:
            output, mp_img = self.rectify(feat_grid.float(), batch_img.float(), control_point.float(),
                                          atten_score.float())
        return {"output": output, "logits": None, "mp_img": mp_img, "pc_score": atten_score}


# `preprocessor/__init__.py:6` of the reference imports a (never released) `TPS_PPv2` into the
# PREPROCESSOR registry; the name is provided so configs referring to it resolve.
PREPROCESSOR.register_module(name="TPS_PPv2", module=TPS_PP)
