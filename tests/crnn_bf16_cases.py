"""VeryDeepVgg's reduced-precision arithmetic restated on the CPU in float64, shared by tests/test_crnn_bf16_host.py and
tests/test_gpu_crnn_bf16.py (a helper module, not a test file): the golden models, the folded weights, and the two routes

  x3    every operand split into hi = bf16(x), lo = bf16(x - hi); a product is hi*hi + hi*lo + lo*hi; float64 accumulation;
        maps are fp32 between the layers;
  bf16  image, weights and every map between the layers rounded to bf16 (where the bf16 route rounds them); float64
        accumulation; the last layer leaves in fp32.

BatchNorm 2 / 4 / 6 is folded first, in fp32, as the product folds it; conv6 is the 2x2 kernel zero-extended to 3x3 at stride
(2, 1), sliced to its first W - 1 columns.  Results are cached per (model, route): the GPU tests read the host test's numbers."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from tps_pp_amd import build_detector

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import crnn_cases as CC  # noqa: E402

POOLS = {0: (2, 2, 0), 1: (2, 2, 0), 3: ((2, 2), (2, 1), (0, 1)), 5: ((2, 2), (2, 1), (0, 1))}     # after conv i
CHANNELS = (64, 128, 256, 256, 512, 512, 512)


def golden():
    return np.load(os.path.join(HERE, "golden", "crnn_tps.npz"))


def build_model(name, device=None):
    m = build_detector(CC.models()[name]).eval()
    sd = CC.state(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m if device is None else m.to(device)


def vgg_input(name, G):
    """What the golden VGG of model `name` reads: the golden rectified images (crnn_tps: `images()` behind the golden
    preprocessor) or `images32()` (crnn: no preprocessor); and the key of its golden features."""
    if name == "crnn_tps":
        return torch.from_numpy(G["rect"]).float(), "feat"
    return torch.from_numpy(CC.images32()), "feat32"


def rb(x):
    """Rounded to bf16, dtype kept."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def folded(vgg):
    """[(w fp32 (Cout, Cin, 3, 3), b fp32 (Cout))] of the seven layers: y = gamma (conv(x) + b - mean) / sqrt(var + eps) +
    beta folded in fp32; conv6 zero-extended (first row and column)."""
    out = []
    for i in range(7):
        conv, bn = getattr(vgg.cnn, f"conv{i}"), getattr(vgg.cnn, f"batchnorm{i}", None)
        w, b = conv.weight.detach().float(), conv.bias.detach().float()
        if i == 6:
            w = F.pad(w, (1, 0, 1, 0))
        if bn is not None:
            scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
            w = w * scale.view(-1, 1, 1, 1)
            b = bn.bias.detach().float() + (b - bn.running_mean.float()) * scale
        out.append((w, b))
    return out


def conv64(x, w, b, stride, x3):
    """One layer in float64 with ReLU: operands as the route delivers them (x3: fp32 values, split here; bf16: already
    rounded)."""
    def c(a, ww):
        return F.conv2d(a.double(), ww.double(), None, stride=stride, padding=1)
    if x3:
        xh, wh = rb(x), rb(w)
        xl, wl = rb(x - xh), rb(w - wh)
        y = c(xh, wh) + c(xh, wl) + c(xl, wh)
    else:
        y = c(x, w)
    return F.relu(y + b.double().view(1, -1, 1, 1))


def vgg64(vgg, img, x3):
    """The whole VGG along one route -> float64 features (N, 512, 1, W / 4 + 1)."""
    fw = folded(vgg)
    x = img.float() if x3 else rb(img.float())
    for i, (w, b) in enumerate(fw):
        y = conv64(x, w if x3 else rb(w), b, (2, 1) if i == 6 else (1, 1), x3)
        if i == 6:
            return y[:, :, :, :x.shape[3] - 1]
        x = y.float() if x3 else rb(y.float())              # the map as it is stored: fp32, or bf16
        if i in POOLS:
            x = F.max_pool2d(x, *POOLS[i])


@functools.lru_cache(maxsize=None)
def route_errors(name):
    """{'x3': max abs error of the x3 route's features against the golden, 'bf16_abs': the same for the bf16 route,
    'bf16_rel': its relative L2 error} on model `name`'s golden batch."""
    G = golden()
    vgg = build_model(name).backbone
    img, key = vgg_input(name, G)
    want = torch.from_numpy(G[key]).double()
    with torch.no_grad():
        e3 = (vgg64(vgg, img, True) - want).abs().max().item()
        d = vgg64(vgg, img, False) - want
    return {"x3": e3, "bf16_abs": d.abs().max().item(), "bf16_rel": (d.norm() / want.norm()).item()}


def layer_shapes(width):
    """[(Cin, H, W)] of the seven layers' inputs for a 1 x 32 x width image."""
    out, c, h, w = [], 1, 32, width
    for i in range(7):
        out.append((c, h, w))
        c = CHANNELS[i]
        if i in (0, 1):
            h, w = h // 2, w // 2
        elif i in (3, 5):
            h, w = h // 2, w + 1
    return out
