"""Writes tests/golden/augment_pillow.npz: the INSTALLED Pillow's own outputs of what the train pipeline's
TorchVisionWrapper transforms do to a PIL image (crnn_pp_pipeline.py:34-47,66-73 through transform_wrappers.py:113-123):

    RandomAffine       Image.transform(size, Image.AFFINE, inverse matrix, Image.NEAREST)
    RandomPerspective  Image.transform(size, Image.PERSPECTIVE, coefficients, Image.BILINEAR)
    ColorJitter        ImageEnhance.Brightness / Contrast / Color (.enhance(factor)) and torchvision's adjust_hue:
                       h, s, v = img.convert('HSV').split(); h += uint8(hue_factor * 255) (wrapping); merge; convert back

on seeded uint8 images, as lists of the op records of include/tpspp_augment.h (code, 8 doubles).  The fixture holds the
Pillow version, the input images, every case's image name and op list, and Pillow's output.  Every time it runs, the script
also asserts that tests/augment_ref.py (the numpy restatement the GPU kernel is held to) reproduces every output bit for
bit.  Code 3 (OpenCV's warpAffine) has no case here: OpenCV is not installed, that code is unpinned.

    python tests/golden/make_augment_golden.py            (needs Pillow; run in the build container)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import augment_ref as R                                         # noqa: E402
from tps_pp_amd import ocr_transforms as T, synth              # noqa: E402

MAX_OPS, OP_PARAMS = 8, 8
BLEND_FACTORS = (0.5, 0.77, 1.0, 1.31, 1.5)
HUE_FACTORS = (-0.1, 0.0, 0.1)


def pillow_apply(img, ops):
    """The op list through the installed Pillow: img (H, W, C) uint8 in RGB order (or one channel) -> the same shape."""
    from PIL import Image, ImageEnhance
    H, W, C = img.shape
    im = Image.fromarray(img[:, :, 0] if C == 1 else img)
    for code, p in ops:
        code = int(code)
        if code == R.END:
            break
        if code == R.AFFINE_NEAREST_PIL:
            im = im.transform((W, H), Image.AFFINE, [float(v) for v in p[:6]], Image.NEAREST)
        elif code == R.PERSPECTIVE_BILINEAR_PIL:
            im = im.transform((W, H), Image.PERSPECTIVE, [float(v) for v in p[:8]], Image.BILINEAR)
        elif code == R.BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(float(p[0]))
        elif code == R.CONTRAST:
            im = ImageEnhance.Contrast(im).enhance(float(p[0]))
        elif code == R.SATURATION:
            im = ImageEnhance.Color(im).enhance(float(p[0]))
        elif code == R.HUE:
            h, s, v = im.convert("HSV").split()
            np_h = ((np.array(h, dtype=np.uint8).astype(np.int64) + int(p[0])) & 255).astype(np.uint8)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert(im.mode)
        else:
            raise ValueError(f"no Pillow counterpart for op code {code}")
    out = np.array(im)
    return out[:, :, None] if C == 1 else out


def images():
    def u8(v):
        return np.ascontiguousarray(np.clip(np.floor(v.astype(np.float64) * 128.0 + 128.0), 0, 255).astype(np.uint8))
    small = u8(synth.dyadic((8, 20, 3), "augment.small", 7))
    color = u8(synth.smooth_image((1, 3, 32, 128), "augment.color", 7)[0].transpose(1, 2, 0))
    # text-like: strokes of the varied image on a flat background (which also keeps the compressed fixture small)
    stroke = np.sort(np.abs(synth.smooth_image((1, 1, 32, 128), "augment.stroke", 7)[0, 0]).reshape(-1))
    mask = np.abs(synth.smooth_image((1, 1, 32, 128), "augment.stroke", 7)[0, 0]) <= stroke[stroke.size // 3]
    color = np.where(mask[:, :, None], color, np.array([201, 180, 163], dtype=np.uint8)).astype(np.uint8)
    noise1 = u8(synth.dyadic((32, 128, 1), "augment.gray", 7))
    gray = np.where(noise1 >= 128, noise1, 0).astype(np.uint8)            # half text-like zeros, half noise
    half = np.where((np.arange(160) % 2 == 0).reshape(8, 20, 1), 10, 11).astype(np.uint8)   # mean of L exactly 10.5
    return {"small": small, "color": color, "gray": gray,
            "grey_const": np.full((32, 128, 3), 77, dtype=np.uint8),
            "half3": np.ascontiguousarray(np.repeat(half, 3, axis=2)), "half1": half}


def _affine(H, W, angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=(0.0, 0.0)):
    one = np.ones(1)
    m = T._get_inverse_affine_matrix((W * 0.5, H * 0.5), angle * one, (translate[0] * one, translate[1] * one), scale * one,
                                     (shear[0] * one, shear[1] * one))[0]
    return (R.AFFINE_NEAREST_PIL, tuple(m) + (0.0, 0.0))


def cases(imgs):
    """-> [(label, image name, [(code, params), ...])]"""
    out = []
    for name in ("small", "color", "gray"):
        H, W, C = imgs[name].shape
        geo = [("affine identity", (R.AFFINE_NEAREST_PIL, (1, 0, 0, 0, 1, 0, 0, 0))),
               ("affine translate (3, -2)", _affine(H, W, translate=(3, -2)))]
        geo += [(f"affine {a:+d} deg", _affine(H, W, angle=a)) for a in (15, -15)]
        geo += [(f"affine scale {s}", _affine(H, W, scale=s)) for s in (0.5, 2.0)]
        geo += [(f"affine shear {s:+d} deg", _affine(H, W, shear=(s, 0.0))) for s in (45, -45)]
        ra = T.TorchVisionWrapper("RandomAffine", degrees=15, translate=(0.3, 0.3), scale=(0.5, 2.), shear=(-45, 45))
        c, p = ra.sample_batch(np.random.default_rng(11), 8, H, W)
        geo += [(f"affine draw {i}", (int(c[i, 0]), tuple(p[i, 0]))) for i in range(8)]
        geo.append(("perspective identity", (R.PERSPECTIVE_BILINEAR_PIL, (1, 0, 0, 0, 1, 0, 0, 0))))
        rp = T.TorchVisionWrapper("RandomPerspective", distortion_scale=0.5, p=1)
        c, p = rp.sample_batch(np.random.default_rng(12), 6, H, W)
        geo += [(f"perspective draw {i}", (int(c[i, 0]), tuple(p[i, 0]))) for i in range(6)]
        out += [(label, name, [op]) for label, op in geo]
        blends = [("brightness", R.BRIGHTNESS), ("contrast", R.CONTRAST)] + ([("saturation", R.SATURATION)] if C == 3 else [])
        for label, code in blends:
            out += [(f"{label} {f}", name, [(code, (f,) + (0.0,) * 7)]) for f in BLEND_FACTORS]
        if C == 3:
            out += [(f"hue {f}", name, [(R.HUE, (float(R.hue_k(f)),) + (0.0,) * 7)]) for f in HUE_FACTORS]
            # one ColorJitter draw in the fixed order saturation, brightness, hue, contrast
            out.append(("ColorJitter chain", name, [(R.SATURATION, (0.8,) + (0.0,) * 7), (R.BRIGHTNESS, (1.2,) + (0.0,) * 7),
                                                    (R.HUE, (float(R.hue_k(0.07)),) + (0.0,) * 7),
                                                    (R.CONTRAST, (1.3,) + (0.0,) * 7)]))
    for code, label in ((R.BRIGHTNESS, "brightness"), (R.CONTRAST, "contrast"), (R.SATURATION, "saturation")):
        out.append((f"constant grey, {label} 1.31", "grey_const", [(code, (1.31,) + (0.0,) * 7)]))
    out.append(("constant grey, hue 0.1", "grey_const", [(R.HUE, (float(R.hue_k(0.1)),) + (0.0,) * 7)]))
    for name in ("half3", "half1"):
        out += [(f"mean L = 10.5, contrast {f}", name, [(R.CONTRAST, (f,) + (0.0,) * 7)]) for f in (0.5, 1.5)]
    return out


def pack_ops(ops):
    codes = np.zeros(MAX_OPS, dtype=np.int32)
    params = np.zeros((MAX_OPS, OP_PARAMS), dtype=np.float64)
    for i, (code, p) in enumerate(ops):
        codes[i] = code
        params[i, :len(p)] = p
    return codes, params


def main():
    import PIL
    imgs = images()
    cs = cases(imgs)
    out = {f"img_{k}": v for k, v in imgs.items()}
    codes, params = zip(*(pack_ops(ops) for _, _, ops in cs))
    for i, (label, name, ops) in enumerate(cs):
        ref = pillow_apply(imgs[name], ops)
        got = R.apply_ops(imgs[name], ops, bgr=False)
        assert np.array_equal(got, ref), f"augment_ref != Pillow on case {i} ({label} on {name}): {(got != ref).sum()} bytes"
        out[f"out{i}"] = ref
    L = R.luma(imgs["half3"], False)
    assert L.sum() * 2 == 21 * L.size and np.array_equal(out[f"out{len(cs) - 4}"], pillow_apply(imgs["half3"], cs[-4][2]))
    out["case_label"] = np.array([c[0] for c in cs])
    out["case_image"] = np.array([c[1] for c in cs])
    out["case_codes"] = np.stack(codes)
    out["case_params"] = np.stack(params)
    out["pillow_version"] = np.array(PIL.__version__)
    path = os.path.join(HERE, "augment_pillow.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cs)} cases, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}; augment_ref == Pillow on all")


if __name__ == "__main__":
    main()
