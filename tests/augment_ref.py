"""CPU reference of the seven augmentation codes of include/tpspp_augment.h: a plain numpy restatement, op by op, of what
the train pipeline's transforms do to a uint8 image (a helper module of tests/test_augment_host.py and
tests/test_gpu_augment.py, not a test file).

Codes 1, 2 and 4..7 restate Pillow (Image.transform(AFFINE, NEAREST) / (PERSPECTIVE, BILINEAR), ImageEnhance.Brightness /
Contrast / Color, convert('HSV') and back) and are PINNED: tests/golden/augment_pillow.npz holds the installed Pillow's own
outputs and tests/test_augment_host.py compares bit for bit.  Code 3 restates OpenCV's warpAffine(INTER_NEAREST) and is
UNPINNED: OpenCV is not installed, so nothing here was ever compared with it.

Images are (H, W, C) uint8, C = 1 or 3; `bgr=True` means channel 0 is blue.  fp32 steps are numpy float32 operations, fp64
steps float64: the same IEEE operations the kernel performs, in the same order.
"""
import numpy as np

END, AFFINE_NEAREST_PIL, PERSPECTIVE_BILINEAR_PIL, AFFINE_NEAREST_CV2, BRIGHTNESS, CONTRAST, SATURATION, HUE = range(8)
F32 = np.float32


def _fix16(v):
    return np.int64(np.floor(np.float64(v) * 65536.0 + 0.5))


def _wrap32(v):
    """int64 -> the int32 it wraps to (Pillow accumulates in a C int)."""
    return ((np.asarray(v, dtype=np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def _gather(img, xs, ys):
    """img[ys, xs] where (xs, ys) lies inside, 0 elsewhere."""
    H, W, _ = img.shape
    ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    out = img[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)]
    out[~ok] = 0
    return out


def affine_nearest_pil(img, a):
    H, W, _ = img.shape
    a = [np.float64(v) for v in a[:6]]
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    xx = _wrap32(_fix16(a[2] + a[0] * 0.5 + a[1] * 0.5) + x * _fix16(a[0]) + y * _fix16(a[1]))
    yy = _wrap32(_fix16(a[5] + a[3] * 0.5 + a[4] * 0.5) + x * _fix16(a[3]) + y * _fix16(a[4]))
    return _gather(img, xx >> 16, yy >> 16)


def perspective_bilinear_pil(img, a):
    H, W, _ = img.shape
    a = [np.float64(v) for v in a[:8]]
    xi = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yi = np.arange(H, dtype=np.float64)[:, None] + 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        den = a[6] * xi + a[7] * yi + 1.0
        xin = (a[0] * xi + a[1] * yi + a[2]) / den
        yin = (a[3] * xi + a[4] * yi + a[5]) / den
        inside = ~((xin < 0) | (xin >= W) | (yin < 0) | (yin >= H))        # (a NaN coordinate counts as inside, as in C)
    xin = np.where(inside & np.isfinite(xin), xin, 0.5) - 0.5
    yin = np.where(inside & np.isfinite(yin), yin, 0.5) - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x0)[:, :, None], (yin - y0)[:, :, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    p = img.astype(np.float64)
    r0 = np.clip(y0, 0, H - 1)
    v1 = p[r0, xa] + (p[r0, xb] - p[r0, xa]) * dx
    has = (y0 + 1 >= 0) & (y0 + 1 < H)
    r1 = np.clip(y0 + 1, 0, H - 1)
    v2 = np.where(has[:, :, None], p[r1, xa] + (p[r1, xb] - p[r1, xa]) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.uint8)               # values lie in [0, 255]: the cast truncates
    out[~inside] = 0
    return out


def affine_nearest_cv2(img, m):
    """UNPINNED (see the module docstring)."""
    H, W, _ = img.shape
    m = [np.float64(v) for v in m[:6]]
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    X = (np.rint(m[0] * x * 1024.0).astype(np.int64) + np.rint((m[1] * y + m[2]) * 1024.0).astype(np.int64) + 512) >> 10
    Y = (np.rint(m[3] * x * 1024.0).astype(np.int64) + np.rint((m[4] * y + m[5]) * 1024.0).astype(np.int64) + 512) >> 10
    return _gather(img, X, Y)


def luma(img, bgr):
    """Pillow's RGB -> L on an (H, W, 3) image; a one-channel image is its own L."""
    if img.shape[2] == 1:
        return img[:, :, 0].astype(np.int64)
    v = img.astype(np.int64)
    r, g, b = (v[:, :, 2], v[:, :, 1], v[:, :, 0]) if bgr else (v[:, :, 0], v[:, :, 1], v[:, :, 2])
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def blend(d, p, f):
    """Pillow's ImagingBlend(degenerate d, image p, f) per byte, fp32."""
    f = F32(f)
    d32, p32 = np.asarray(d).astype(F32), np.asarray(p).astype(F32)
    t = d32 + f * (p32 - d32)
    if not (F32(0) <= f <= F32(1)):
        t = np.where(t <= 0, F32(0), np.where(t >= 255, F32(255), t))
    return t.astype(np.int32).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f, bgr=False):
    L = luma(img, bgr)
    mean = int(np.float64(int(L.sum())) / np.float64(L.size) + 0.5)
    return blend(np.full_like(img, mean), img, f)


def saturation(img, f, bgr=False):
    assert img.shape[2] == 3
    L = luma(img, bgr)[:, :, None]
    return blend(np.broadcast_to(L, img.shape), img, f)


def rgb_to_hsv(r, g, b):
    """Pillow's rgb2hsv on integer arrays -> (h, s, v) bytes."""
    r, g, b = (np.asarray(t).astype(np.int64) for t in (r, g, b))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = ((maxc - t).astype(F32) / cr for t in (r, g, b))
        rc64, gc64, bc64 = (t.astype(np.float64) for t in (rc, gc, bc))
        h = np.where(r == maxc, bc64 - gc64, np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(F32)
        x = h.astype(np.float64) / 6.0 + 1.0
        h = (x - np.floor(x)).astype(F32)                      # fmod(x, 1.0) for x > 0
        uh = np.clip(np.nan_to_num(h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        us = np.clip(np.nan_to_num(s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    return np.where(grey, 0, uh), np.where(grey, 0, us), maxc


def hsv_to_rgb(h, s, v):
    """Pillow's hsv2rgb on byte arrays -> (r, g, b)."""
    h, s, v = (np.asarray(t).astype(np.int64) for t in (h, s, v))
    hf = h.astype(np.float64) * 6.0 / 255.0
    fi = np.floor(hf)
    f = (hf - fi).astype(F32).astype(np.float64)
    fs = (s.astype(np.float64) / 255.0).astype(F32).astype(np.float64)
    vd = v.astype(np.float64)

    def rnd(t):
        return np.clip(np.floor(t + 0.5).astype(np.int64), 0, 255)
    p = rnd(vd * (1.0 - fs))
    q = rnd(vd * (1.0 - fs * f))
    t = rnd(vd * (1.0 - fs * (1.0 - f)))
    i = fi.astype(np.int64) % 6
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    grey = s == 0
    return np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)


def hue_rgb(r, g, b, k):
    h, s, v = rgb_to_hsv(r, g, b)
    return hsv_to_rgb((h + int(k)) & 255, s, v)


def hue(img, k, bgr=False):
    assert img.shape[2] == 3
    ch = (2, 1, 0) if bgr else (0, 1, 2)
    r, g, b = hue_rgb(img[:, :, ch[0]], img[:, :, ch[1]], img[:, :, ch[2]], int(k))
    out = np.empty_like(img)
    out[:, :, ch[0]], out[:, :, ch[1]], out[:, :, ch[2]] = r, g, b
    return out


def hue_k(hue_factor):
    """uint8(hue_factor * 255) as torchvision's adjust_hue wraps it."""
    return int(hue_factor * 255) & 255


def load_fixture():
    """tests/golden/augment_pillow.npz -> (Pillow version, [(label, image (H, W, C) in RGB order, ops, Pillow's output)])."""
    import os
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_pillow.npz"))
    cases = []
    for i, (label, name) in enumerate(zip(G["case_label"], G["case_image"])):
        codes, params = G["case_codes"][i], G["case_params"][i]
        ops = [(int(c), tuple(float(v) for v in p)) for c, p in zip(codes, params) if c != END]
        cases.append((str(label), G[f"img_{name}"], ops, G[f"out{i}"]))
    return str(G["pillow_version"]), cases


def train_pipeline(p_geo=None, p_color=None):
    """The reference's train_pipeline (tests/golden/crnn_pp_train_pipeline.json: its settings, as a list of dicts), the
    two probabilities optionally replaced."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crnn_pp_train_pipeline.json")
    with open(path) as f:
        cfg = json.load(f)["train_pipeline"]
    wrappers = [c for c in cfg if c["type"] == "RandomWrapper"]
    assert len(wrappers) == 3
    if p_geo is not None:
        wrappers[0]["p"] = p_geo
    if p_color is not None:
        wrappers[2]["p"] = p_color
    return cfg


def apply_op(img, code, params, bgr=False):
    code = int(code)
    if code == AFFINE_NEAREST_PIL:
        return affine_nearest_pil(img, params)
    if code == PERSPECTIVE_BILINEAR_PIL:
        return perspective_bilinear_pil(img, params)
    if code == AFFINE_NEAREST_CV2:
        return affine_nearest_cv2(img, params)
    if code == BRIGHTNESS:
        return brightness(img, params[0])
    if code == CONTRAST:
        return contrast(img, params[0], bgr)
    if code == SATURATION:
        return saturation(img, params[0], bgr)
    if code == HUE:
        return hue(img, int(params[0]), bgr)
    raise ValueError(f"augment_ref: unknown op code {code}")


def apply_ops(img, ops, bgr=False):
    """ops: iterable of (code, params); a code 0 ends the list."""
    img = np.ascontiguousarray(img)
    for code, params in ops:
        if int(code) == END:
            break
        img = np.ascontiguousarray(apply_op(img, code, params, bgr))
    return img
