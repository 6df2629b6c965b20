"""CPU tests of the train pipeline's augmentation stage (include/tpspp_augment.h, tps_pp_amd/ocr_transforms.py):
tests/augment_ref.py -- the numpy restatement the kernel is held to in tests/test_gpu_augment.py -- reproduces the
installed Pillow's committed outputs (tests/golden/augment_pillow.npz) and the live Pillow bit for bit, its HSV round trip on
all 2^24 triples; the header, the binding table and the shared object agree; argument errors come back as -22 before
anything is launched; the samplers draw from torchvision's / the reference's distributions; what is not implemented is
refused by name, and `skip=` drops it with one warning."""
import ctypes
import itertools
import math
import os
import warnings

import numpy as np
import pytest

import augment_ref as R
from tps_pp_amd import (OCRTrainBatchPreprocessor, OneOfWrapper, RandomRotateTextDet, RandomWrapper, TorchVisionWrapper,
                        _lib, build, ocr_transforms as T, ops)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tpspp_augment.h")
SKIP = ("PyramidRescale", "Albu")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


# ---- the restatement against Pillow ---------------------------------------------------------------------------------------
def test_restatement_equals_the_pillow_fixture_on_every_case(fixture):
    version, cases = fixture
    assert len(cases) >= 120 and version
    seen = set()
    for label, img, ops_, want in cases:
        got = R.apply_ops(img, ops_, bgr=False)
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"{label} on {img.shape}: {(got != want).sum()} bytes differ"
        seen.update(c for c, _ in ops_)
        if "identity" in label:
            assert np.array_equal(want, img), label            # Pillow itself returns the input
    assert seen == {R.AFFINE_NEAREST_PIL, R.PERSPECTIVE_BILINEAR_PIL, R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE}


def test_bgr_order_is_the_rgb_result_with_the_channels_flipped(fixture):
    for label, img, ops_, want in fixture[1]:
        if img.shape[2] == 3 and ("chain" in label or "saturation" in label or "hue" in label or "contrast" in label):
            got = R.apply_ops(np.ascontiguousarray(img[:, :, ::-1]), ops_, bgr=True)
            assert np.array_equal(got[:, :, ::-1], want), label


def test_restatement_and_fixture_equal_the_live_pillow(fixture):
    pytest.importorskip("PIL")
    import make_augment_golden as MG
    for label, img, ops_, want in fixture[1]:
        assert np.array_equal(MG.pillow_apply(img, ops_), want), f"{label}: the installed Pillow no longer gives the fixture"
    g = np.random.default_rng(5)
    img = g.integers(0, 256, (13, 37, 3), dtype=np.uint8)
    ra = TorchVisionWrapper("RandomAffine", degrees=15, translate=(0.3, 0.3), scale=(0.5, 2.), shear=(-45, 45))
    rp = TorchVisionWrapper("RandomPerspective", distortion_scale=0.5, p=1)
    cj = TorchVisionWrapper("ColorJitter", brightness=0.5, saturation=0.5, contrast=0.5, hue=0.1)
    for t in (ra, rp, cj):
        for _ in range(20):
            ops_ = t.sample(g, 13, 37)
            assert np.array_equal(R.apply_ops(img, ops_), MG.pillow_apply(img, ops_)), ops_


def test_hsv_round_trip_equals_pillow_on_all_triples():
    Image = pytest.importorskip("PIL.Image")
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    hsv = np.array(Image.fromarray(rgb).convert("HSV"))
    h, s, val = R.rgb_to_hsv(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    assert np.array_equal(np.stack([h, s, val], -1), hsv)
    back = np.array(Image.frombytes("HSV", (4096, 4096), rgb.tobytes()).convert("RGB"))
    r, g, b = R.hsv_to_rgb(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    assert np.array_equal(np.stack([r, g, b], -1), back)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------
def test_header_names_what_it_replaces_and_its_codes_are_the_python_ones():
    text = open(HEADER).read()
    assert "replaces:" in text and "UNPINNED" in text and "crnn_pp_pipeline.py:2-84" in text
    for k, code in (("END", 0), ("AFFINE_NEAREST_PIL", 1), ("PERSPECTIVE_BILINEAR_PIL", 2), ("AFFINE_NEAREST_CV2", 3),
                    ("BRIGHTNESS", 4), ("CONTRAST", 5), ("SATURATION", 6), ("HUE", 7)):
        assert getattr(ops, "AUG_" + k) == getattr(R, k) == code
        assert any(line.split()[:3] == ["#define", "TPSPP_AUG_" + k, str(code)] for line in text.splitlines()), k


def test_argument_errors_are_codes_with_messages_and_launch_nothing(lib):
    """Every call names host memory (or nothing) as its operands: a launch would fail loudly, a -22 launches none."""
    keep = (ctypes.c_double * 64)()
    p = ctypes.cast(keep, ctypes.c_void_p).value
    err = lib.tpspp_last_error
    ptrs = ("src", "off", "sh", "sw", "dw", "lut", "out", "codes", "params")

    def call(N=1, C=3, H=32, W=128, pad=0, interp=0, max_ops=8, bgr=1, **null):
        a = {k: (None if null.get(k) is None and k in null else p) for k in ptrs}
        return lib.tpspp_augment_normalize_fwd(a["src"], a["off"], a["sh"], a["sw"], a["dw"], a["lut"], pad, N, C, H, W,
                                               a["out"], interp, a["codes"], a["params"], max_ops, bgr, None)

    for k in ptrs:
        assert call(**{k: None}) == -22 and b"null pointer" in err(), k
    for bad in (-1, 2):
        assert call(interp=bad) == -22 and b"interpolation" in err(), bad
    for kw in (dict(C=0), dict(C=2), dict(C=4), dict(H=0), dict(W=-3), dict(pad=256), dict(pad=-1), dict(N=-1)):
        assert call(**kw) == -22 and b"bad sizes" in err(), kw
    for bad in (0, -1, 9):
        assert call(max_ops=bad) == -22 and b"max_ops" in err(), bad
    # two images (each rounded up to 16 bytes) and 16 bytes more must fit 160 KB of LDS: 2 * 81904 + 16 = 163824 does
    assert call(N=0, H=1, W=27301) == 0
    for kw in (dict(H=1, W=27302), dict(H=256, W=512), dict(C=1, H=1, W=81905), dict(N=0, H=4096, W=4096)):
        assert call(**kw) == -22 and b"do not fit the LDS" in err(), kw
    assert call(N=0, C=1, H=1, W=81904) == 0
    assert call(N=0) == 0                                       # an empty batch: nothing to launch
    del keep


def test_the_python_wrapper_has_no_cpu_fallback_and_checks_before_it_calls():
    import torch
    z = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(_lib.TpsppError, match="packed must be a GPU tensor"):
        ops.augment_normalize(z, z, z, z, z, z, 0, 1, 3, 32, 128, z, z)
    with pytest.raises(ValueError, match="interpolation"):
        ops.augment_normalize(z, z, z, z, z, z, 0, 1, 3, 32, 128, z, z, interpolation=2)


# ---- the samplers -----------------------------------------------------------------------------------------------------------
def _scalar_inverse_affine(center, angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix, scalar by scalar."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [x / scale for x in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def test_random_affine_draws_and_matrix():
    t = TorchVisionWrapper("RandomAffine", degrees=15, translate=(0.3, 0.3), scale=(0.5, 2.), shear=(-45, 45))
    H, W, N = 32, 128, 4000
    angle, (tx, ty), scale, (shx, shy) = t.transform.get_params(np.random.default_rng(1), N, H, W)
    assert angle.min() >= -15 and angle.max() <= 15 and angle.min() < -14 and angle.max() > 14
    assert np.array_equal(tx, np.round(tx)) and np.array_equal(ty, np.round(ty))              # integers
    assert np.abs(tx).max() <= round(0.3 * W) and np.abs(ty).max() <= round(0.3 * H) and np.abs(tx).max() >= 36
    assert scale.min() >= 0.5 and scale.max() <= 2.0 and scale.max() > 1.9
    assert shx.min() >= -45 and shx.max() <= 45 and not shy.any()                             # x-shear only
    assert abs(angle.mean()) < 1.0 and abs(scale.mean() - 1.25) < 0.05 and abs(shx.mean()) < 3.0
    m = T._get_inverse_affine_matrix((W * 0.5, H * 0.5), angle, (tx, ty), scale, (shx, shy))
    for i in range(0, N, 400):
        want = _scalar_inverse_affine((W * 0.5, H * 0.5), angle[i], (tx[i], ty[i]), scale[i], (shx[i], shy[i]))
        assert np.allclose(m[i], want, rtol=1e-13, atol=1e-11)
    codes, params = t.sample_batch(np.random.default_rng(1), N, H, W)
    assert (codes == R.AFFINE_NEAREST_PIL).all() and np.array_equal(params[:, 0, :6], m) and not params[:, 0, 6:].any()


def test_random_perspective_draws_and_coefficients():
    t = TorchVisionWrapper("RandomPerspective", distortion_scale=0.5, p=1)
    H, W, N = 32, 128, 2000
    start, end = t.transform.get_params(np.random.default_rng(2), N, H, W)
    bw, bh = int(0.5 * (W // 2)), int(0.5 * (H // 2))
    assert np.array_equal(start, [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]])
    for corner, (xl, xh), (yl, yh) in ((0, (0, bw), (0, bh)), (1, (W - bw - 1, W - 1), (0, bh)),
                                       (2, (W - bw - 1, W - 1), (H - bh - 1, H - 1)), (3, (0, bw), (H - bh - 1, H - 1))):
        x, y = end[:, corner, 0], end[:, corner, 1]
        assert x.min() == xl and x.max() == xh and y.min() == yl and y.max() == yh, corner      # both ends are reached
        assert np.array_equal(x, np.round(x))
    co = t.transform.coeffs(start, end)
    x, y = end[:, :, 0], end[:, :, 1]
    den = co[:, 6:7] * x + co[:, 7:8] * y + 1
    assert np.allclose((co[:, 0:1] * x + co[:, 1:2] * y + co[:, 2:3]) / den, start[None, :, 0], atol=1e-8)
    assert np.allclose((co[:, 3:4] * x + co[:, 4:5] * y + co[:, 5:6]) / den, start[None, :, 1], atol=1e-8)
    codes, _ = TorchVisionWrapper("RandomPerspective", distortion_scale=0.5, p=0.3).sample_batch(np.random.default_rng(3), N, H, W)
    assert set(np.unique(codes)) == {0, R.PERSPECTIVE_BILINEAR_PIL} and abs((codes != 0).mean() - 0.3) < 0.04


def test_color_jitter_factors_and_uniform_permutation():
    t = TorchVisionWrapper("ColorJitter", brightness=0.5, saturation=0.5, contrast=0.5, hue=0.1)
    N = 4800
    codes, params = t.sample_batch(np.random.default_rng(4), N, 32, 128)
    assert codes.shape == (N, 4) and (np.sort(codes, axis=1) == [4, 5, 6, 7]).all()
    counts = {perm: 0 for perm in itertools.permutations((4, 5, 6, 7))}
    for row in codes:
        counts[tuple(row)] += 1
    # 24 orders, 200 expected each, sigma = 13.8: +-60 is 4.3 sigma
    assert all(140 <= c <= 260 for c in counts.values()), counts
    f = params[:, :, 0]
    blend = f[codes != R.HUE]
    assert blend.min() >= 0.5 and blend.max() <= 1.5 and blend.min() < 0.51 and blend.max() > 1.49
    k = f[codes == R.HUE]
    assert np.array_equal(k, np.round(k)) and set(np.unique(k)) == set(range(0, 26)) | set(range(231, 256))
    assert R.hue_k(-0.1) == 231 and R.hue_k(0.1) == 25 and R.hue_k(0.0) == 0
    only = TorchVisionWrapper("ColorJitter", brightness=0.2).sample_batch(np.random.default_rng(4), 50, 32, 128)[0]
    assert ((only != 0).sum(1) == 1).all() and set(np.unique(only)) == {0, R.BRIGHTNESS}       # the other three are off


def test_rotate_matrix_is_the_inverse_of_the_rotation_about_the_centre():
    t = RandomRotateTextDet(max_angle=15)
    H, W = 32, 128
    codes, params = t.sample_batch(np.random.default_rng(6), 500, H, W)
    assert (codes == R.AFFINE_NEAREST_CV2).all()
    ang = RandomRotateTextDet.sample_angle(np.random.default_rng(7), 15, 2000)
    assert ang.min() >= -15 and ang.max() < 15 and ang.min() < -14.9 and ang.max() > 14.9
    for a in (-15.0, -3.3, 0.0, 7.0, 15.0):
        al, be = math.cos(math.radians(a)), math.sin(math.radians(a))
        M = np.array([[al, be, (1 - al) * W / 2 - be * H / 2], [-be, al, be * W / 2 + (1 - al) * H / 2], [0, 0, 1]])
        assert np.allclose(RandomRotateTextDet.inverse_matrix(np.array([a]), H, W)[0], np.linalg.inv(M)[:2].reshape(-1),
                           rtol=1e-12, atol=1e-10)
    none, _ = RandomRotateTextDet(rotate_ratio=0.0).sample_batch(np.random.default_rng(6), 100, H, W)
    assert not none.any()


def test_wrappers_follow_their_probabilities():
    N = 6000
    one = OneOfWrapper([dict(type="RandomRotateTextDet", max_angle=15),
                        dict(type="TorchVisionWrapper", op="RandomAffine", degrees=15),
                        dict(type="TorchVisionWrapper", op="RandomPerspective", distortion_scale=0.5, p=1)])
    codes, _ = one.sample_batch(np.random.default_rng(8), N, 32, 128)
    share = np.bincount(codes[:, 0], minlength=4)[1:4] / N
    assert codes.shape == (N, 1) and np.abs(share - 1 / 3).max() < 0.03, share
    for p in (0.0, 0.25, 1.0):
        w = RandomWrapper([dict(type="TorchVisionWrapper", op="ColorJitter", brightness=0.5, hue=0.1)], p=p)
        c, _ = w.sample_batch(np.random.default_rng(9), N, 32, 128)
        ran = (c != 0).any(1)
        assert abs(ran.mean() - p) < 0.02 and ((c != 0).sum(1)[ran] == 2).all(), p
    assert one.sample(np.random.default_rng(1), 32, 128)[0][0] in (1, 2, 3)


def test_constructor_assertions_of_the_reference_and_of_torchvision():
    with pytest.raises(AssertionError):
        RandomWrapper([], p=1.5)
    with pytest.raises(AssertionError):
        OneOfWrapper([])
    with pytest.raises(AssertionError):
        OneOfWrapper(dict(type="RandomRotateTextDet"))
    with pytest.raises(TypeError):
        OneOfWrapper([3])
    with pytest.raises(AssertionError):
        TorchVisionWrapper(3)
    for kw in (dict(degrees=-1), dict(degrees=10, translate=(1.5, 0)), dict(degrees=10, scale=(0, 1)),
               dict(degrees=10, shear=(1, 2, 3))):
        with pytest.raises(ValueError):
            TorchVisionWrapper("RandomAffine", **kw)
    for kw in (dict(hue=0.7), dict(brightness=-0.1), dict(contrast=(2, 1))):
        with pytest.raises(ValueError):
            TorchVisionWrapper("ColorJitter", **kw)


def test_what_is_not_implemented_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="GaussianBlur"):
        TorchVisionWrapper("GaussianBlur", kernel_size=3)
    with pytest.raises(NotImplementedError, match="RandomAffine.*interpolation"):
        TorchVisionWrapper("RandomAffine", degrees=15, interpolation=2)          # PIL's BILINEAR
    with pytest.raises(NotImplementedError, match="RandomPerspective.*interpolation"):
        TorchVisionWrapper("RandomPerspective", interpolation="nearest")
    with pytest.raises(NotImplementedError, match="RandomAffine.*fill"):
        TorchVisionWrapper("RandomAffine", degrees=15, fill=128)
    with pytest.raises(NotImplementedError, match="RandomPerspective.*fill"):
        TorchVisionWrapper("RandomPerspective", fill=(0, 0, 1))
    TorchVisionWrapper("RandomAffine", degrees=15, interpolation=0, fill=0)       # the defaults, spelled out
    TorchVisionWrapper("RandomPerspective", interpolation="bilinear", fill=(0, 0, 0))
    for name in SKIP:
        with pytest.raises(NotImplementedError, match=name):
            T.PIPELINES.build(dict(type=name))
    with pytest.raises(NotImplementedError, match="PyramidRescale"):
        OCRTrainBatchPreprocessor(R.train_pipeline(), "cpu")
    with pytest.raises(NotImplementedError, match="Albu"), pytest.warns(UserWarning, match="WITHOUT PyramidRescale"):
        OCRTrainBatchPreprocessor(R.train_pipeline(), "cpu", skip=("PyramidRescale",))
    with pytest.raises(KeyError, match="Distort"):
        OCRTrainBatchPreprocessor([dict(type="ResizeOCR", height=32, max_width=128), dict(type="Distort"),
                                   dict(type="NormalizeOCR", mean=[0.5], std=[0.5])], "cpu")


def test_skip_drops_the_unpinned_transforms_with_one_warning():
    with pytest.warns(UserWarning, match="WITHOUT Albu, PyramidRescale") as rec:
        pre = OCRTrainBatchPreprocessor(R.train_pipeline(), "cpu", seed=3, skip=SKIP)
    assert len([w for w in rec if "OCRTrainBatchPreprocessor" in str(w.message)]) == 1, [str(w.message) for w in rec]
    assert [type(a).__name__ for a in pre.augments] == ["RandomWrapper"] * 3 and pre.augments[1].transforms == []
    assert pre.resize.height == 32 and pre.resize.max_width == 128 and not pre.resize.keep_aspect_ratio
    assert pre.normalize.mean == [0.485, 0.456, 0.406]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # nothing to skip, nothing to warn about
        cfg = [c for c in R.train_pipeline() if c.get("p") != 0.25 or "ColorJitter" in str(c)]
        OCRTrainBatchPreprocessor(cfg, "cpu", skip=SKIP)
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        pre([np.zeros((8, 8, 3), dtype=np.uint8)])


def test_batch_plan_distribution_reproducibility_and_compaction():
    with pytest.warns(UserWarning):
        a = OCRTrainBatchPreprocessor(R.train_pipeline(), "cpu", seed=3, skip=SKIP)
        b = OCRTrainBatchPreprocessor(R.train_pipeline(), "cpu", seed=3, skip=SKIP)
        c = OCRTrainBatchPreprocessor(R.train_pipeline(), "cpu", seed=4, skip=SKIP)
        off = OCRTrainBatchPreprocessor(R.train_pipeline(0.0, 0.0), "cpu", seed=3, skip=SKIP)
    N = 8000
    ca, pa = a.plan(N, 32, 128)
    cb, pb = b.plan(N, 32, 128)
    assert ca.shape == (N, 8) and pa.shape == (N, 8, 8) and ca.dtype == np.int32 and pa.dtype == np.float64
    assert np.array_equal(ca, cb) and np.array_equal(pa, pb)                   # the same seed: the same plan
    assert not np.array_equal(ca, c.plan(N, 32, 128)[0])
    assert not np.array_equal(ca, a.plan(N, 32, 128)[0])                       # the stream moves on from batch to batch
    assert not off.plan(N, 32, 128)[0].any()                                   # probabilities 0: every list empty
    geo = (ca >= 1) & (ca <= 3)
    assert abs(geo.any(1).mean() - 0.5) < 0.02 and (geo.sum(1) <= 1).all() and (~geo[:, 1:]).all()
    col = ca >= 4
    assert abs(col.any(1).mean() - 0.25) < 0.02 and set(np.unique(col.sum(1))) == {0, 4}
    n = (ca != 0).sum(1)
    assert n.max() == 5 and all((row[:k] != 0).all() and not row[k:].any() for row, k in zip(ca[:200], n[:200]))   # no gaps
    assert not pa[ca == 0].any()
    # a one-channel image: Pillow's Color and hue leave it as it is, the plan drops them
    c1, _ = a.plan(N, 32, 128, C=1)
    assert not np.isin(c1, (R.SATURATION, R.HUE)).any() and np.isin(c1, (R.BRIGHTNESS, R.CONTRAST)).any()
    codes = np.array([[0, 4, 0, 5], [0, 0, 0, 0], [7, 0, 0, 1]], dtype=np.int32)
    params = np.arange(3 * 4 * 8, dtype=np.float64).reshape(3, 4, 8)
    cc, pp = T.compact_plan(codes, params)
    assert cc[:, :2].tolist() == [[4, 5], [0, 0], [7, 1]] and not cc[:, 2:].any()
    assert np.array_equal(pp[0, 0], params[0, 1]) and np.array_equal(pp[0, 1], params[0, 3]) and np.array_equal(pp[2, 1], params[2, 3])
    with pytest.raises(ValueError, match="more than 8"):
        T.compact_plan(np.ones((2, 9), dtype=np.int32), np.zeros((2, 9, 8)))
