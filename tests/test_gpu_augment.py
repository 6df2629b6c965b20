"""GPU tests of tpspp_augment_normalize_fwd (include/tpspp_augment.h): ResizeOCR, a list of augmentation ops per image and
the normalisation in one launch.  Bit-exactness throughout: against the installed Pillow's own outputs
(tests/golden/augment_pillow.npz) for the pinned codes, against tests/augment_ref.py -- which tests/test_augment_host.py
holds to Pillow -- everywhere else; code 3 (OpenCV's warpAffine) only against its integer restatement: it is UNPINNED.
With the lookup table set to the byte's own value the fp32 output IS the uint8 image the ops produced."""
import numpy as np
import pytest
import torch

import augment_ref as R
from guarded_alloc import guarded
from oracle import resize_oracle as RO
from tps_pp_amd import (NormalizeOCR, OCRBatchPreprocessor, OCRTrainBatchPreprocessor, RandomRotateTextDet, ResizeOCR,
                        TorchVisionWrapper, _lib, ops)

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
Z7 = (0.0,) * 7


def pack_lists(lists, max_ops=8):
    codes = np.zeros((len(lists), max_ops), dtype=np.int32)
    params = np.zeros((len(lists), max_ops, 8), dtype=np.float64)
    for n, lst in enumerate(lists):
        for k, (c, p) in enumerate(lst):
            codes[n, k] = c
            params[n, k, :len(p)] = p
    return codes, params


def launch(dev, imgs, lists, H, W, interpolation=ops.RESIZE_PILLOW, bgr=False, resize_w=None, pad=0, lut=None, max_ops=8,
           put=None):
    """imgs: uint8 (h, w, C) arrays -> the kernel's (N, C, H, W) fp32 output; `lut` None = the byte's own value."""
    put = put or (lambda t: t.to(dev))
    N, C = len(imgs), imgs[0].shape[2]
    sizes = np.array([a.size for a in imgs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    packed = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in imgs]))
    sh = torch.tensor([a.shape[0] for a in imgs], dtype=torch.int32)
    sw = torch.tensor([a.shape[1] for a in imgs], dtype=torch.int32)
    dw = torch.tensor([W] * N if resize_w is None else list(resize_w), dtype=torch.int32)
    if lut is None:
        lut = torch.arange(256, dtype=torch.float32).repeat(C, 1)
    codes, params = pack_lists(lists, max_ops)
    return ops.augment_normalize(put(packed), put(torch.from_numpy(offs)), put(sh), put(sw), put(dw), put(lut.contiguous()),
                                 pad, N, C, H, W, put(torch.from_numpy(codes)), put(torch.from_numpy(params)),
                                 interpolation, bgr)


def as_bytes(out):
    """(N, C, H, W) fp32 of byte values -> (N, H, W, C) uint8 on the host."""
    o = out.cpu()
    assert torch.equal(o, o.round()) and float(o.min()) >= 0 and float(o.max()) <= 255
    return o.permute(0, 2, 3, 1).contiguous().numpy().astype(np.uint8)


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()[1]


def test_every_fixture_case_bit_for_bit(cuda, fixture):
    """One launch per input image of the fixture, one image of the batch per case; RGB order, then the same bytes handed
    over in BGR order with the bgr flag."""
    groups = {}
    for case in fixture:
        groups.setdefault(case[1].tobytes() + bytes(case[1].shape), []).append(case)
    assert len(groups) == 6
    for cases in groups.values():
        img = cases[0][1]
        H, W, C = img.shape
        got = as_bytes(launch(cuda, [img] * len(cases), [c[2] for c in cases], H, W))
        for g, (label, _, _, want) in zip(got, cases):
            assert np.array_equal(g, want), f"{label} on {img.shape}: {(g != want).sum()} bytes differ from Pillow"
        if C == 3:
            flipped = np.ascontiguousarray(img[:, :, ::-1])
            got = as_bytes(launch(cuda, [flipped] * len(cases), [c[2] for c in cases], H, W, interpolation=ops.RESIZE_CV2,
                                  bgr=True))
            for g, (label, _, _, want) in zip(got, cases):
                assert np.array_equal(g[:, :, ::-1], want), f"{label} on {img.shape}, BGR order"


def test_hue_on_all_rgb_triples(cuda):
    """All 2^24 triples through code 7, k = 0 and k = 25: each ONE launch of 2048 images of 64 x 128 x 3."""
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(2048, 64, 128, 3)
    h, s, val = R.rgb_to_hsv(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    imgs = list(rgb)
    for k in (0, 25):
        want = torch.from_numpy(np.stack(R.hsv_to_rgb((h + k) & 255, s, val), 1).astype(np.uint8)).to(cuda)   # (N, 3, H, W)
        out = launch(cuda, imgs, [[(R.HUE, (float(k),) + Z7)]] * 2048, 64, 128, max_ops=1)
        bad = int((out != want.to(torch.float32)).sum())
        assert bad == 0, f"k = {k}: {bad} of {3 << 24} bytes differ from the restatement of Pillow's HSV round trip"


def test_cv2_rotation_equals_its_integer_restatement(cuda):
    """UNPINNED arithmetic: this only shows that the kernel and the restatement of OpenCV's fixed point agree."""
    g = np.random.default_rng(21)
    for shape in ((8, 20, 3), (32, 128, 1), (13, 37, 3)):
        H, W, C = shape
        img = g.integers(0, 256, shape, dtype=np.uint8)
        angles = np.array([-15.0, -7.25, -0.5, 0.0, 0.5, 3.0, 15.0, 90.0, 180.0])
        mats = RandomRotateTextDet.inverse_matrix(angles, H, W)
        lists = [[(R.AFFINE_NEAREST_CV2, tuple(m))] for m in mats]
        got = as_bytes(launch(cuda, [img] * len(lists), lists, H, W))
        for a, gi, lst in zip(angles, got, lists):
            assert np.array_equal(gi, R.apply_ops(img, lst)), (shape, a)
        assert np.array_equal(got[3], img)                       # 0 degrees: the image itself


def mixed_lists(g, N, H, W, C):
    """N op lists of 0..5 ops drawn from the three samplers (and the cv2 rotation), colour ops in random order."""
    ra = TorchVisionWrapper("RandomAffine", degrees=15, translate=(0.3, 0.3), scale=(0.5, 2.), shear=(-45, 45))
    rp = TorchVisionWrapper("RandomPerspective", distortion_scale=0.5, p=1)
    cj = TorchVisionWrapper("ColorJitter", brightness=0.5, saturation=0.5, contrast=0.5, hue=0.1)
    rr = RandomRotateTextDet(max_angle=15)
    lists = []
    for n in range(N):
        lst = [] if n % 5 == 4 else (ra, rp, rr, ra)[n % 4].sample(g, H, W)
        if n % 3 != 1:
            lst = lst + [op for op in cj.sample(g, H, W) if C == 3 or op[0] in (R.BRIGHTNESS, R.CONTRAST)]
        lists.append(lst)
    return lists


@pytest.mark.parametrize("backend,C", [(None, 3), ("pillow", 3), ("pillow", 1)])
def test_ragged_batch_with_mixed_op_lists(cuda, backend, C):
    """Crops of different sizes, resized width below the padded width (pad columns take part in every op), the real
    normalisation table: the resize oracle, then augment_ref, then torch's own ToTensor + Normalize, bit for bit."""
    g = np.random.default_rng(31 + C)
    shapes = [(19, 35), (25, 119), (64, 256), (31, 400), (48, 48), (7, 3), (32, 128), (100, 17), (33, 77), (40, 301), (5, 64)]
    imgs = [g.integers(0, 256, (h, w, C), dtype=np.uint8) for h, w in shapes]
    H, W, pad = 32, 128, 7
    lists = mixed_lists(g, len(imgs), H, W, C)
    assert any(not lst for lst in lists) and max(len(lst) for lst in lists) == (5 if C == 3 else 3)
    mean, std = MEAN[:C], STD[:C]
    want, rw = [], []
    for im, lst in zip(imgs, lists):
        r, p = RO.resize_ocr(im, H, 32, W, True, pad, backend)
        assert r.shape == (H, W, C)
        rw.append(p["resize_w"])
        want.append(RO.to_tensor_normalize(R.apply_ops(r, lst, bgr=True), mean, std))
    assert min(rw) < W
    out = launch(cuda, imgs, lists, H, W, ops.RESIZE_PILLOW if backend == "pillow" else ops.RESIZE_CV2, True, rw, pad,
                 NormalizeOCR(mean, std).table("cpu"))
    got = out.cpu().numpy()
    for n in range(len(imgs)):
        assert np.array_equal(got[n].view(np.uint32), want[n].view(np.uint32)), (n, shapes[n], [c for c, _ in lists[n]])


@pytest.mark.parametrize("backend", [None, "pillow"])
def test_train_preprocessor_against_the_test_preprocessor_and_the_reference(cuda, backend):
    g = np.random.default_rng(41)
    imgs = [g.integers(0, 256, (int(g.integers(5, 70)), int(g.integers(5, 300)), 3), dtype=np.uint8) for _ in range(48)]

    def cfg(*p):
        c = R.train_pipeline(*p)
        next(t for t in c if t["type"] == "ResizeOCR")["backend"] = backend
        return c
    with pytest.warns(UserWarning, match="WITHOUT"):
        off = OCRTrainBatchPreprocessor(cfg(0.0, 0.0), cuda, seed=1, skip=("PyramidRescale", "Albu"))
        on = OCRTrainBatchPreprocessor(cfg(), cuda, seed=1, skip=("PyramidRescale", "Albu"))
    plain = OCRBatchPreprocessor(ResizeOCR(32, min_width=128, max_width=128, keep_aspect_ratio=False,
                                           width_downsample_ratio=0.25, backend=backend), NormalizeOCR(MEAN, STD), cuda)
    a, ma = off(imgs)
    b, mb = plain(imgs)
    assert torch.equal(a, b) and a.shape == (48, 3, 32, 128)                # probabilities 0: the test pipeline's bits
    assert all(m["augment_ops"] == [] and {k: v for k, v in m.items() if k != "augment_ops"} == q for m, q in zip(ma, mb))
    c, mc = on(imgs)
    applied = [m["augment_ops"] for m in mc]
    assert sum(bool(lst) for lst in applied) > 10
    for n, (im, lst) in enumerate(zip(imgs, applied)):
        r, _ = RO.resize_ocr(im, 32, 128, 128, False, 0, backend)
        want = RO.to_tensor_normalize(R.apply_ops(r, lst, bgr=True), MEAN, STD)
        assert np.array_equal(c[n].cpu().numpy().view(np.uint32), want.view(np.uint32)), (n, [k for k, _ in lst])


def test_lists_of_one_to_eight_ops_and_short_tables(cuda):
    """The ping-pong parity: the result must come out of the right LDS buffer after any number of ops; a table of fewer
    than 8 slots ends the list at its last slot."""
    g = np.random.default_rng(51)
    img = g.integers(0, 256, (32, 128, 3), dtype=np.uint8)
    ra = TorchVisionWrapper("RandomAffine", degrees=15, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=(-10, 10))
    rp = TorchVisionWrapper("RandomPerspective", distortion_scale=0.3, p=1)
    full = [(R.CONTRAST, (1.4,) + Z7), ra.sample(g, 32, 128)[0], (R.HUE, (12.0,) + Z7), (R.SATURATION, (0.6,) + Z7),
            rp.sample(g, 32, 128)[0], (R.CONTRAST, (0.7,) + Z7), (R.BRIGHTNESS, (1.3,) + Z7),
            (R.AFFINE_NEAREST_CV2, tuple(RandomRotateTextDet.inverse_matrix(np.array([4.0]), 32, 128)[0]))]
    lists = [full[:k] for k in range(9)]
    got = as_bytes(launch(cuda, [img] * 9, lists, 32, 128, bgr=True))
    for k in range(9):
        assert np.array_equal(got[k], R.apply_ops(img, lists[k], bgr=True)), k
    for max_ops in (1, 3):
        got = as_bytes(launch(cuda, [img] * 2, [full[:max_ops], []], 32, 128, bgr=True, max_ops=max_ops))
        assert np.array_equal(got[0], R.apply_ops(img, full[:max_ops], bgr=True)) and np.array_equal(got[1], img)
    # a code outside 1..7 ends the list, and so does a three-channel code on a one-channel image
    grey = img[:, :, :1].copy()
    got = as_bytes(launch(cuda, [grey] * 2, [[(R.BRIGHTNESS, (0.5,) + Z7), (R.HUE, (9.0,) + Z7), (R.CONTRAST, (2.0,) + Z7)],
                                             [(9, Z7), (R.BRIGHTNESS, (0.5,) + Z7)]], 32, 128))
    assert np.array_equal(got[0], R.brightness(grey, 0.5)) and np.array_equal(got[1], grey)


@pytest.mark.parametrize("shape", [(8, 20, 3), (32, 128, 3)])
def test_guard_bands_and_poison_on_a_mixed_batch(cuda, shape):
    """Nothing outside the output written, every element of it written (tests/guarded_alloc.py); inputs between NaN bands."""
    H, W, C = shape
    g = np.random.default_rng(61)
    imgs = [g.integers(0, 256, (int(g.integers(3, 50)), int(g.integers(3, 200)), C), dtype=np.uint8) for _ in range(7)]
    lists = mixed_lists(g, len(imgs), H, W, C)
    rw = [max(1, W - 3 * n) for n in range(len(imgs))]
    with guarded(cuda) as gd:
        out = launch(cuda, imgs, lists, H, W, ops.RESIZE_CV2, True, rw, 3, put=gd.input)
        assert gd.check(out, require_guarded=True) == 1 and not gd.fallthrough
    want = [R.apply_ops(np.concatenate([RO.imresize_bilinear_u8(im, (w, H)), np.full((H, W - w, C), 3, np.uint8)], 1), lst, True)
            for im, lst, w in zip(imgs, lists, rw)]
    assert np.array_equal(as_bytes(out), np.stack(want))


def test_an_image_too_large_for_the_lds_is_refused(cuda):
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    with pytest.raises(_lib.TpsppError, match="do not fit the LDS"):
        launch(cuda, [img], [[]], 256, 512)
    big = as_bytes(launch(cuda, [img + 9], [[(R.BRIGHTNESS, (2.0,) + Z7)]], 100, 273))     # 2 x 81900 bytes: the largest that fits
    assert big.shape == (1, 100, 273, 3) and (big == 18).all()
