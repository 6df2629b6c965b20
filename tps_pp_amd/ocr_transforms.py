"""GPU-side test pipeline of the recogniser: ResizeOCR + ToTensorOCR + NormalizeOCR on a batch (SURVEY.md section 8f,
row F4).

Mirror of `mmocr/datasets/pipelines/ocr_transforms.py:18-156` (reference): `ResizeOCR` keeps the constructor, its
assertions and the per-image host logic (`plan`: resized width, padded width, `valid_ratio`, `resize_shape`,
`pad_shape` exactly as `__call__` computes them, :83-121); the pixel work of the three transforms is ONE HIP kernel
over the whole batch (`tpspp_resize_normalize_fwd`) instead of a per-sample OpenCV / torchvision call in a CPU data
loader.  `OCRBatchPreprocessor` strings them together the way `configs/_base_/recog_pipelines/crnn_pp_pipeline.py:85-95`
does and returns the tensor plus the `img_metas` the recogniser reads (`resize_shape`, `valid_ratio`, ...).

`backend` is honoured as the reference forwards it to `mmcv.imresize` (ocr_transforms.py:34-36,46,65,99-101):
`'pillow'` -> Pillow's `Image.resize(size, Image.BILINEAR)` arithmetic, PINNED bit for bit against the installed Pillow
(tests/golden/resize_pillow.npz); `None` / `'cv2'` -> OpenCV's 8-bit INTER_LINEAR arithmetic, which could not be pinned
against OpenCV itself (not installed at build time): see oracle/resize_oracle.py and DESIGN.md section 4f; anything else
raises `ValueError` when the transform is applied, as `mmcv.imresize` does.  No CPU fallback.

The TRAIN pipeline (`crnn_pp_pipeline.py:2-84`) is here as well: `RandomWrapper`, `OneOfWrapper`, `TorchVisionWrapper`
(`RandomAffine`, `RandomPerspective`, `ColorJitter`) and `RandomRotateTextDet` draw their parameters on the host, and
`OCRTrainBatchPreprocessor` runs resize, the drawn ops and the normalisation of a whole batch as ONE launch of
`tpspp_augment_normalize_fwd` (include/tpspp_augment.h).  The torchvision transforms are Pillow's arithmetic, PINNED bit for
bit (tests/golden/augment_pillow.npz); `RandomRotateTextDet` is OpenCV's, unpinned; `PyramidRescale` and `Albu` are refused
by name.  DESIGN.md section 4f.1.
"""
import math

import numpy as np
import torch

from . import _lib, ops
from .registry import Registry

PIPELINES = Registry("pipeline")


def _is_none_or_type(x, t):
    return x is None or isinstance(x, t)


@PIPELINES.register_module()
class ResizeOCR:
    """`ocr_transforms.py:18-129`: same arguments and assertions; `plan(img_shape)` is the host half of `__call__`."""

    def __init__(self, height, min_width=None, max_width=None, keep_aspect_ratio=True, img_pad_value=0,
                 width_downsample_ratio=1.0 / 16, backend=None):
        assert isinstance(height, (int, tuple))
        assert _is_none_or_type(min_width, (int, tuple))
        assert _is_none_or_type(max_width, (int, tuple))
        if not keep_aspect_ratio:
            assert max_width is not None, '"max_width" must assigned if "keep_aspect_ratio" is False'
        assert isinstance(img_pad_value, int)
        if isinstance(height, tuple):
            assert isinstance(min_width, tuple)
            assert isinstance(max_width, tuple)
            assert len(height) == len(min_width) == len(max_width)
        self.height, self.min_width, self.max_width = height, min_width, max_width
        self.keep_aspect_ratio = keep_aspect_ratio
        self.img_pad_value = img_pad_value
        self.width_downsample_ratio = width_downsample_ratio
        self.backend = backend

    def interpolation(self):
        """`backend` -> the kernel's interpolation code (`mmcv.imresize`: None = the global backend, cv2 by default;
        an unknown name raises ValueError there as well, at call time)."""
        if self.backend in (None, "cv2"):
            return ops.RESIZE_CV2
        if self.backend == "pillow":
            return ops.RESIZE_PILLOW
        raise ValueError(f"backend: {self.backend} is not supported for resize. Supported backends are 'cv2', 'pillow'")

    def _dst(self, rank=0):
        if isinstance(self.height, int):
            return self.height, self.min_width, self.max_width
        idx = rank % len(self.height)          # multi-scale: one (height, width) pair per rank (:76-82)
        return self.height[idx], self.min_width[idx], self.max_width[idx]

    def plan(self, img_shape, rank=0):
        """-> dict(height, resize_w, out_w, valid_ratio, resize_shape, pad_shape) for one image of `img_shape`."""
        dst_height, dst_min_width, dst_max_width = self._dst(rank)
        ori_height, ori_width = img_shape[:2]
        c = img_shape[2] if len(img_shape) > 2 else 1
        valid_ratio = 1.0
        if self.keep_aspect_ratio:
            new_width = math.ceil(float(dst_height) / ori_height * ori_width)
            width_divisor = int(1 / self.width_downsample_ratio)
            if new_width % width_divisor != 0:
                new_width = round(new_width / width_divisor) * width_divisor
            if dst_min_width is not None:
                new_width = max(dst_min_width, new_width)
            if dst_max_width is not None:
                valid_ratio = min(1.0, 1.0 * new_width / dst_max_width)
                resize_width = min(dst_max_width, new_width)
                out_width = dst_max_width if new_width < dst_max_width else resize_width
            else:
                resize_width = out_width = new_width
        else:
            resize_width = out_width = dst_max_width
        return dict(height=dst_height, resize_w=int(resize_width), out_w=int(out_width), valid_ratio=valid_ratio,
                    resize_shape=(dst_height, int(resize_width), c), pad_shape=(dst_height, int(out_width), c))


@PIPELINES.register_module()
class NormalizeOCR:
    """`ocr_transforms.py:145-156`; `table()` tabulates ToTensorOCR + NormalizeOCR for the 256 byte values with
    torch's own fp32 arithmetic (x / 255, then (x - mean) / std), so the kernel's table lookup is exact."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def table(self, device):
        v = torch.arange(256, dtype=torch.float32).div(255)
        m = torch.as_tensor(self.mean, dtype=torch.float32).view(-1, 1)
        s = torch.as_tensor(self.std, dtype=torch.float32).view(-1, 1)
        return v.view(1, -1).repeat(m.shape[0], 1).sub_(m).div_(s).contiguous().to(device)


class OCRBatchPreprocessor:
    """ResizeOCR -> ToTensorOCR -> NormalizeOCR on a list of uint8 HWC images (numpy arrays or tensors, any sizes)
    -> (tensor (N, C, height, width) on `device`, img_metas).  All images of a batch share the padded width (the
    reference's `max_width` when it pads; otherwise they must agree)."""

    def __init__(self, resize, normalize, device="cuda"):
        self.resize, self.normalize, self.device = resize, normalize, torch.device(device)
        self._lut = None

    def _prepare(self, imgs, rank):
        """Checks, per-image plans, and the packed batch with its per-image arrays on the device."""
        if self.device.type != "cuda":
            raise _lib.TpsppError(f"{type(self).__name__}: the HIP path needs a GPU device (no CPU fallback)")
        arrs = []
        for im in imgs:
            a = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.ndim == 2:                   # a grayscale crop as mmcv.imread(color_type='grayscale') hands it over
                a = a[:, :, None]
            if a.dtype != np.uint8 or a.ndim != 3:
                raise TypeError("OCRBatchPreprocessor: images must be uint8 (H, W, C) or (H, W) arrays")
            arrs.append(np.ascontiguousarray(a))
        if not arrs:
            raise ValueError("OCRBatchPreprocessor: empty batch")
        interpolation = self.resize.interpolation()          # (raises for an unknown backend)
        C = arrs[0].shape[2]
        plans = [self.resize.plan(a.shape, rank) for a in arrs]
        H, W = plans[0]["height"], plans[0]["out_w"]
        if any(a.shape[2] != C for a in arrs) or any(p["out_w"] != W or p["height"] != H for p in plans):
            raise ValueError("OCRBatchPreprocessor: the images of a batch must agree on channels and padded size "
                             "(set max_width, as the reference's test pipeline does)")
        if self._lut is None or self._lut.device != self.device:
            self._lut = self.normalize.table(self.device)
        if self._lut.shape[0] != C:
            raise ValueError("OCRBatchPreprocessor: mean / std need one entry per channel")
        sizes = np.array([a.size for a in arrs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(self.device, non_blocking=True)
        meta = np.stack([np.array([a.shape[0] for a in arrs]), np.array([a.shape[1] for a in arrs]),
                         np.array([p["resize_w"] for p in plans])]).astype(np.int32)
        meta_d = torch.from_numpy(meta).to(self.device)
        offs_d = torch.from_numpy(offs).to(self.device)
        return arrs, plans, (C, H, W), interpolation, packed, offs_d, meta_d

    def _metas(self, arrs, plans):
        return [dict(ori_shape=a.shape, img_shape=p["resize_shape"], resize_shape=p["resize_shape"],
                     pad_shape=p["pad_shape"], valid_ratio=p["valid_ratio"],
                     img_norm_cfg=dict(mean=self.normalize.mean, std=self.normalize.std))
                for a, p in zip(arrs, plans)]

    def __call__(self, imgs, rank=0):
        arrs, plans, (C, H, W), interpolation, packed, offs_d, meta_d = self._prepare(imgs, rank)
        out = ops.resize_normalize(packed, offs_d, meta_d[0], meta_d[1], meta_d[2], self._lut,
                                   self.resize.img_pad_value, len(arrs), C, H, W, interpolation)
        return out, self._metas(arrs, plans)


# ---- the train pipeline's augmentations (crnn_pp_pipeline.py:11-74) ---------------------------------------------------------
# Every transform below keeps the reference's constructor and draws its parameters on the host; the pixel work of a whole
# batch is one launch of tpspp_augment_normalize_fwd.  Instead of `__call__(results)` a transform has
#     sample(rng, H, W)            -> [(code, params), ...] for one image, the op records of include/tpspp_augment.h
#     sample_batch(rng, N, H, W)   -> codes (N, K) int32, params (N, K, 8) float64 for N images at once (vectorised numpy;
#                                     a code 0 is an empty slot, not the end: the batch preprocessor closes the gaps)
# `rng` is an explicit numpy.random.Generator.  What is claimed is each parameter's DISTRIBUTION, restated from
# torchvision.transforms' get_params / the reference's own sampling -- not the reference's random stream: that one
# interleaves Python's `random`, numpy's global state and torch's generator across data-loader workers and cannot be
# reproduced from a seed here (nor is torchvision installed to compare draws with).
def _interp_name(v):
    v = getattr(v, "value", v)                 # torchvision's InterpolationMode carries the name as its value
    if isinstance(v, str):
        return v.lower()
    return {0: "nearest", 2: "bilinear", 3: "bicubic", 4: "box", 5: "hamming", 1: "lanczos"}.get(v, repr(v))


def _refuse_unpinned(op, kwargs, default):
    interp = kwargs.pop("interpolation", None)
    if interp is not None and _interp_name(interp) != default:
        raise NotImplementedError(f"TorchVisionWrapper(op='{op}'): interpolation={interp!r} is not implemented on the GPU "
                                  f"(only the transform's default, {default})")
    fill = kwargs.pop("fill", 0)
    if fill is not None and np.any(np.asarray(fill) != 0):
        raise NotImplementedError(f"TorchVisionWrapper(op='{op}'): fill={fill!r} is not implemented on the GPU (only 0)")


def _setup_angle(x, name, req_sizes=(2,)):
    """torchvision.transforms.transforms._setup_angle"""
    if isinstance(x, (int, float)):
        if x < 0:
            raise ValueError(f"If {name} is a single number, it must be positive.")
        return [-float(x), float(x)]
    if len(x) not in req_sizes:
        raise ValueError(f"{name} should be a sequence of length {' or '.join(str(s) for s in req_sizes)}.")
    return [float(d) for d in x]


def _get_inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix on arrays of N draws -> (N, 6) float64."""
    rot, sx, sy = np.radians(angle), np.radians(shear[0]), np.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = np.cos(rot - sy) / np.cos(sy)
    b = -np.cos(rot - sy) * np.tan(sx) / np.cos(sy) - np.sin(rot)
    c = np.sin(rot - sy) / np.cos(sy)
    d = -np.sin(rot - sy) * np.tan(sx) / np.cos(sy) + np.cos(rot)
    zero = np.zeros_like(a)
    m = np.stack([d, -b, zero, -c, a, zero], axis=-1) / np.asarray(scale, dtype=np.float64)[..., None]
    m[..., 2] += m[..., 0] * (-cx - tx) + m[..., 1] * (-cy - ty)
    m[..., 5] += m[..., 3] * (-cx - tx) + m[..., 4] * (-cy - ty)
    m[..., 2] += cx
    m[..., 5] += cy
    return m


def _records(codes, params):
    """One image's row of a batch plan -> [(code, params), ...] without the empty slots."""
    return [(int(c), tuple(float(v) for v in p)) for c, p in zip(codes, params) if c != ops.AUG_END]


class _BatchSampled:
    """`sample` from `sample_batch`.  Both draw from an explicit numpy.random.Generator: the DISTRIBUTIONS of the reference's
    parameters, not its random stream (three global generators interleaved across worker processes; see above)."""

    def sample(self, rng, H, W):
        codes, params = self.sample_batch(rng, 1, H, W)
        return _records(codes[0], params[0])


def _empty_plan(N, K):
    return np.zeros((N, K), dtype=np.int32), np.zeros((N, K, ops.AUG_OP_PARAMS), dtype=np.float64)


class _RandomAffine(_BatchSampled):
    """torchvision.transforms.RandomAffine on a PIL image: Image.transform(size, AFFINE, inverse matrix, NEAREST)."""

    def __init__(self, degrees, translate=None, scale=None, shear=None, center=None, **kwargs):
        _refuse_unpinned("RandomAffine", kwargs, "nearest")
        if kwargs:
            raise TypeError(f"RandomAffine: unexpected arguments {sorted(kwargs)}")
        if center is not None:
            raise NotImplementedError("TorchVisionWrapper(op='RandomAffine'): center is not implemented on the GPU")
        self.degrees = _setup_angle(degrees, "degrees")
        if translate is not None:
            if len(translate) != 2:
                raise TypeError("translate should be a sequence of length 2.")
            for t in translate:
                if not 0.0 <= t <= 1.0:
                    raise ValueError("translation values should be between 0 and 1")
        if scale is not None:
            if len(scale) != 2:
                raise TypeError("scale should be a sequence of length 2.")
            for s in scale:
                if s <= 0:
                    raise ValueError("scale values should be positive")
        self.translate, self.scale = translate, scale
        self.shear = None if shear is None else _setup_angle(shear, "shear", (2, 4))

    def get_params(self, rng, N, H, W):
        """RandomAffine.get_params for N images: angle, (tx, ty), scale, (shear_x, shear_y)."""
        angle = rng.uniform(self.degrees[0], self.degrees[1], N)
        if self.translate is not None:
            max_dx, max_dy = float(self.translate[0] * W), float(self.translate[1] * H)
            tx, ty = np.round(rng.uniform(-max_dx, max_dx, N)), np.round(rng.uniform(-max_dy, max_dy, N))
        else:
            tx = ty = np.zeros(N)
        scale = rng.uniform(self.scale[0], self.scale[1], N) if self.scale is not None else np.ones(N)
        shear_x = shear_y = np.zeros(N)
        if self.shear is not None:
            shear_x = rng.uniform(self.shear[0], self.shear[1], N)
            if len(self.shear) == 4:
                shear_y = rng.uniform(self.shear[2], self.shear[3], N)
        return angle, (tx, ty), scale, (shear_x, shear_y)

    def sample_batch(self, rng, N, H, W):
        angle, translate, scale, shear = self.get_params(rng, N, H, W)
        codes, params = _empty_plan(N, 1)
        codes[:, 0] = ops.AUG_AFFINE_NEAREST_PIL
        params[:, 0, :6] = _get_inverse_affine_matrix((W * 0.5, H * 0.5), angle, translate, scale, shear)
        return codes, params


class _RandomPerspective(_BatchSampled):
    """torchvision.transforms.RandomPerspective on a PIL image: Image.transform(size, PERSPECTIVE, coeffs, BILINEAR)."""

    def __init__(self, distortion_scale=0.5, p=0.5, **kwargs):
        _refuse_unpinned("RandomPerspective", kwargs, "bilinear")
        if kwargs:
            raise TypeError(f"RandomPerspective: unexpected arguments {sorted(kwargs)}")
        self.distortion_scale, self.p = distortion_scale, p

    def get_params(self, rng, N, H, W):
        """RandomPerspective.get_params -> startpoints (4, 2), endpoints (N, 4, 2): the four corners, jittered inwards."""
        ds = self.distortion_scale
        bw, bh = int(ds * (W // 2)), int(ds * (H // 2))
        lo_x, lo_y = rng.integers(0, bw + 1, (N, 2)), rng.integers(0, bh + 1, (N, 2))
        hi_x, hi_y = rng.integers(W - bw - 1, W, (N, 2)), rng.integers(H - bh - 1, H, (N, 2))
        end = np.stack([np.stack([lo_x[:, 0], lo_y[:, 0]], -1), np.stack([hi_x[:, 0], lo_y[:, 1]], -1),
                        np.stack([hi_x[:, 1], hi_y[:, 0]], -1), np.stack([lo_x[:, 1], hi_y[:, 1]], -1)], 1)
        start = np.array([[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], dtype=np.float64)
        return start, end.astype(np.float64)

    @staticmethod
    def coeffs(start, end):
        """_get_perspective_coeffs: the 8 coefficients that send the endpoints to the startpoints, the (square) least-squares
        system solved in float64, all images at once."""
        N = end.shape[0]
        A = np.zeros((N, 8, 8), dtype=np.float64)
        sx, sy = start[None, :, 0], start[None, :, 1]
        A[:, 0::2, 0], A[:, 0::2, 1], A[:, 0::2, 2] = end[:, :, 0], end[:, :, 1], 1.0
        A[:, 0::2, 6], A[:, 0::2, 7] = -sx * end[:, :, 0], -sx * end[:, :, 1]
        A[:, 1::2, 3], A[:, 1::2, 4], A[:, 1::2, 5] = end[:, :, 0], end[:, :, 1], 1.0
        A[:, 1::2, 6], A[:, 1::2, 7] = -sy * end[:, :, 0], -sy * end[:, :, 1]
        b = np.broadcast_to(start.reshape(1, 8, 1), (N, 8, 1))
        return np.linalg.solve(A, b)[:, :, 0]

    def sample_batch(self, rng, N, H, W):
        codes, params = _empty_plan(N, 1)
        start, end = self.get_params(rng, N, H, W)
        params[:, 0, :] = self.coeffs(start, end)
        codes[:, 0] = np.where(rng.random(N) < self.p, ops.AUG_PERSPECTIVE_BILINEAR_PIL, ops.AUG_END)
        return codes, params


class _ColorJitter(_BatchSampled):
    """torchvision.transforms.ColorJitter on a PIL image: ImageEnhance.Brightness / Contrast / Color and the hue shift
    through convert('HSV'), in a random order."""
    _CODES = (ops.AUG_BRIGHTNESS, ops.AUG_CONTRAST, ops.AUG_SATURATION, ops.AUG_HUE)     # fn_idx 0..3

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = self._check_input(brightness, "brightness")
        self.contrast = self._check_input(contrast, "contrast")
        self.saturation = self._check_input(saturation, "saturation")
        self.hue = self._check_input(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def _check_input(value, name, center=1, bound=(0, float("inf")), clip_first_on_zero=True):
        if isinstance(value, (int, float)):
            if value < 0:
                raise ValueError(f"If {name} is a single number, it must be non negative.")
            value = [center - float(value), center + float(value)]
            if clip_first_on_zero:
                value[0] = max(value[0], 0.0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            value = [float(value[0]), float(value[1])]
        else:
            raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError(f"{name} values should be between {bound}, but got {value}.")
        return None if value[0] == value[1] == center else tuple(value)

    def sample_batch(self, rng, N, H, W):
        codes, params = _empty_plan(N, 4)
        order = rng.permuted(np.tile(np.arange(4), (N, 1)), axis=1)          # fn_idx: a uniform permutation per image
        ranges = (self.brightness, self.contrast, self.saturation, self.hue)
        factor = np.zeros((N, 4), dtype=np.float64)
        for i, r in enumerate(ranges):
            if r is not None:
                factor[:, i] = rng.uniform(r[0], r[1], N)
        factor[:, 3] = (factor[:, 3] * 255.0).astype(np.int64) & 255         # uint8(hue_factor * 255), wrapping
        active = np.array([r is not None for r in ranges])
        codes[:] = np.where(active[order], np.asarray(self._CODES, dtype=np.int32)[order], ops.AUG_END)
        params[:, :, 0] = np.take_along_axis(factor, order, axis=1)
        return codes, params


_TV_OPS = {"RandomAffine": _RandomAffine, "RandomPerspective": _RandomPerspective, "ColorJitter": _ColorJitter}


@PIPELINES.register_module()
class TorchVisionWrapper(_BatchSampled):
    """`transform_wrappers.py:74-128` for the three torchvision transforms the train pipeline uses; any other `op`, an
    `interpolation` other than the transform's default and a non-zero `fill` raise NotImplementedError by name."""

    def __init__(self, op, **kwargs):
        assert type(op) is str
        if op not in _TV_OPS:
            raise NotImplementedError(f"TorchVisionWrapper: op='{op}' is not implemented on the GPU "
                                      f"(implemented: {', '.join(sorted(_TV_OPS))})")
        self.op, self.kwargs = op, dict(kwargs)
        self.transform = _TV_OPS[op](**kwargs)

    def sample_batch(self, rng, N, H, W):
        return self.transform.sample_batch(rng, N, H, W)


@PIPELINES.register_module()
class RandomRotateTextDet(_BatchSampled):
    """`transforms.py:179-223`: cv2.warpAffine(img, getRotationMatrix2D((w / 2, h / 2), angle, 1), (w, h), INTER_NEAREST).
    UNPINNED like backend='cv2': the matrix and its inversion restate OpenCV's published code, the kernel its 10-bit fixed
    point; none of it was compared with OpenCV itself."""

    def __init__(self, rotate_ratio=1.0, max_angle=10):
        self.rotate_ratio, self.max_angle = rotate_ratio, max_angle

    @staticmethod
    def sample_angle(rng, max_angle, N=None):
        return rng.random(N) * 2 * max_angle - max_angle

    @staticmethod
    def inverse_matrix(angle, H, W):
        """getRotationMatrix2D((W / 2, H / 2), angle, 1), then the inversion warpAffine performs -> (N, 6) float64."""
        rad = np.asarray(angle, dtype=np.float64) * (np.pi / 180.0)
        alpha, beta = np.cos(rad), np.sin(rad)
        cx, cy = W / 2, H / 2
        m0, m1, m2 = alpha, beta, (1 - alpha) * cx - beta * cy
        m3, m4, m5 = -beta, alpha, beta * cx + (1 - alpha) * cy
        D = m0 * m4 - m1 * m3
        D = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 0.0)
        a11, a22 = m4 * D, m0 * D
        m0, m1, m3, m4 = a11, m1 * -D, m3 * -D, a22
        b1, b2 = -m0 * m2 - m1 * m5, -m3 * m2 - m4 * m5
        return np.stack([m0, m1, b1, m3, m4, b2], axis=-1)

    def sample_batch(self, rng, N, H, W):
        codes, params = _empty_plan(N, 1)
        codes[:, 0] = np.where(rng.random(N) < self.rotate_ratio, ops.AUG_AFFINE_NEAREST_CV2, ops.AUG_END)
        params[:, 0, :6] = self.inverse_matrix(self.sample_angle(rng, self.max_angle, N), H, W)
        return codes, params


def _build_all(transforms):
    out = []
    for t in transforms:
        if isinstance(t, dict):
            t = PIPELINES.build(t)
        elif not hasattr(t, "sample_batch"):
            raise TypeError("transform must be a dict or have sample_batch(rng, N, H, W)")
        out.append(t)
    return out


@PIPELINES.register_module()
class OneOfWrapper(_BatchSampled):
    """`transform_wrappers.py:14-46`: one of the transforms, each with the same chance."""

    def __init__(self, transforms):
        assert isinstance(transforms, list) or isinstance(transforms, tuple)
        assert len(transforms) > 0, 'Need at least one transform.'
        self.transforms = _build_all(transforms)

    def sample_batch(self, rng, N, H, W):
        plans = [t.sample_batch(rng, N, H, W) for t in self.transforms]
        codes, params = _empty_plan(N, max(c.shape[1] for c, _ in plans))
        choice = rng.integers(0, len(plans), N)
        for i, (c, p) in enumerate(plans):
            rows = choice == i
            codes[rows, :c.shape[1]], params[rows, :c.shape[1]] = c[rows], p[rows]
        return codes, params


@PIPELINES.register_module()
class RandomWrapper(_BatchSampled):
    """`transform_wrappers.py:49-71`: the transforms, in order, with probability p (u < p on u in [0, 1): p = 0 never
    runs them, p = 1 always)."""

    def __init__(self, transforms, p):
        assert 0 <= p <= 1
        self.transforms, self.p = _build_all(transforms), p

    def sample_batch(self, rng, N, H, W):
        plans = [t.sample_batch(rng, N, H, W) for t in self.transforms]
        run = rng.random(N) < self.p
        if not plans:
            return _empty_plan(N, 0)
        codes = np.concatenate([c for c, _ in plans], axis=1)
        params = np.concatenate([p for _, p in plans], axis=1)
        codes[~run] = ops.AUG_END
        return codes, params


class _Unpinned:
    """A transform of the train pipeline whose arithmetic (OpenCV / albumentations) cannot be pinned here."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} is not implemented on the GPU (OpenCV / albumentations arithmetic "
                                  f"that cannot be pinned); pass skip=('{type(self).__name__}',) to "
                                  f"OCRTrainBatchPreprocessor to train without it")


@PIPELINES.register_module()
class PyramidRescale(_Unpinned):
    pass


@PIPELINES.register_module()
class Albu(_Unpinned):
    pass


def compact_plan(codes, params, max_ops=ops.AUG_MAX_OPS):
    """Close the gaps (code 0 slots) of a batch plan, keeping each image's order -> codes (N, max_ops), params (N, max_ops, 8)."""
    N, K = codes.shape
    order = np.argsort(codes == ops.AUG_END, axis=1, kind="stable")
    codes = np.take_along_axis(codes, order, axis=1)
    params = np.take_along_axis(params, order[:, :, None], axis=1)
    params[codes == ops.AUG_END] = 0.0
    if K > max_ops:
        if np.any(codes[:, max_ops:] != ops.AUG_END):
            raise ValueError(f"the pipeline asks for more than {max_ops} augmentation ops on one image")
        codes, params = codes[:, :max_ops], params[:, :max_ops]
    out_c, out_p = _empty_plan(N, max_ops)
    out_c[:, :codes.shape[1]], out_p[:, :codes.shape[1]] = codes, params
    return out_c, out_p


class OCRTrainBatchPreprocessor(OCRBatchPreprocessor):
    """The reference's `train_pipeline` (crnn_pp_pipeline.py:2-84), as written, on a list of uint8 HWC images ->
    (tensor (N, C, height, width) on `device`, img_metas); `img_metas[i]['augment_ops']` is the op list applied to image i.

    `LoadImageFromFile`, `ToTensorOCR` and `Collect` are taken as given (the images arrive as arrays, the tensor leaves
    normalised).  `PyramidRescale` and `Albu` raise NotImplementedError by name unless listed in `skip`, which drops them
    (wherever they are nested) with one warning.  `bgr`: channel 0 is blue, as mmcv.imread loads.  The draws come from
    `numpy.random.default_rng(seed)`: the same seed and batches give the same plans; see the note on distributions above."""
    _GIVEN = ("LoadImageFromFile", "ToTensorOCR", "Collect")

    def __init__(self, pipeline_cfg, device="cuda", seed=0, skip=(), bgr=True):
        skip = (skip,) if isinstance(skip, str) else tuple(skip)
        dropped = []
        cfg = self._strip(list(pipeline_cfg), skip, dropped)
        if dropped:
            import warnings
            warnings.warn(f"OCRTrainBatchPreprocessor: training WITHOUT {', '.join(sorted(set(dropped)))} (skip=)")
        resize = normalize = None
        self.augments = []
        for c in cfg:
            t = c["type"]
            if t in self._GIVEN:
                continue
            if t == "ResizeOCR":
                if resize is not None or self.augments or normalize is not None:
                    raise ValueError("OCRTrainBatchPreprocessor: one ResizeOCR, before the augmentations")
                resize = PIPELINES.build(c)
            elif t == "NormalizeOCR":
                if normalize is not None:
                    raise ValueError("OCRTrainBatchPreprocessor: one NormalizeOCR")
                normalize = PIPELINES.build(c)
            else:
                if resize is None or normalize is not None:
                    raise ValueError(f"OCRTrainBatchPreprocessor: {t} must stand between ResizeOCR and NormalizeOCR")
                obj = PIPELINES.build(c)
                if not hasattr(obj, "sample_batch"):
                    raise NotImplementedError(f"OCRTrainBatchPreprocessor: {t} is not implemented on the GPU")
                self.augments.append(obj)
        if resize is None or normalize is None:
            raise ValueError("OCRTrainBatchPreprocessor: the pipeline needs a ResizeOCR and a NormalizeOCR")
        super().__init__(resize, normalize, device)
        self.rng = np.random.default_rng(seed)
        self.bgr = bool(bgr)

    @classmethod
    def _strip(cls, cfgs, skip, dropped):
        out = []
        for c in cfgs:
            if isinstance(c, dict) and c.get("type") in skip:
                dropped.append(c["type"])
                continue
            if isinstance(c, dict) and isinstance(c.get("transforms"), (list, tuple)) and c.get("type") != "Albu":
                c = dict(c, transforms=cls._strip(list(c["transforms"]), skip, dropped))
            out.append(c)
        return out

    def plan(self, N, H, W, C=3):
        """The op lists of a batch of N images of H x W x C: codes (N, 8) int32, params (N, 8, 8) float64, gaps closed."""
        plans = [t.sample_batch(self.rng, N, H, W) for t in self.augments]
        codes = np.concatenate([c for c, _ in plans] + [_empty_plan(N, 1)[0]], axis=1)
        params = np.concatenate([p for _, p in plans] + [_empty_plan(N, 1)[1]], axis=1)
        if C == 1:
            # Pillow: ImageEnhance.Color and adjust_hue leave a one-channel image as it is
            codes[(codes == ops.AUG_SATURATION) | (codes == ops.AUG_HUE)] = ops.AUG_END
        return compact_plan(codes, params)

    def __call__(self, imgs, rank=0):
        arrs, plans, (C, H, W), interpolation, packed, offs_d, meta_d = self._prepare(imgs, rank)
        if C not in (1, 3):
            raise ValueError("OCRTrainBatchPreprocessor: images must have 1 or 3 channels")
        codes, params = self.plan(len(arrs), H, W, C)
        out = ops.augment_normalize(packed, offs_d, meta_d[0], meta_d[1], meta_d[2], self._lut,
                                    self.resize.img_pad_value, len(arrs), C, H, W,
                                    torch.from_numpy(codes).to(self.device), torch.from_numpy(params).to(self.device),
                                    interpolation, self.bgr)
        metas = self._metas(arrs, plans)
        for m, c, p in zip(metas, codes, params):
            m["augment_ops"] = _records(c, p)
        return out, metas
