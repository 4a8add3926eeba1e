"""Host side of the native image loaders (must3r_amd.image; include/must3r_hip.h ABI 9), no GPU needed:

* the bucket choice and both 3x3 matrices equal the reference's must3r/tools/image.py, run verbatim;
* must3r_hip_resample_coeffs + a numpy emulation of the integer two-pass pipeline equals PIL.Image.resize bit for bit;
* the fp32 coefficients + a sequential fp32 emulation equal F.interpolate (antialiased bilinear, nearest-exact) on the CPU;
* preproc_frame's geometry equals a restatement of must3r/slam/model.py:99-120 with Pillow's own resize.
"""
import importlib
import sys

import numpy as np
import PIL.Image
import pytest
import torch
import torch.nn.functional as F

from conftest import HAS_REFERENCE
from must3r_amd import _lib
from must3r_amd import image as I

LANCZOS, BICUBIC = _lib.RESAMPLE_PIL_LANCZOS, _lib.RESAMPLE_PIL_BICUBIC


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. buckets and matrices against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _sizes():
    rng = np.random.default_rng(7)
    fixed = [(384, 512), (512, 384), (224, 224), (288, 512), (512, 288), (336, 512), (160, 512), (256, 512), (512, 160),
             (1080, 1920), (1920, 1080), (3024, 4032), (4032, 3024), (1000, 1000), (240, 320), (481, 640), (641, 480),
             (490, 700), (700, 490),     # halfway between 4/3 and 32/21
             (900, 1700), (1700, 900),   # halfway between 16/9 and 2
             (500, 1300), (1300, 500),   # halfway between 2 and 16/5
             (64, 64), (64, 6000), (6000, 64), (6000, 5999), (333, 997)]
    rand = [tuple(int(v) for v in rng.integers(64, 6001, 2)) for _ in range(60)]
    return fixed + rand


@pytest.fixture
def ref_image(monkeypatch):
    if not HAS_REFERENCE:
        pytest.skip("runs the reference's tools/image.py live; its tree is not present")
    from oracle import ref_shims
    ref_shims.install()
    tvf = sys.modules["torchvision.transforms"]
    calls = []

    class CenterCrop:
        def __init__(self, size):
            calls.append(("crop", list(size)))

    class Resize:
        def __init__(self, size, interpolation="bilinear"):
            calls.append(("resize", list(size), interpolation))

    class Compose:
        def __init__(self, ops):
            self.ops = ops

    class InterpolationMode:
        NEAREST_EXACT = "nearest-exact"

    for name, obj in (("CenterCrop", CenterCrop), ("Resize", Resize), ("Compose", Compose), ("InterpolationMode", InterpolationMode)):
        monkeypatch.setattr(tvf, name, obj, raising=False)
    mod = importlib.import_module("must3r.tools.image")
    return mod, calls


@pytest.mark.parametrize("maxdim", [224, 512])
def test_buckets_and_matrices_equal_the_reference(ref_image, maxdim):
    ref, calls = ref_image
    assert {m: {k: list(v) for k, v in d.items()} for m, d in I.ratios_resolutions.items()} == ref.ratios_resolutions
    n_identity = 0
    for H, W in _sizes():
        assert I.get_HW_resolution(H, W, maxdim) == ref.get_HW_resolution(H, W, maxdim), (H, W)
        for is_mask in (False, True):
            calls.clear()
            r_op, r_resc, r_orig = ref.get_resize_function(maxdim, 16, H, W, is_mask=is_mask)
            op, resc, orig = I.get_resize_function(maxdim, 16, H, W, is_mask=is_mask)
            assert np.array_equal(resc, r_resc) and np.array_equal(orig, r_orig), (H, W)
            if not calls:   # the reference's identity case
                n_identity += 1
                x = object()
                assert op(x) is x
                continue
            (_, crop), (_, target, interp) = calls
            assert [op.crop_H, op.crop_W] == crop and list(op.target) == list(target), (H, W)
            assert op.mode == (_lib.RESAMPLE_NEAREST_EXACT if is_mask else _lib.RESAMPLE_AA_BILINEAR)
            assert (interp == "nearest-exact") == is_mask
    assert n_identity >= 2


def test_bucket_refusals():
    with pytest.raises(ValueError, match="patch size"):
        I.get_HW_resolution(1080, 1920, 512, patchsize=14)
    with pytest.raises(ValueError, match="patch size"):
        I.get_resize_function(512, 24, 1080, 1920)
    with pytest.raises(ValueError, match="not implemented"):
        I.get_resize_function(500, 16, 1080, 1920)
    with pytest.raises(ValueError, match="empty"):
        I.get_resize_function(512, 16, 0, 1920)


@pytest.mark.parametrize("H, W, crop_H, crop_W", [(101, 200, 100, 200), (103, 200, 100, 200), (100, 201, 100, 198), (100, 205, 100, 200)])
def test_center_offsets_round_half_to_even(H, W, crop_H, crop_W):
    # torchvision center_crop: int(round((H - crop_H) / 2.0)) -- 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    top, left = I._center_offsets(H, W, crop_H, crop_W)
    assert (top, left) == (int(round((H - crop_H) / 2.0)), int(round((W - crop_W) / 2.0)))
    assert {(101, 200): (0, 0), (103, 200): (2, 0), (100, 201): (0, 2), (100, 205): (0, 2)}[(H, W)] == (top, left)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. Pillow bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _pil_pass(a, axis, mode, out):
    """Pillow's 8-bit pass along `axis` with the library's coefficients: int32 sums from 1 << 21, >> 22, clip8."""
    bounds, w = I.resample_coeffs(mode, a.shape[axis], out)
    k = np.arange(w.shape[1])
    idx = np.minimum(bounds[:, :1] + k[None], a.shape[axis] - 1)            # [out, ksize]; taps past the count have weight 0
    wk = np.where(k[None] < bounds[:, 1:], w, 0).astype(np.int64)
    src = np.moveaxis(a, axis, 0).astype(np.int64)                          # [in, ...]
    acc = (1 << 21) + np.einsum("ok,ok...->o...", wk, src[idx])
    assert np.all(np.abs(acc) < 2 ** 31)                                    # int32 like Pillow's
    return np.moveaxis(np.clip(acc >> 22, 0, 255).astype(np.uint8), 0, axis)


def _pil_emulation(img, w, h, mode):
    return _pil_pass(_pil_pass(img, 1, mode, w), 0, mode, h)


def _grid():
    cases = []
    for f in (1.01, 1.5, 2.0, 3.75, 7.875):
        cases.append(((round(63 * f), round(101 * f)), (63, 101)))
    cases += [((40, 30), (97, 61)), ((17, 23), (18, 24)),             # enlargements
              ((1, 57), (1, 13)), ((57, 1), (11, 1)), ((64, 64), (1, 1)), ((1, 1), (5, 3)),
              ((97, 89), (13, 89)), ((89, 97), (89, 13)),             # one axis unchanged
              ((101, 131), (7, 53)), ((211, 127), (59, 31)),          # primes
              ((120, 160), (120, 160))]                               # no change at all
    return cases


@pytest.mark.parametrize("mode, pil_filter", [(LANCZOS, PIL.Image.LANCZOS), (BICUBIC, PIL.Image.BICUBIC)], ids=["lanczos", "bicubic"])
@pytest.mark.parametrize("src, dst", _grid())
def test_pil_coefficients_bit_exact(mode, pil_filter, src, dst):
    rng = np.random.default_rng(src[0] * 1000 + dst[1])
    img = rng.integers(0, 256, (*src, 3), dtype=np.uint8)
    ref = np.asarray(PIL.Image.fromarray(img).resize((dst[1], dst[0]), pil_filter))
    assert np.array_equal(_pil_emulation(img, dst[1], dst[0], mode), ref)


def test_pil_coefficients_layout():
    b, w = I.resample_coeffs(LANCZOS, 1920, 512)
    assert w.dtype == np.int32 and b.shape == (512, 2) and w.shape[1] == 2 * int(np.ceil(3 * 1920 / 512)) + 1
    assert np.all(np.abs(w.sum(1) - (1 << 22)) <= w.shape[1])           # normalised, rounded per tap
    b, w = I.resample_coeffs(BICUBIC, 77, 77)                            # unchanged axis: an exact one-tap copy
    assert w.shape == (77, 1) and np.array_equal(b[:, 0], np.arange(77)) and np.all(b[:, 1] == 1) and np.all(w == 1 << 22)
    with pytest.raises(_lib.HipError, match="mode"):
        I.resample_coeffs(9, 10, 5)
    with pytest.raises(_lib.HipError, match="positive"):
        I.resample_coeffs(LANCZOS, 0, 5)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 modes against torch's CPU kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32_pass(x, axis, mode, out):
    bounds, w = I.resample_coeffs(mode, x.shape[axis], out)
    src = np.moveaxis(x, axis, 0)
    res = np.zeros((out,) + src.shape[1:], np.float32)
    for k in range(w.shape[1]):                                           # ascending taps, fp32 sums, like ATen's loop
        live = k < bounds[:, 1]
        idx = np.minimum(bounds[:, 0] + k, x.shape[axis] - 1)
        term = (src[idx] * w[:, k].reshape(-1, *[1] * (src.ndim - 1))).astype(np.float32)
        res = np.where(live.reshape(-1, *[1] * (src.ndim - 1)), (res + term).astype(np.float32), res)
    return np.moveaxis(res, 0, axis)


@pytest.mark.parametrize("src, dst", [((378, 504), (96, 128)), ((135, 240), (72, 128)), ((125, 125), (96, 128)), ((60, 80), (96, 128)),
                                      ((121, 77), (224, 224)), ((50, 60), (50, 17)), ((7, 3), (3, 2))])
def test_f32_coefficients_match_torch(src, dst):
    x = torch.rand(3, *src, generator=torch.Generator().manual_seed(src[0])) * 2 - 1
    ref = F.interpolate(x[None], dst, mode="bilinear", align_corners=False, antialias=True)[0].numpy()
    got = _f32_pass(_f32_pass(x.numpy(), 2, _lib.RESAMPLE_AA_BILINEAR, dst[1]), 1, _lib.RESAMPLE_AA_BILINEAR, dst[0])
    assert np.abs(got - ref).max() <= 2e-7
    ref = F.interpolate(x[None], dst, mode="nearest-exact")[0].numpy()
    got = _f32_pass(_f32_pass(x.numpy(), 2, _lib.RESAMPLE_NEAREST_EXACT, dst[1]), 1, _lib.RESAMPLE_NEAREST_EXACT, dst[0])
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. preproc_frame geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def _reference_preproc_geometry(H1, W1, res):
    """must3r/slam/model.py:99-120 with dust3r's _resize_pil_image, on a PIL image of the frame's size."""
    img = PIL.Image.new("RGB", (W1, H1))
    cx, cy = W1 // 2, H1 // 2
    longsize = res
    if res in [224, 336, 448]:
        longsize = max(W1, H1) / min(W1, H1) * res
    S = max(img.size)
    interp = PIL.Image.LANCZOS if S > longsize else PIL.Image.BICUBIC
    new_size = tuple(int(round(x * longsize / S)) for x in img.size)
    img = img.resize(new_size, interp)
    W, H = img.size
    cx, cy = W // 2, H // 2
    to_orig_focal = W1 / W
    if res in [224, 336, 448]:
        halfw = halfh = res // 2
    else:
        halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
    img = img.crop((cx - halfw, cy - halfh, cx + halfw, cy + halfh))
    return interp, (H, W), np.int32([img.size[::-1]]), np.int32([[cx - halfw, cy - halfh]]), to_orig_focal


@pytest.mark.parametrize("res", [512, 224])
@pytest.mark.parametrize("H1, W1", [(1080, 1920), (1920, 1080), (480, 640), (640, 480), (3024, 4032), (384, 512), (200, 100), (721, 1283)])
def test_preproc_frame_geometry(H1, W1, res):
    interp, size, true_shape, offset, focal = _reference_preproc_geometry(H1, W1, res)
    mode, got_size, (y0, x0, h, w), got_focal = I._frame_geometry(H1, W1, res)
    assert mode == (LANCZOS if interp == PIL.Image.LANCZOS else BICUBIC)
    assert got_size == size
    assert np.array_equal(np.int32([[h, w]]), true_shape) and np.array_equal(np.int32([[x0, y0]]), offset)
    assert got_focal == focal
    assert h % 16 == 0 and w % 16 == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# preproc_frame keeps the reference's signature, transform included (slam/model.py:99; its caller, slam/model.py:482, passes it)
# ---------------------------------------------------------------------------------------------------------------------------------
class ToTensor:
    pass


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms


DUST3R_IMGNORM = Compose([ToTensor(), Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])   # dust3r/datasets/utils/transforms.py's ImgNorm


def test_preproc_frame_binds_the_reference_call():
    import inspect
    sig = inspect.signature(I.preproc_frame)
    assert list(sig.parameters) == ["img", "idx", "res", "transform"] and sig.parameters["res"].default == 512
    sig.bind(np.zeros((4, 4, 3), np.uint8), 0, res=512, transform=DUST3R_IMGNORM)   # slam/model.py:482


def test_preproc_frame_transform_must_be_imgnorm():
    for t in (None, I.ImgNorm, DUST3R_IMGNORM, Compose([ToTensor(), Normalize([0.5], [0.5])])):
        assert I._is_imgnorm(t)
    others = (lambda x: x, Compose([ToTensor(), Normalize((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]), Compose([ToTensor()]),
              Compose([Normalize((0.5,) * 3, (0.5,) * 3), ToTensor()]))
    for t in others:
        assert not I._is_imgnorm(t)
        with pytest.raises(ValueError, match="ImgNorm"):   # refused before anything is uploaded
            I.preproc_frame(np.zeros((64, 64, 3), np.uint8), 0, res=512, transform=t)
