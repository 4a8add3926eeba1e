"""The yardstick of the training augmentation (must3r_amd/train_augment.py, csrc/train_augment.hip).

Two things live here.  The yardstick itself runs the real Pillow calls per view -- ``Image.crop``, ``Image.resize`` (LANCZOS or BICUBIC), ``ImageEnhance.Brightness`` /
``Contrast`` / ``Color``, ``convert("HSV")`` and back, then ImgNorm -- with the geometry chain and the depth gather of the issue restated in float64 numpy (dust3r
and cv2 are no dependencies of this project: the stated formulas are the definition) and the axis swap of a landscape-stored portrait view.  Beside it stand the numpy emulations of
the four colour operations, the arithmetic the kernel implements; tests/test_augment_host.py shows that they equal Pillow.

The geometry is written here a second time, step by step and independently of ``train_augment.crop_resize_geometry``, so that the two can be compared."""
import types

import numpy as np
import torch
from PIL import Image, ImageEnhance

BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy emulations of the four operations (uint8 in, uint8 out)
# ---------------------------------------------------------------------------------------------------------------------------------
def blend_np(a, b, f):
    """Pillow's Image.blend(a, b, f) per byte: t = float(a) + f * float(b - a), one fp32 multiply then one fp32 add; 0 if t <= 0, 255 if t >= 255, else trunc"""
    a = np.asarray(a).astype(np.int32)
    b = np.asarray(b).astype(np.int32)
    f = np.float32(f)
    prod = (f * (b - a).astype(np.float32)).astype(np.float32)
    t = (a.astype(np.float32) + prod).astype(np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.uint8)


def luma_np(rgb):
    """Pillow's RGB -> L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    c = np.asarray(rgb).astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def contrast_mean(lsum, count):
    """int(sum(L) / count + 0.5), the division and the add in double"""
    return int(float(int(lsum)) / float(int(count)) + 0.5)


def rgb_to_hsv_np(rgb):
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = mx == mn
    cr = np.where(grey, 1, mx - mn).astype(np.float32)
    mxf = np.where(grey, 1, mx).astype(np.float32)
    s = (cr / mxf).astype(np.float32)
    rc, gc, bc = (((mx - ch).astype(np.float32) / cr).astype(np.float32) for ch in (r, g, b))
    h_r = (bc - gc).astype(np.float32)
    h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32)
    h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)
    h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(grey, 0, H), np.where(grey, 0, S), mx], axis=-1).astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb_np(hsv):
    c = np.asarray(hsv).astype(np.int32)
    H, S, V = c[..., 0], c[..., 1], c[..., 2]
    hh = H.astype(np.float64) * 6.0 / 255.0
    i = np.floor(hh)
    f = hh - i
    fs = S.astype(np.float64) / 255.0
    v = V.astype(np.float64)
    p = np.clip(_round_half_away(v * (1.0 - fs)), 0, 255).astype(np.int32)
    q = np.clip(_round_half_away(v * (1.0 - fs * f)), 0, 255).astype(np.int32)
    t = np.clip(_round_half_away(v * (1.0 - fs * (1.0 - f))), 0, 255).astype(np.int32)
    k = i.astype(np.int32) % 6
    table = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    out = np.empty(c.shape, dtype=np.int32)
    for ch in range(3):
        out[..., ch] = np.select([k == n for n in range(6)], [table[n][ch] for n in range(6)])
    out = np.where((S == 0)[..., None], V[..., None], out)
    return out.astype(np.uint8)


def hue_shift(hue_factor):
    """trunc(hue_factor * 255) mod 256, the factor as fp32 and the product in double"""
    return int(np.trunc(float(np.float32(hue_factor)) * 255.0)) % 256


def apply_op_np(img, op, factor, mean=None):
    """One operation on an HxWx3 uint8 image; ``mean`` overrides the contrast mean (for a view that is part of something larger: never, here)"""
    if op == BRIGHTNESS:
        return blend_np(np.zeros_like(img), img, factor)
    if op == SATURATION:
        return blend_np(np.repeat(luma_np(img)[..., None], 3, axis=-1), img, factor)
    if op == CONTRAST:
        L = luma_np(img)
        m = contrast_mean(L.astype(np.int64).sum(), L.size) if mean is None else mean
        return blend_np(np.full_like(img, m), img, factor)
    if op == HUE:
        hsv = rgb_to_hsv_np(img)
        hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + hue_shift(factor)) % 256).astype(np.uint8)
        return hsv_to_rgb_np(hsv)
    raise ValueError(op)


def contrast_boundary_images():
    """two grey 48 x 64 images whose mean L is k + 0.5 -+ 1 / 3072: sum / count + 0.5 falls just below and just above the integer k + 1"""
    out = []
    for delta in (-1, +1):
        img = np.full((48, 64, 3), 100, dtype=np.uint8)
        img.reshape(-1, 3)[:48 * 64 // 2 + delta] = 101          # grey: L == the value
        out.append(img)
    return out


def jitter_np(img, order, factors, flags=(1, 1, 1, 1)):
    for op in order:
        if flags[op]:
            img = apply_op_np(img, op, factors[op])
    return img


# ---------------------------------------------------------------------------------------------------------------------------------
# the same with the real Pillow calls (what torchvision's PIL backend does)
# ---------------------------------------------------------------------------------------------------------------------------------
def apply_op_pil(pil, op, factor):
    if op == BRIGHTNESS:
        return ImageEnhance.Brightness(pil).enhance(float(np.float32(factor)))
    if op == CONTRAST:
        return ImageEnhance.Contrast(pil).enhance(float(np.float32(factor)))
    if op == SATURATION:
        return ImageEnhance.Color(pil).enhance(float(np.float32(factor)))
    if op == HUE:
        h, s, v = pil.convert("HSV").split()
        nh = ((np.asarray(h).astype(np.int32) + hue_shift(factor)) % 256).astype(np.uint8)
        return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    raise ValueError(op)


def jitter_pil(img, order, factors, flags=(1, 1, 1, 1)):
    """HxWx3 uint8 numpy -> the same after the flagged operations in ``order``, each a Pillow call"""
    pil = Image.fromarray(np.ascontiguousarray(img), "RGB")
    for op in order:
        if flags[op]:
            pil = apply_op_pil(pil, op, factors[op])
    return np.asarray(pil).copy()


def img_norm_np(u8):
    """ImgNorm of an HxWx3 uint8 image: fp32 [3, H, W], (u / 255 - 0.5) / 0.5 with every operation in fp32"""
    x = np.asarray(u8).astype(np.float32)
    return np.ascontiguousarray((((x / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)).astype(np.float32).transpose(2, 0, 1))


NORM_TABLE = (((np.arange(256).astype(np.float32) / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)


def invert_norm(v):
    """the byte behind an ImgNorm value: u = int(127.5f * v + 127.5f + 0.5f), every operation rounded to fp32"""
    v = np.asarray(v, dtype=np.float32)
    t = (np.float32(127.5) * v).astype(np.float32)
    t = (t + np.float32(127.5)).astype(np.float32)
    t = (t + np.float32(0.5)).astype(np.float32)
    return t.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the geometry chain, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def camera_matrix_of_crop(K, in_size, out_size, scaling=1.0):
    K = np.array(K, dtype=np.float64)
    margins = np.asarray(in_size, dtype=np.float64) * scaling - np.asarray(out_size, dtype=np.float64)
    assert np.all(margins >= 0.0)
    offset = 0.5 * margins
    K[:2, 2] += 0.5
    K[:2, :] *= scaling
    K[:2, 2] -= offset
    K[:2, 2] -= 0.5
    return K


def geometry(W, H, K, resolution, rng=None, aug_crop=0):
    """-> namespace(crop1 (l, t, r, b), size1 (W, H), scale, resized (w, h), lanczos, window (l, t, r, b), out (w', h'), K float64 [3, 3])"""
    K = np.array(K, dtype=np.float64)
    cx, cy = (int(v) for v in np.round(K[:2, 2]))
    mx, my = min(cx, W - cx), min(cy, H - cy)
    if not (mx > W / 5 and my > H / 5):
        raise ValueError("principal point too close to the border")
    l1, t1 = cx - mx, cy - my
    crop1 = (l1, t1, cx + mx, cy + my)
    K[0, 2] -= l1
    K[1, 2] -= t1
    W, H = 2 * mx, 2 * my
    w, h = resolution
    if not w >= h:
        raise ValueError("resolution is (w, h) with w >= h")
    if H > 1.1 * W:
        w, h = h, w
    elif 0.9 < H / W < 1.1 and w != h and rng is not None:
        if rng.integers(2):
            w, h = h, w
    target = np.array([w, h], dtype=np.float64)
    if aug_crop > 1:
        target = target + rng.integers(0, aug_crop)
    size1 = np.array([W, H], dtype=np.float64)
    scale = float(np.max(target / size1)) + 1e-8
    resized = np.floor(size1 * scale).astype(int)
    K = camera_matrix_of_crop(K, (W, H), resized, scaling=scale)
    K2 = camera_matrix_of_crop(K, resized, (w, h), scaling=1)
    l, t = (int(v) for v in np.int32(np.round(K[:2, 2] - K2[:2, 2])))
    window = (l, t, l + w, t + h)
    K[0, 2] -= l
    K[1, 2] -= t
    if l < 0 or t < 0 or window[2] > resized[0] or window[3] > resized[1]:
        raise ValueError("the final crop does not lie inside the rescaled image")
    return types.SimpleNamespace(crop1=crop1, size1=(W, H), scale=scale, resized=(int(resized[0]), int(resized[1])), lanczos=scale < 1, window=window,
                                 out=(w, h), K=K)


def depth_gather(depth, g):
    """the window's depth [h', w']: pixel (x, y) reads depth[t1 + sy, l1 + sx], the source coordinates in double"""
    (l1, t1, _, _), (W, H), (rw, rh), (l, t, _, _), (w, h) = g.crop1, g.size1, g.resized, g.window, g.out
    sx = np.minimum(np.floor((np.arange(w, dtype=np.float64) + l) * (float(W) / float(rw))), W - 1).astype(np.int64)
    sy = np.minimum(np.floor((np.arange(h, dtype=np.float64) + t) * (float(H) / float(rh))), H - 1).astype(np.int64)
    return np.ascontiguousarray(np.asarray(depth)[t1 + sy][:, l1 + sx])


def resample_pil(frame, g):
    """crop, resize and the final window of one HxWx3 uint8 frame, as Pillow does them"""
    pil = Image.fromarray(np.ascontiguousarray(frame), "RGB").crop(g.crop1)
    pil = pil.resize(g.resized, resample=Image.LANCZOS if g.lanczos else Image.BICUBIC)
    return np.asarray(pil.crop(g.window)).copy()


def view_ref(frame, depth, K, resolution, rng=None, aug_crop=0, jitter=None, landscape=True):
    """One view through the whole chain.  ``jitter``: None, or (order, factors, flags).  -> dict of torch tensors on the CPU: ``img`` fp32 [3, Hs, Ws],
    ``depthmap`` [Hs, Ws] in depth's dtype, ``camera_intrinsics`` fp32 [3, 3], ``true_shape`` int32 [2] (h', w'); with ``landscape`` a portrait view is stored
    with its axes swapped.  Also ``u8``: the jittered uint8 image of the true orientation, and ``geometry``."""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    g = geometry(W, H, K, resolution, rng, aug_crop)
    u8 = resample_pil(frame, g)
    if jitter is not None:
        u8 = jitter_pil(u8, *jitter)
    img = img_norm_np(u8)
    d = depth_gather(np.asarray(depth), g)
    w, h = g.out
    if landscape and h > w:
        img, d = np.ascontiguousarray(img.swapaxes(1, 2)), np.ascontiguousarray(d.T)
    dt = torch.from_numpy(d.astype(np.int32)).to(torch.uint16) if d.dtype == np.uint16 else torch.from_numpy(d)
    return dict(img=torch.from_numpy(img), depthmap=dt, camera_intrinsics=torch.from_numpy(g.K.astype(np.float32)),
                true_shape=torch.tensor([h, w], dtype=torch.int32), u8=u8, geometry=g)
