"""Image ingestion on the GPU -- drop-in for the reference's image loaders.

Same names and contracts as the reference, CUDA tensors out, no CPU fallback:

* ``get_HW_resolution`` / ``get_resize_function``   must3r/tools/image.py:26-97 (aspect-ratio buckets, centre crop, resize matrices);
  ``op`` runs the native resampler (``must3r_hip_resample``, MUST3R_RESAMPLE_AA_BILINEAR or _NEAREST_EXACT) on a CUDA fp32 tensor.
* ``load_images``                                   must3r/demo/inference.py:63-76: PIL decodes on the host, the uint8 pixels are
  uploaded from pinned memory and the whole folder is normalised, centre-cropped and resized by ONE native call.
* ``preproc_frame`` / ``preprocess_frames``         must3r/slam/model.py:99-120: dust3r's ``_resize_pil_image`` (Pillow LANCZOS /
  BICUBIC) + crop + ImgNorm, bit-exact with Pillow, for one frame or a [B, H, W, 3] uint8 batch in one call.

ImgNorm (dust3r: ToTensor then Normalize(0.5, 0.5)) maps a byte u to the fp32 value (u / 255 - 0.5) / 0.5; the library applies it
through a 256-entry table built on the host (include/must3r_hip.h).  Palette -> RGB conversion stays on the host in PIL, and so do
JPEG and PNG decoding by default; ``load_images(..., decode="gpu")`` decodes baseline JPEGs on the device (must3r_amd/jpeg.py), and
with ``png="gpu"`` the 8-bit grey, RGB and RGBA PNGs as well (must3r_amd/png.py).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

# The aspect-ratio buckets of must3r/tools/image.py:17-24, restated as the landscape sizes (long side, short side) per maxdim.  The
# reference keys each bucket by its ratio long / short (4/3, 32/21, 16/9, ...); every key there is that exact quotient, so the key is
# computed from the size here.
_BUCKETS = {
    224: ((224, 224),),
    336: ((336, 336),),
    384: ((384, 288), (384, 256), (384, 192), (384, 128)),
    448: ((448, 448),),
    512: ((512, 384), (512, 336), (512, 288), (512, 256), (512, 160)),
    768: ((768, 576), (768, 512), (768, 432), (768, 384), (768, 240)),
}
ratios_resolutions = {m: {long / short: [long, short] for long, short in sizes} for m, sizes in _BUCKETS.items()}

# load_images: uint8 source bytes per native call (the pinned host copies, device copies and fp32 intermediate of one chunk are alive together)
LOAD_CHUNK_BYTES = 256 << 20

# dust3r's preproc_frame crops a square for the resolutions of these training runs (must3r/slam/model.py:104-116)
_SQUARE_RES = (224, 336, 448)


def _buckets(maxdim):
    if isinstance(maxdim, dict):
        return maxdim
    if maxdim not in ratios_resolutions:
        raise ValueError(f"must3r_amd.image: maxdim={maxdim} not implemented (one of {sorted(ratios_resolutions)} or a dict)")
    return ratios_resolutions[maxdim]


def _patch(patchsize):
    if isinstance(patchsize, tuple):
        if len(patchsize) != 2 or not all(isinstance(p, int) for p in patchsize) or patchsize[0] != patchsize[1]:
            raise ValueError(f"must3r_amd.image: patch size {patchsize}: expected an int or a tuple of two equal ints")
        patchsize = patchsize[0]
    return int(patchsize)


def get_HW_resolution(H, W, maxdim, patchsize=16):
    """must3r/tools/image.py:26-52: the bucket [H, W] whose ratio is nearest to W / H (landscape) or H / W (portrait); ties go to the
    bucket listed first.  Raises ValueError when the bucket is not a multiple of ``patchsize``."""
    buckets = _buckets(maxdim)
    ratio = W / H
    refs = np.array([*buckets.keys()])
    landscape = W >= H
    diff = np.abs(ratio - refs) if landscape else np.abs(ratio - (1 / refs))
    res = buckets[refs[np.argmin(diff)]]
    p = _patch(patchsize)
    if p <= 0 or res[0] % p or res[1] % p:
        raise ValueError(f"must3r_amd.image: bucket {res} is not a multiple of patch size {p}")
    return res[::-1] if landscape else res


def _geometry(maxdim, patch_size, H, W):
    """(target [h, w] or None for the identity, crop_H, crop_W, to_rescaled, to_orig) of must3r/tools/image.py:55-97."""
    if H <= 0 or W <= 0:
        raise ValueError(f"must3r_amd.image: empty image ({H} x {W})")
    buckets = _buckets(maxdim)
    if [max(H, W), min(H, W)] in buckets.values():
        _patch(patch_size)
        return None, H, W, np.eye(3), np.eye(3)
    target = get_HW_resolution(H, W, maxdim=maxdim, patchsize=patch_size)
    ratio, target_ratio = W / H, target[1] / target[0]
    to_orig_crop, to_rescaled_crop = np.eye(3), np.eye(3)
    if abs(ratio - target_ratio) < np.finfo(np.float32).eps:
        crop_W, crop_H = W, H
    elif ratio - target_ratio < 0:
        crop_W, crop_H = W, int(W / target_ratio)
        to_orig_crop[1, 2] = (H - crop_H) / 2.0
        to_rescaled_crop[1, 2] = -(H - crop_H) / 2.0
    else:
        crop_W, crop_H = int(H * target_ratio), H
        to_orig_crop[0, 2] = (W - crop_W) / 2.0
        to_rescaled_crop[0, 2] = -(W - crop_W) / 2.0
    to_orig_resize = np.array([[crop_W / target[1], 0, 0], [0, crop_H / target[0], 0], [0, 0, 1]])
    to_rescaled_resize = np.array([[target[1] / crop_W, 0, 0], [0, target[0] / crop_H, 0], [0, 0, 1]])
    return list(target), crop_H, crop_W, to_rescaled_resize @ to_rescaled_crop, to_orig_crop @ to_orig_resize


def _center_offsets(H, W, crop_H, crop_W):
    """torchvision center_crop: top = int(round((H - crop_H) / 2.0)), left alike (Python round: halves to even)."""
    return int(round((H - crop_H) / 2.0)), int(round((W - crop_W) / 2.0))


def _check_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"must3r_amd.image: {what} must be a CUDA tensor; the HIP path has no CPU fallback")


def _desc(src, fmt, channels, H, W, row_stride, plane_stride, crop, resize, window, out_offset):
    return _lib.ImageDesc(src.data_ptr(), fmt, channels, H, W, row_stride, plane_stride, crop[0], crop[1], crop[2], crop[3],
                          resize[0], resize[1], window[0], window[1], window[2], window[3], out_offset)


def _resample(mode, descs, out, keep):
    """One must3r_hip_resample call on the current stream of ``out``'s device; ``keep``: source tensors (alive until the launch)."""
    lib = _lib.load()
    arr = (_lib.ImageDesc * len(descs))(*descs)
    nbytes = lib.must3r_hip_image_scratch_bytes(mode, arr, len(descs))
    if nbytes == 0:   # the call below reports why
        nbytes = 256
    with torch.cuda.device(out.device):
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=out.device)
        _lib.check(lib.must3r_hip_resample(mode, arr, len(descs), out.data_ptr(), scratch.data_ptr(), nbytes,
                                           _lib.stream_ptr(out.device)))
    del keep
    return out


class _ResizeOp:
    """CenterCrop([crop_H, crop_W]) + Resize(target) of torchvision >= 0.17 on a CUDA fp32 [C, H, W] / [B, C, H, W] tensor
    (antialiased bilinear, or nearest-exact for masks), as one native call."""

    def __init__(self, crop_H, crop_W, target, is_mask):
        self.crop_H, self.crop_W, self.target = crop_H, crop_W, tuple(target)
        self.mode = _lib.RESAMPLE_NEAREST_EXACT if is_mask else _lib.RESAMPLE_AA_BILINEAR

    def __call__(self, x):
        _check_cuda(x, "the image")
        if x.dtype != torch.float32:
            raise ValueError(f"must3r_amd.image: the resize op takes fp32 tensors, got {x.dtype}")
        if x.dim() not in (3, 4) or x.shape[-3] < 1 or x.shape[-3] > 4:
            raise ValueError(f"must3r_amd.image: expected [C, H, W] or [B, C, H, W] with 1 <= C <= 4, got {tuple(x.shape)}")
        H, W = int(x.shape[-2]), int(x.shape[-1])
        if H <= 0 or W <= 0 or x.numel() == 0:
            raise ValueError(f"must3r_amd.image: empty image {tuple(x.shape)}")
        if self.crop_H > H or self.crop_W > W:
            raise ValueError(f"must3r_amd.image: crop {self.crop_H} x {self.crop_W} larger than the {H} x {W} image")
        xb = x.reshape(-1, *x.shape[-3:]).contiguous()
        B, Cn = xb.shape[0], xb.shape[1]
        h, w = self.target
        top, left = _center_offsets(H, W, self.crop_H, self.crop_W)
        out = torch.empty((B, Cn, h, w), dtype=torch.float32, device=x.device)
        descs = [_desc(xb[b], _lib.IMG_F32_CHW, Cn, H, W, W, H * W, (top, left, self.crop_H, self.crop_W), (h, w), (0, 0, h, w),
                       b * Cn * h * w) for b in range(B)]
        _resample(self.mode, descs, out, xb)
        return out.reshape(*x.shape[:-2], h, w)


def get_resize_function(maxdim, patch_size, H, W, is_mask=False):
    """must3r/tools/image.py:55-97 -> (op, to_rescaled, to_orig); ``op`` is the identity when (H, W) already is a bucket size."""
    target, crop_H, crop_W, to_rescaled, to_orig = _geometry(maxdim, patch_size, H, W)
    if target is None:
        return (lambda x: x), to_rescaled, to_orig
    return _ResizeOp(crop_H, crop_W, target, is_mask), to_rescaled, to_orig


def _upload_u8(arr, device):
    """HxWx3 uint8 numpy -> CUDA uint8 tensor through pinned host memory (asynchronous copy on the current stream)."""
    host = torch.empty(arr.shape, dtype=torch.uint8, pin_memory=True)
    host.numpy()[...] = arr   # PIL's arrays are read-only: one copy, straight into pinned memory
    return host.to(device, non_blocking=True)


def load_images(folder_content, size, patch_size=16, verbose=True, device="cuda", decode="pil", png="pil"):
    """must3r/demo/inference.py:63-76 -> [dict(img=fp32 [3, h, w] CUDA, true_shape=np.int32([h, w]))].  Files are decoded in order and
    resampled in chunks of about LOAD_CHUNK_BYTES of uint8 pixels, one native call per chunk (12 MP photos: 8 per call), so host
    and device memory stay bounded however long the folder is.  ``decode="pil"`` (the default) decodes every file with Pillow on the host;
    ``decode="gpu"`` decodes the baseline JPEGs among them on the device (must3r_amd.jpeg, bit-equal to Pillow) and hands the pixels to the
    resampler without a host copy; what that decoder refuses still goes through Pillow.  ``png="gpu"`` (with ``decode="gpu"`` only) sends the PNG files
    that must3r_amd.png takes (8-bit grey, RGB and RGBA, not interlaced) to the device as well, in the same chunk as the JPEGs; ``png="pil"`` (the default)
    leaves every PNG with Pillow."""
    import PIL.Image
    if decode not in ("pil", "gpu"):
        raise ValueError(f"must3r_amd.image.load_images: decode={decode!r} (\"pil\" or \"gpu\")")
    if png not in ("pil", "gpu"):
        raise ValueError(f"must3r_amd.image.load_images: png={png!r} (\"pil\" or \"gpu\")")
    if png == "gpu" and decode != "gpu":
        raise ValueError("must3r_amd.image.load_images: png=\"gpu\" needs decode=\"gpu\"")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("must3r_amd.image.load_images: device must be CUDA; the HIP path has no CPU fallback")
    if decode == "gpu":
        return _load_images_gpu(folder_content, size, patch_size, verbose, device, png == "gpu")
    imgs, chunk, nbytes = [], [], 0
    for path in folder_content:
        rgb = PIL.Image.open(path).convert("RGB")
        rgb.load()
        W, H = rgb.size
        target, crop_H, crop_W, _, _ = _geometry(size, patch_size, H, W)
        chunk.append((path, np.asarray(rgb), H, W, target, crop_H, crop_W))
        nbytes += H * W * 3
        if nbytes >= LOAD_CHUNK_BYTES:   # bounded host / device memory: one native call per chunk of files
            imgs += _load_chunk(chunk, device, verbose)
            chunk, nbytes = [], 0
    if chunk:
        imgs += _load_chunk(chunk, device, verbose)
    return imgs


def _load_images_gpu(folder_content, size, patch_size, verbose, device, png_gpu=False):
    """load_images with the JPEG decode on the device (and the PNG decode, with ``png_gpu``): per chunk one decode call per format and one resample call, the
    pixels never on the host"""
    from . import jpeg, png
    device = jpeg._cuda_device(device, "image.load_images")
    imgs, preps, paths, nbytes = [], [], [], 0

    def prepare(path):
        """-> (decoder module, its prepared item); a PNG that must3r_amd.png refuses arrives decoded by Pillow and travels with the JPEG decoder's refusals"""
        if png_gpu:
            with open(path, "rb") as f:
                is_png = f.read(8) == b"\x89PNG\r\n\x1a\n"
            if is_png:
                p = png._prepare(path, "rgb", len(paths))
                return (png, p) if p[0] == "gpu" else (jpeg, p[:4])
        return jpeg, jpeg._prepare(path)

    def flush():
        nonlocal preps, paths, nbytes
        tensors = [None] * len(preps)
        for mod in (jpeg, png):
            idx = [k for k, (m, _) in enumerate(preps) if m is mod]
            if idx:
                for k, t in zip(idx, mod._decode_prepared([preps[k][1] for k in idx], device)):
                    tensors[k] = t
        chunk = []
        for path, (_, p), t in zip(paths, preps, tensors):
            H, W = p[2], p[3]
            target, crop_H, crop_W, _, _ = _geometry(size, patch_size, H, W)
            chunk.append((path, t, H, W, target, crop_H, crop_W))
        preps, paths, nbytes = [], [], 0
        return _load_chunk(chunk, device, verbose)

    for path in folder_content:
        preps.append(prepare(path))
        paths.append(path)
        H, W = preps[-1][1][2], preps[-1][1][3]
        _geometry(size, patch_size, H, W)   # a size the buckets refuse is reported before anything is launched for the chunk
        nbytes += H * W * 3
        if nbytes >= LOAD_CHUNK_BYTES:
            imgs += flush()
    if preps:
        imgs += flush()
    return imgs


def _load_chunk(items, device, verbose):
    descs, srcs, shapes, off = [], [], [], 0
    for path, arr, H, W, target, crop_H, crop_W in items:
        src = arr if isinstance(arr, torch.Tensor) else _upload_u8(arr, device)   # decode="gpu": the pixels are on the device already
        h, w = (H, W) if target is None else target
        top, left = _center_offsets(H, W, crop_H, crop_W)
        descs.append(_desc(src, _lib.IMG_U8_HWC, 3, H, W, W * 3, 0, (top, left, crop_H, crop_W), (h, w), (0, 0, h, w), off))
        srcs.append(src)
        shapes.append((h, w))
        off += 3 * h * w
    out = torch.empty((off,), dtype=torch.float32, device=device)
    _resample(_lib.RESAMPLE_AA_BILINEAR, descs, out, srcs)
    imgs, off = [], 0
    for (path, _, H, W, *_), (h, w) in zip(items, shapes):
        imgs.append(dict(img=out[off:off + 3 * h * w].view(3, h, w), true_shape=np.int32([h, w])))
        off += 3 * h * w
        if verbose:
            print(f" - adding {path} with resolution {W}x{H} --> {w}x{h}")
    return imgs


def _frame_geometry(H1, W1, res):
    """must3r/slam/model.py:99-120 with dust3r's _resize_pil_image (dust3r/utils/image.py, un-vendored: LANCZOS when the long side
    shrinks, BICUBIC otherwise; new size = round(x * long_edge / long side) per axis) -> (mode, (H, W), crop (y0, x0, h, w), to_orig_focal)."""
    if H1 <= 0 or W1 <= 0:
        raise ValueError(f"must3r_amd.image: empty frame ({H1} x {W1})")
    longsize = res
    if res in _SQUARE_RES:
        longsize = max(W1, H1) / min(W1, H1) * res   # the short side has to reach res
    S = max(W1, H1)
    mode = _lib.RESAMPLE_PIL_LANCZOS if S > longsize else _lib.RESAMPLE_PIL_BICUBIC
    W, H = (int(round(x * longsize / S)) for x in (W1, H1))
    cx, cy = W // 2, H // 2
    if res in _SQUARE_RES:
        halfw = halfh = res // 2
    else:
        halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
    x0, y0 = cx - halfw, cy - halfh
    if x0 < 0 or y0 < 0 or cx + halfw > W or cy + halfh > H or halfw <= 0 or halfh <= 0:
        raise ValueError(f"must3r_amd.image: crop box {(x0, y0, cx + halfw, cy + halfh)} does not lie inside the {W} x {H} resized frame")
    return mode, (H, W), (y0, x0, 2 * halfh, 2 * halfw), W1 / W


def _frames_u8(frames):
    _check_cuda(frames, "frames")
    if frames.dtype != torch.uint8:
        raise ValueError(f"must3r_amd.image: frames must be uint8 (RGB bytes), got {frames.dtype}")
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"must3r_amd.image: expected [B, H, W, 3] uint8 frames, got {tuple(frames.shape)}")
    if frames.shape[0] == 0 or frames.shape[1] == 0 or frames.shape[2] == 0:
        raise ValueError(f"must3r_amd.image: empty frames {tuple(frames.shape)}")
    return frames.contiguous()


def _preprocess(frames, res):
    B, H1, W1 = (int(s) for s in frames.shape[:3])
    mode, (H, W), (y0, x0, h, w), to_orig_focal = _frame_geometry(H1, W1, res)
    out = torch.empty((B, 3, h, w), dtype=torch.float32, device=frames.device)
    descs = [_desc(frames[b], _lib.IMG_U8_HWC, 3, H1, W1, W1 * 3, 0, (0, 0, H1, W1), (H, W), (y0, x0, h, w), b * 3 * h * w)
             for b in range(B)]
    _resample(mode, descs, out, frames)
    return out, (h, w), (x0, y0), to_orig_focal


class _ImgNormSpec:
    """dust3r's ImgNorm = Compose([ToTensor(), Normalize((0.5,) * 3, (0.5,) * 3)]), which the library applies through its byte table."""

    def __repr__(self):
        return "must3r_amd.image.ImgNorm"


ImgNorm = _ImgNormSpec()


def _is_imgnorm(transform):
    """None, ImgNorm above, or a torchvision-style Compose([ToTensor(), Normalize(0.5, 0.5)]) such as dust3r's ImgNorm."""
    if transform is None or transform is ImgNorm:
        return True
    ops = getattr(transform, "transforms", None)
    if not isinstance(ops, (list, tuple)) or len(ops) != 2:
        return False
    to_tensor, normalize = ops
    if type(to_tensor).__name__ != "ToTensor" or type(normalize).__name__ != "Normalize":
        return False
    try:
        mean = [float(v) for v in np.ravel(normalize.mean)]
        std = [float(v) for v in np.ravel(normalize.std)]
    except (AttributeError, TypeError, ValueError):
        return False
    return len(mean) in (1, 3) and len(std) in (1, 3) and all(v == 0.5 for v in mean + std)


def preproc_frame(img, idx, res=512, transform=None):
    """must3r/slam/model.py:99-120 (same signature; its caller, slam/model.py:482, passes transform=ImgNorm): img HxWx3 uint8 (numpy,
    or a CUDA uint8 tensor) ->
    (dict(img=fp32 [1, 3, h, w] CUDA, true_shape=np.int32([[h, w]]), idx, instance=str(idx), offset=np.int32([[x0, y0]])), to_orig_focal).
    ``transform`` must be None or ImgNorm (dust3r's, or ``must3r_amd.image.ImgNorm``): the normalisation is built into the native call; any
    other transform is refused with ValueError."""
    if not _is_imgnorm(transform):
        raise ValueError(f"must3r_amd.image.preproc_frame: transform {transform!r} is not ImgNorm (ToTensor + Normalize(0.5, 0.5)); "
                         "the native path applies only that normalisation")
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise ValueError(f"must3r_amd.image: frames must be uint8 (RGB bytes), got {img.dtype}")
        if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] == 0 or img.shape[1] == 0:
            raise ValueError(f"must3r_amd.image: expected an HxWx3 frame, got {img.shape}")
        img = _upload_u8(img, torch.device("cuda", torch.cuda.current_device()))
    _check_cuda(img, "the frame")
    if img.dim() != 3:
        raise ValueError(f"must3r_amd.image: expected an HxWx3 frame, got {tuple(img.shape)}")
    out, (h, w), (x0, y0), to_orig_focal = _preprocess(_frames_u8(img[None]), res)
    return dict(img=out, true_shape=np.int32([[h, w]]), idx=idx, instance=str(idx), offset=np.int32([[x0, y0]])), to_orig_focal


def preprocess_frames(frames_u8, res=512):
    """``preproc_frame`` for a CUDA uint8 [B, H, W, 3] batch of one source size, in one native call ->
    (fp32 [B, 3, h, w] CUDA, true_shape np.int32 [B, 2])."""
    out, (h, w), _, _ = _preprocess(_frames_u8(frames_u8), res)
    return out, np.int32([[h, w]] * out.shape[0])


def resample_coeffs(mode, in_size, out_size):
    """Host coefficients of one axis (must3r_hip_resample_coeffs; no GPU needed) -> (bounds int32 [out, 2], weights [out, ksize])
    with int32 fixed-point weights for the PIL modes and fp32 otherwise."""
    lib = _lib.load()
    k = C.c_int(0)
    _lib.check(lib.must3r_hip_resample_coeffs(int(mode), int(in_size), int(out_size), C.byref(k), None, None))
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    pil = mode in (_lib.RESAMPLE_PIL_LANCZOS, _lib.RESAMPLE_PIL_BICUBIC)
    weights = np.zeros((out_size, k.value), dtype=np.int32 if pil else np.float32)
    _lib.check(lib.must3r_hip_resample_coeffs(int(mode), int(in_size), int(out_size), C.byref(k), bounds.ctypes.data_as(C.c_void_p),
                                              weights.ctypes.data_as(C.c_void_p)))
    return bounds, weights
