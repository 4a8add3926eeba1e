"""PNG decoding on the GPU (csrc/png_parse.hpp, csrc/png_inflate.hpp, csrc/png.hip; include/must3r_hip.h ABI 21, additive).

* ``probe(data)``            the parser alone (host, no GPU): a dict of the file's geometry when the native decoder takes it, ``None`` otherwise
                             (``refusal(data)`` gives the reason).
* ``decode_images(items, device)``  paths or ``bytes`` -> uint8 ``[H, W, 3]`` CUDA tensors, bit-equal to ``numpy.asarray(PIL.Image.open(f).convert("RGB"))``:
                             8-bit grey, RGB and RGBA files.  16-bit grey is refused here (Pillow's ``I;16 -> RGB`` clips to 255: it stays on Pillow), and so is
                             everything the parser refuses: those items go through Pillow and the upload ``load_images`` uses.
* ``decode_gray(items, device)``  the depth and mask loader: ``[H, W]`` uint8 or uint16 CUDA tensors, bit-equal to ``numpy.asarray(PIL.Image.open(f))`` for
                             Pillow's modes ``L`` and ``I;16``.  The uint16 output is what ``train_augment.augment_views(depths=...)`` and
                             ``train_data.ground_truth(..., depth_scale=)`` take; co3d's float16 depth is ``.view(torch.float16)`` of it.  What is not colour type 0
                             goes through Pillow when Pillow's mode is ``L`` or ``I;16``, and is a ``ValueError`` otherwise.
* ``path_record()``          ``dict(gpu=, failed=, pillow=)``: items per path since ``reset_path_record()``; ``failed`` counts the images whose status word the
                             device set (a damaged stream: unspecified, in-bounds pixels).  Reading it waits for the decodes.

The IDAT payloads of a file are copied back to back into the pinned upload buffer: the device sees one contiguous zlib stream per image.  Nothing is read back
and the call returns with the work queued on the current stream, unless ``check=True``: then the call waits, reads the status words and raises ``ValueError``
naming the first failed item.
"""
import ctypes as C
import io
import os

import numpy as np
import torch

from . import _lib

_REASON_BYTES = 256
_MAX_BATCH = 4096          # images of one native call
GRAY_CHUNK_BYTES = 2 << 30  # decode_gray: pixels of one native call.  A stream is one workgroup, so a call wants hundreds of images: 280 depth frames are 1.1 GB
_pending = []              # (status tensor, count) of decode calls whose status words are not counted yet
_record = {"gpu": 0, "failed": 0, "pillow": 0}
_FORMAT = {"rgb": _lib.PNG_OUT_RGB8, "L": _lib.PNG_OUT_GRAY8, "I;16": _lib.PNG_OUT_GRAY16}
_OUT_BYTES = {_lib.PNG_OUT_RGB8: 3, _lib.PNG_OUT_GRAY8: 1, _lib.PNG_OUT_GRAY16: 2}


def _alloc_u8(nbytes, device):
    """every device buffer of this module (tests wrap it with canaries)"""
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(os.fspath(item), "rb") as f:
        return f.read()


class _Parsed:
    __slots__ = ("info", "ranges", "data", "name")

    def __init__(self, info, ranges, data, name):
        self.info, self.ranges, self.data, self.name = info, ranges, data, name


def _parse(data, name=None):
    """-> (_Parsed, None) or (None, reason)"""
    lib = _lib.load()
    info = _lib.PngInfo()
    reason = C.create_string_buffer(_REASON_BYTES)
    buf = (C.c_char * len(data)).from_buffer_copy(data) if len(data) else (C.c_char * 1)()
    if lib.must3r_hip_png_parse(buf, len(data), C.byref(info), None, 0, reason, _REASON_BYTES):
        return None, reason.value.decode("utf-8", "replace")
    ranges = (_lib.PngRange * info.n_idat)()
    if lib.must3r_hip_png_parse(buf, len(data), C.byref(info), ranges, info.n_idat, reason, _REASON_BYTES):
        return None, reason.value.decode("utf-8", "replace")
    return _Parsed(info, ranges, data, name), None


def refusal(data):
    """why the native decoder does not take ``data`` (a string), or ``None`` when it does"""
    return _parse(_read(data))[1]


def probe(data):
    """dict(width, height, color_type, bit_depth, channels, mode, rowbytes, inflated_bytes, n_idat, idat_bytes) when the native decoder takes the file, else None;
    ``mode`` is Pillow's: L, I;16, RGB or RGBA"""
    p, _ = _parse(_read(data))
    if p is None:
        return None
    i = p.info
    return dict(width=i.width, height=i.height, color_type=i.color_type, bit_depth=i.bit_depth, channels=i.channels, mode=_mode(i),
                rowbytes=int(i.rowbytes), inflated_bytes=int(i.inflated_bytes), n_idat=i.n_idat, idat_bytes=int(i.idat_bytes))


def _mode(info):
    return {(0, 8): "L", (0, 16): "I;16", (2, 8): "RGB", (6, 8): "RGBA"}[(info.color_type, info.bit_depth)]


def _up(x, a):
    return (x + a - 1) & ~(a - 1)


def _decode_chunk(parsed, formats, device, keep_inflated=False):
    """one native call: [_Parsed], [MUST3R_PNG_OUT_*] -> ([tensors, views of one output buffer], status tensor); with ``keep_inflated`` (the tests' hook) also
    the scanline buffers: per image the inflated zlib stream with the scanlines unfiltered in place"""
    lib = _lib.load()
    n = len(parsed)
    in_off, out_off, inf_off, a, b, c = [], [], [], 0, 0, 0
    for p, fmt in zip(parsed, formats):
        in_off.append(a)
        out_off.append(b)
        inf_off.append(c)
        a += _up(int(p.info.idat_bytes), 16)
        b += _up(p.info.height * p.info.width * _OUT_BYTES[fmt], 16)
        c += _up(int(p.info.inflated_bytes), 256) + 256
    host = torch.zeros((a,), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for p, o in zip(parsed, in_off):
        src = np.frombuffer(p.data, dtype=np.uint8)
        for r in p.ranges:   # the IDAT payloads back to back: one zlib stream
            hv[o:o + r.length] = src[r.offset:r.offset + r.length]
            o += r.length
    with torch.cuda.device(device):
        comp = _alloc_u8(a, device)
        comp.copy_(host, non_blocking=True)
        out = _alloc_u8(b, device)
        status = _alloc_u8(4 * n, device)
        inflated, ip = None, 0
        if keep_inflated:
            inflated = _alloc_u8(c + 256, device)
            ip = (inflated.data_ptr() + 255) & ~255
        imgs = (_lib.PngImage * n)()
        for k, (p, fmt) in enumerate(zip(parsed, formats)):
            imgs[k] = _lib.PngImage(C.pointer(p.info), comp.data_ptr() + in_off[k], out.data_ptr() + out_off[k], p.info.width * _OUT_BYTES[fmt], fmt, 0,
                                    ip + inf_off[k] if keep_inflated else None)
        nbytes = lib.must3r_hip_png_scratch_bytes(imgs, n)
        if nbytes == 0:
            raise _lib.HipError(lib.must3r_hip_last_error().decode("utf-8", "replace"))
        scratch = _alloc_u8(nbytes + 256, device)
        sp = (scratch.data_ptr() + 255) & ~255
        batch = _lib.PngBatch(imgs, n, 0, status.data_ptr(), sp, nbytes, _lib.stream_ptr(device))
        _lib.check(lib.must3r_hip_png_decode(C.byref(batch)))
    # comp and scratch go back to the caching allocator here: it hands their blocks out again in the order of this stream; the pinned block is held by its copy
    if len(_pending) >= 256:
        path_record()
    _pending.append((status, n))
    outs = []
    for p, fmt, o in zip(parsed, formats, out_off):
        H, W = p.info.height, p.info.width
        flat = out[o:o + H * W * _OUT_BYTES[fmt]]
        outs.append(flat.view(H, W, 3) if fmt == _lib.PNG_OUT_RGB8 else flat.view(H, W) if fmt == _lib.PNG_OUT_GRAY8 else flat.view(torch.uint16).view(H, W))
    if keep_inflated:
        base = ip - inflated.data_ptr()
        return outs, status, [inflated[base + o:base + o + int(p.info.inflated_bytes)] for p, o in zip(parsed, inf_off)]
    return outs, status


def _name(item, k):
    return f"item {k}" if isinstance(item, (bytes, bytearray, memoryview)) else f"item {k} ({os.fspath(item)})"


def _prepare(item, kind, k=0):
    """read and parse one item -> ("gpu", _Parsed, H, W, MUST3R_PNG_OUT_*), or ("pil", array decoded by Pillow on the host, H, W, None) when the native path does
    not take it.  kind "rgb": the array is HxWx3 uint8; kind "gray": HxW uint8 or uint16"""
    data = _read(item)
    p, _ = _parse(data, _name(item, k))
    if p is not None:
        mode = _mode(p.info)
        if kind == "rgb" and mode != "I;16":
            return "gpu", p, p.info.height, p.info.width, _FORMAT["rgb"]
        if kind == "gray" and mode in ("L", "I;16"):
            return "gpu", p, p.info.height, p.info.width, _FORMAT[mode]
    import PIL.Image
    im = PIL.Image.open(io.BytesIO(data))
    if kind == "rgb":
        im = im.convert("RGB")
    elif im.mode not in ("L", "I;16"):
        raise ValueError(f"must3r_amd.png.decode_gray: {_name(item, k)} has Pillow mode {im.mode!r} (L or I;16)")
    im.load()
    arr = np.asarray(im)
    return "pil", arr, arr.shape[0], arr.shape[1], None


def _upload(arr, device):
    """a numpy array -> CUDA tensor of its dtype through pinned host memory (asynchronous copy on the current stream)"""
    if arr.dtype == np.uint8 and arr.ndim == 3:
        from .image import _upload_u8
        return _upload_u8(arr, device)
    host = torch.empty(arr.shape, dtype=torch.uint16 if arr.dtype == np.uint16 else torch.uint8, pin_memory=True)
    host.numpy()[...] = arr
    return host.to(device, non_blocking=True)


def _decode_prepared(preps, device, check=False):
    """[_prepare(item)] -> [CUDA tensor], in order: the accepted ones in one native call (per _MAX_BATCH), the others uploaded as load_images does"""
    out = [None] * len(preps)
    idx = [k for k, p in enumerate(preps) if p[0] == "gpu"]
    for a in range(0, len(idx), _MAX_BATCH):
        part = idx[a:a + _MAX_BATCH]
        tensors, status = _decode_chunk([preps[k][1] for k in part], [preps[k][4] for k in part], device)
        for k, t in zip(part, tensors):
            out[k] = t
        if check:
            words = status[:4 * len(part)].cpu().view(torch.int32).tolist()   # waits for the call
            for k, w in zip(part, words):
                if w:
                    raise ValueError(f"must3r_amd.png: {preps[k][1].name}: the stream is damaged ({_lib.PNG_STATUS.get(w, w)})")
    for k, p in enumerate(preps):
        if p[0] == "pil":
            out[k] = _upload(p[1], device)
            _record["pillow"] += 1
    return out


def _decode(items, kind, device, limit, check):
    from . import jpeg
    device = jpeg._cuda_device(device, "png.decode_images" if kind == "rgb" else "png.decode_gray")
    out, chunk, nbytes = [], [], 0
    for k, item in enumerate(items):
        chunk.append(_prepare(item, kind, k))
        nbytes += chunk[-1][2] * chunk[-1][3] * (3 if kind == "rgb" else 2)
        if nbytes >= limit:
            out += _decode_prepared(chunk, device, check)
            chunk, nbytes = [], 0
    if chunk:
        out += _decode_prepared(chunk, device, check)
    return out


def decode_images(items, device="cuda", chunk_bytes=None, check=False):
    """paths or bytes -> [uint8 [H, W, 3] CUDA tensor per item, in order]; see the module docstring"""
    from . import image
    return _decode(items, "rgb", device, image.LOAD_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes), check)


def decode_gray(items, device="cuda", check=False):
    """paths or bytes -> [uint8 or uint16 [H, W] CUDA tensor per item, in order]; see the module docstring"""
    return _decode(items, "gray", device, GRAY_CHUNK_BYTES, check)


def path_record():
    """dict(gpu=, failed=, pillow=): items per path since reset_path_record(); waits for the decode calls whose status words it has not read yet"""
    while _pending:
        status, n = _pending.pop()
        f = status[:4 * n].cpu().view(torch.int32)
        failed = int((f != 0).sum())
        _record["failed"] += failed
        _record["gpu"] += n - failed
    return dict(_record)


def reset_path_record():
    path_record()
    for k in _record:
        _record[k] = 0
