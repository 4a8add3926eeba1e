"""Baseline JPEG decoding on the GPU (csrc/jpeg_parse.hpp, csrc/jpeg_entropy.hpp, csrc/jpeg.hip; include/must3r_hip.h ABI 21, additive).

* ``probe(data)``            the parser alone (host, no GPU): a dict of the file's geometry when the native decoder takes it, ``None`` otherwise
                             (``refusal(data)`` gives the reason).
* ``decode_images(items, device)``  paths or ``bytes`` -> uint8 ``[H, W, 3]`` CUDA tensors, bit-equal to ``numpy.asarray(PIL.Image.open(f).convert("RGB"))``.
                             The compressed bytes travel through pinned memory; one native call per chunk of about ``image.LOAD_CHUNK_BYTES`` of pixels.  What
                             the parser refuses (progressive, CMYK, other samplings, PNG, ...) goes through Pillow and the upload ``load_images`` uses, exactly as
                             before.  Nothing is read back: the call returns with the work queued on the current stream.
* ``path_record()``          how many items took which path since ``reset_path_record()``: ``fast`` (the parallel entropy decode verified), ``sequential`` (the
                             verification failed and one thread per restart segment decoded the image again) or ``pillow``.  Reading it waits for the decodes.

Accepted: SOF0 / SOF1 with 8-bit samples, Huffman coding, one interleaved scan, grey or YCbCr with luma 1x1, 2x1 or 2x2; EXIF orientation is ignored, as
Pillow's ``open().convert()`` ignores it.  The test corpus is encoded by Pillow's encoder only: files of other encoders are covered by the parser's
refusals, not by pixels.
"""
import ctypes as C
import io
import os

import numpy as np
import torch

from . import _lib

_REASON_BYTES = 256
_MAX_BATCH = 4096          # images of one native call
_pending = []              # (flags tensor, count) of decode calls whose paths are not counted yet
_record = {"fast": 0, "sequential": 0, "pillow": 0}


def _alloc_u8(nbytes, device):
    """every device buffer of this module (tests wrap it with canaries)"""
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(os.fspath(item), "rb") as f:
        return f.read()


class _Parsed:
    __slots__ = ("info", "seg", "data")

    def __init__(self, info, seg, data):
        self.info, self.seg, self.data = info, seg, data


def _parse(data):
    """-> (_Parsed, None) or (None, reason)"""
    lib = _lib.load()
    info = _lib.JpegInfo()
    reason = C.create_string_buffer(_REASON_BYTES)
    buf = (C.c_char * len(data)).from_buffer_copy(data) if len(data) else (C.c_char * 1)()
    if lib.must3r_hip_jpeg_parse(buf, len(data), C.byref(info), None, 0, reason, _REASON_BYTES):
        return None, reason.value.decode("utf-8", "replace")
    seg = (C.c_uint32 * info.n_segments)()
    if lib.must3r_hip_jpeg_parse(buf, len(data), C.byref(info), seg, info.n_segments, reason, _REASON_BYTES):
        return None, reason.value.decode("utf-8", "replace")
    return _Parsed(info, seg, data), None


def refusal(data):
    """why the native decoder does not take ``data`` (a string), or ``None`` when it does"""
    return _parse(_read(data))[1]


def probe(data):
    """dict(width, height, components, sampling=(hs, vs), restart_interval, n_segments, n_blocks, scan_bytes) when the native decoder takes the file, else None"""
    p, _ = _parse(_read(data))
    if p is None:
        return None
    i = p.info
    return dict(width=i.width, height=i.height, components=i.components, sampling=(i.hs, i.vs), mode="L" if i.components == 1 else "RGB",
                restart_interval=i.restart_interval, n_segments=i.n_segments, n_blocks=i.n_blocks, scan_bytes=int(i.scan_bytes))


def _decode_chunk(parsed, device):
    """one native call: [_Parsed] -> [uint8 [H, W, 3] tensors], views of one output buffer"""
    lib = _lib.load()
    n = len(parsed)
    in_off, out_off, a, b = [], [], 0, 0
    for p in parsed:
        in_off.append(a)
        out_off.append(b)
        a += (len(p.data) + 15) & ~15
        b += (p.info.height * p.info.width * 3 + 15) & ~15
    host = torch.empty((a,), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for p, o in zip(parsed, in_off):
        hv[o:o + len(p.data)] = np.frombuffer(p.data, dtype=np.uint8)
    with torch.cuda.device(device):
        comp = _alloc_u8(a, device)
        comp.copy_(host, non_blocking=True)
        out = _alloc_u8(b, device)
        flags = _alloc_u8(4 * n, device)
        imgs = (_lib.JpegImage * n)()
        for k, p in enumerate(parsed):
            imgs[k] = _lib.JpegImage(C.pointer(p.info), p.seg, comp.data_ptr() + in_off[k], len(p.data), out.data_ptr() + out_off[k], p.info.width * 3)
        nbytes = lib.must3r_hip_jpeg_scratch_bytes(imgs, n)
        scratch = _alloc_u8(nbytes + 256, device)
        sp = (scratch.data_ptr() + 255) & ~255
        batch = _lib.JpegBatch(imgs, n, 0, flags.data_ptr(), sp, nbytes if nbytes else 256, _lib.stream_ptr(device))
        _lib.check(lib.must3r_hip_jpeg_decode(C.byref(batch)))
    # comp and scratch go back to the caching allocator here: it hands their blocks out again in the order of this stream; the pinned block is held by its copy
    if len(_pending) >= 256:
        path_record()
    _pending.append((flags, n))
    return [out[o:o + p.info.height * p.info.width * 3].view(p.info.height, p.info.width, 3) for p, o in zip(parsed, out_off)]


def _prepare(item):
    """read and parse one item -> ("gpu", _Parsed, H, W), or ("pil", HxWx3 uint8 array decoded by Pillow on the host, H, W) when the parser refuses it"""
    data = _read(item)
    p, _ = _parse(data)
    if p is not None:
        return "gpu", p, p.info.height, p.info.width
    import PIL.Image
    rgb = PIL.Image.open(io.BytesIO(data) if isinstance(item, (bytes, bytearray, memoryview)) else item).convert("RGB")
    rgb.load()
    arr = np.asarray(rgb)
    return "pil", arr, arr.shape[0], arr.shape[1]


def _decode_prepared(preps, device):
    """[_prepare(item)] -> [uint8 [H, W, 3] CUDA tensor], in order: the accepted ones in one native call (per _MAX_BATCH), the others uploaded as load_images does"""
    from .image import _upload_u8
    out = [None] * len(preps)
    idx = [k for k, p in enumerate(preps) if p[0] == "gpu"]
    for a in range(0, len(idx), _MAX_BATCH):
        part = idx[a:a + _MAX_BATCH]
        for k, t in zip(part, _decode_chunk([preps[k][1] for k in part], device)):
            out[k] = t
    for k, p in enumerate(preps):
        if p[0] == "pil":
            out[k] = _upload_u8(p[1], device)
            _record["pillow"] += 1
    return out


def _cuda_device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"must3r_amd.{who}: device must be CUDA; the HIP path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def decode_images(items, device="cuda", chunk_bytes=None):
    """paths or bytes -> [uint8 [H, W, 3] CUDA tensor per item, in order]; see the module docstring"""
    from . import image
    device = _cuda_device(device, "jpeg.decode_images")
    limit = image.LOAD_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    out, chunk, nbytes = [], [], 0
    for item in items:
        chunk.append(_prepare(item))
        nbytes += chunk[-1][2] * chunk[-1][3] * 3
        if nbytes >= limit:
            out += _decode_prepared(chunk, device)
            chunk, nbytes = [], 0
    if chunk:
        out += _decode_prepared(chunk, device)
    return out


def path_record():
    """dict(fast=, sequential=, pillow=): items per path since reset_path_record(); waits for the decode calls whose flags it has not read yet"""
    while _pending:
        flags, n = _pending.pop()
        f = flags[:4 * n].cpu().view(torch.int32)
        seq = int((f != _lib.JPEG_PATH_FAST).sum())
        _record["sequential"] += seq
        _record["fast"] += n - seq
    return dict(_record)


def reset_path_record():
    path_record()
    for k in _record:
        _record[k] = 0
