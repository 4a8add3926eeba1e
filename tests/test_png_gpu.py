"""GPU (-m gpu): the PNG decoder (must3r_amd.png, csrc/png.hip) against Pillow for the pixels and ``zlib.decompress`` for the inflated scanlines, bit for bit.

Every device buffer of the module is allocated between canaries here (``png._alloc_u8`` is wrapped): the zlib streams, the output, the status words, the scratch
and the scanline buffers of the tests' hook; the canaries are checked after every case.  The corpus is tests/png_cases.py's; the references are computed once
(``png_cases.references()``) and shared.  Damaged deflate streams run in tests/c/png_check.cpp on the host and never here: the three bad streams below are
valid deflate whose end is well defined.
"""
import io
import struct
import zlib

import numpy as np
import pytest
import torch

import png_cases as P
from must3r_amd import _lib, image, jpeg, png

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
PATTERN = 0xA5


@pytest.fixture(autouse=True)
def canaries(monkeypatch):
    held = []

    def alloc(nbytes, device):
        n = max(int(nbytes), 1)
        pad = (-n) % 256
        buf = torch.full((GUARD + n + pad + GUARD,), PATTERN, dtype=torch.uint8, device=device)
        held.append((buf, n))
        return buf[GUARD:GUARD + n]

    monkeypatch.setattr(png, "_alloc_u8", alloc)
    png.reset_path_record()
    yield held
    torch.cuda.synchronize()
    assert held, "the case allocated nothing through png._alloc_u8"
    for buf, n in held:
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n + ((-n) % 256):] == PATTERN).all()), f"a canary around a buffer of {n} bytes was written"


def _np(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


def _same(name, got, want):
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{name}: {len(bad)} elements differ from Pillow, the first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _decode(cases, **kw):
    """[(name, kind, data)] -> tensors in order, through decode_images and decode_gray"""
    out = [None] * len(cases)
    for kind, fn in (("rgb", png.decode_images), ("gray", png.decode_gray)):
        idx = [k for k, c in enumerate(cases) if c[1] == kind]
        for k, t in zip(idx, fn([cases[k][2] for k in idx], DEV, **kw)):
            out[k] = t
    return out


def _by_name(*names):
    by = {n: (n, k, d) for n, k, d in P.corpus()}
    return [by[n] for n in names]


# ---------------------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------------------
def test_corpus_is_bit_equal_to_pillow_and_never_on_the_pillow_path():
    cases = P.corpus()
    refs = P.references()
    for (name, kind, _), t in zip(cases, _decode(cases, check=True)):
        assert t.is_cuda
        _same(name, t, refs[name][1])
    rec = png.path_record()
    print(rec)
    assert rec == dict(gpu=len(cases), failed=0, pillow=0)


def test_inflated_scanlines_are_zlibs():
    """the tests' hook: the scanline buffer of every image, kept -- the inflated stream with the scanlines unfiltered in place.  Its filter-type bytes are
    zlib.decompress's, its other bytes are Pillow's samples in file order, and for the files of filter type 0 the whole buffer is zlib.decompress's output"""
    cases = P.corpus()
    refs = P.references()
    parsed = [png._parse(d, n)[0] for n, _, d in cases]
    fmts = [_lib.PNG_OUT_GRAY16 if p.info.bit_depth == 16 else _lib.PNG_OUT_GRAY8 if k == "gray" else _lib.PNG_OUT_RGB8 for p, (_, k, _) in zip(parsed, cases)]
    outs, status, kept = png._decode_chunk(parsed, fmts, torch.device(DEV, torch.cuda.current_device()), keep_inflated=True)
    assert not status.cpu().view(torch.int32).any()
    whole = 0
    for (name, kind, data), p, buf in zip(cases, parsed, kept):
        want = np.frombuffer(refs[name][0], np.uint8).reshape(p.info.height, 1 + p.info.rowbytes)
        got = buf.cpu().numpy().reshape(want.shape)
        assert np.array_equal(got[:, 0], want[:, 0]), name
        if not want[:, 0].any():
            assert np.array_equal(got, want), name
            whole += 1
        import PIL.Image
        px = np.asarray(PIL.Image.open(io.BytesIO(data)))
        samples = px.astype(">u2").view(np.uint8) if px.dtype == np.uint16 else px
        assert np.array_equal(got[:, 1:], samples.reshape(p.info.height, -1)), name
    assert whole >= 5


def test_alone_equals_batch_and_calls_repeat():
    names = ["size_8x130_L16g", "size_63x130_RGB8", "filter4_every_row_RGBA8", "pillow_level6_L8", "filter3_every_row_L8g", "big_256x300_L16g", "z_rle",
             "period_32768_far_matches", "stored_0_and_65535"]
    cases = _by_name(*names)
    assert {(png.probe(d)["mode"], k) for _, k, d in cases} == {("L", "rgb"), ("L", "gray"), ("I;16", "gray"), ("RGB", "rgb"), ("RGBA", "rgb")}
    together = _decode(cases)
    again = _decode(cases)
    refs = P.references()
    for k, c in enumerate(cases):
        (alone,) = _decode([c])
        _same(c[0], together[k], refs[c[0]][1])
        assert np.array_equal(_np(alone), _np(together[k])) and np.array_equal(_np(again[k]), _np(together[k])), c[0]
    small = png.decode_images([c[2] for c in cases if c[1] == "rgb"], DEV, chunk_bytes=1)       # one native call per image
    assert all(np.array_equal(_np(a), _np(together[k])) for a, k in zip(small, [k for k, c in enumerate(cases) if c[1] == "rgb"]))
    assert png.path_record()["failed"] == 0


def test_refused_files_between_accepted_ones_come_back_in_order(tmp_path):
    import PIL.Image
    rgb = P.synthetic(50, 40, 9, "RGB8")
    jpg, pal = io.BytesIO(), io.BytesIO()
    PIL.Image.fromarray(rgb).save(jpg, "JPEG")
    PIL.Image.fromarray(rgb).convert("P").save(pal, "PNG")
    path = tmp_path / "file.png"
    path.write_bytes(P.write_png(P.synthetic(31, 22, 10, "RGBA8"), filters=4))
    deep = P.write_png(P.synthetic(20, 10, 11, "L16g"), filters=1)           # 16-bit grey: Pillow's I;16 -> RGB clips, it stays on Pillow in decode_images
    items = [P.write_png(rgb, filters=2), pal.getvalue(), str(path), jpg.getvalue(), deep, path, P.write_png(rgb[..., 0], filters=3)]
    outs = png.decode_images(items, DEV, check=True)
    for k, (item, out) in enumerate(zip(items, outs)):
        src = item if isinstance(item, bytes) else open(item, "rb").read()
        assert np.array_equal(out.cpu().numpy(), np.asarray(PIL.Image.open(io.BytesIO(src)).convert("RGB"))), k
    assert png.path_record() == dict(gpu=4, failed=0, pillow=3)
    png.reset_path_record()
    mask = (rgb[..., 0] > 100).astype(np.uint8) * 255
    outs = png.decode_gray([deep, P.pillow_png(mask), P.write_png(mask, filters=0)], DEV, check=True)
    assert outs[0].dtype == torch.uint16 and outs[1].dtype == torch.uint8 and torch.equal(outs[1], outs[2])
    assert np.array_equal(_np(outs[0]), P.pillow_pixels(deep, "gray")) and np.array_equal(_np(outs[1]), mask)
    with pytest.raises(ValueError):
        png.decode_gray([P.write_png(rgb, filters=0)], DEV)                 # Pillow's mode RGB: no grey image
    assert png.path_record() == dict(gpu=3, failed=0, pillow=0)


def test_everything_runs_on_the_callers_stream():
    """in the manner of tests/test_stream_order_gpu.py: the reference bits on the default stream; a decoy batch of the same sizes, so that the buffers the allocator
    hands out again hold the decoy's bytes; then the call on a side stream behind a delay"""
    from test_stream_order_gpu import Delay
    delay = Delay()
    A = [P.write_png(P.synthetic(160, 120, 60 + i, f), filters=(4, 1, 3)) for i, f in enumerate(("RGB8", "RGBA8", "L8"))]
    B = [P.write_png(P.synthetic(160, 120, 90 + i, f), filters=(4, 1, 3)) for i, f in enumerate(("RGB8", "RGBA8", "L8"))]
    ref = [t.clone() for t in png.decode_images(A, DEV)]
    decoy = [t.clone() for t in png.decode_images(B, DEV)]
    torch.cuda.synchronize()
    assert all(not torch.equal(a, b) for a, b in zip(ref, decoy))
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        png.decode_images(B, DEV)       # the side stream's own blocks hold the decoy too
        delay.enqueue(60.0)
        done.record()
        outs = png.decode_images(A, DEV)
        premise = not done.query()
        got = [t.clone() for t in outs]
    s.synchronize()
    assert premise, "the delay ended before the call returned on the host: a host synchronisation inside decode_images, or a delay too short"
    for k, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), f"image {k} on a side stream differs from the default-stream bits (the decoy's: {torch.equal(g, decoy[k])})"
    assert png.path_record() == dict(gpu=12, failed=0, pillow=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# valid streams with a well-defined bad end
# ---------------------------------------------------------------------------------------------------------------------------------
def _bad_streams():
    px = P.synthetic(70, 50, 21, "RGB8")
    raw = P.scanlines(px, 4)
    good = zlib.compress(raw, 6)
    wrong_adler = good[:-4] + struct.pack(">I", (zlib.adler32(raw) ^ 0x00010000) & 0xFFFFFFFF)
    short = zlib.compress(raw[:-211], 6)          # a complete zlib stream of one row less than the header's size needs
    long = zlib.compress(raw + raw[:300], 6)      # and of more
    return px, {"wrong_adler": (wrong_adler, "Adler"), "short": (short, "size"), "long": (long, "beyond")}


@pytest.mark.parametrize("which", ["wrong_adler", "short", "long"])
def test_bad_end_sets_the_status_and_nothing_else(which):
    px, streams = _bad_streams()
    stream, word = streams[which]
    bad = P.write_png(px, stream=stream)
    raw_deflate = zlib.decompressobj(-15)        # the deflate data itself is valid in all three
    assert png.probe(bad) is not None and len(raw_deflate.decompress(stream[2:])) == 50 * 211 + {"wrong_adler": 0, "short": -211, "long": 300}[which] and raw_deflate.eof
    others = _by_name("filters_rotating_RGB8", "pillow_level6_RGBA8")
    refs = P.references()
    items = [others[0][2], bad, others[1][2]]
    outs = png.decode_images(items, DEV)
    assert tuple(outs[1].shape) == (50, 70, 3)
    _same(others[0][0], outs[0], refs[others[0][0]][1])
    _same(others[1][0], outs[2], refs[others[1][0]][1])
    assert png.path_record() == dict(gpu=2, failed=1, pillow=0)
    with pytest.raises(ValueError, match=f"item 1.*{word}"):
        png.decode_images(items, DEV, check=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# load_images and the training side
# ---------------------------------------------------------------------------------------------------------------------------------
def test_load_images_png_gpu_equals_pil(tmp_path):
    import PIL.Image
    import jpeg_ref as R
    files = []
    for i, (w, h, s) in enumerate(((640, 480, "420"), (300, 533, "444"))):
        files.append(str(tmp_path / f"{i}.jpg"))
        with open(files[-1], "wb") as f:
            f.write(R.encode(R.synthetic(w, h, 70 + i), sampling=s, quality=88))
    for i, fmt in enumerate(("RGB8", "RGBA8", "L8", "L16g")):                 # the last: 16-bit grey, which stays on Pillow
        files.append(str(tmp_path / f"{i}.png"))
        with open(files[-1], "wb") as f:
            f.write(P.write_png(P.synthetic(400 + 37 * i, 300 + 11 * i, 80 + i, fmt), filters=(4, 2, 1, 3, 0)))
    files.append(str(tmp_path / "pal.png"))
    PIL.Image.fromarray(P.synthetic(320, 240, 90, "RGB8")).convert("P").save(files[-1])
    jpeg.reset_path_record()
    pil = image.load_images(files, 512, verbose=False, decode="pil")
    gpu = image.load_images(files, 512, verbose=False, decode="gpu", png="gpu")
    jrec = jpeg.path_record()
    assert png.path_record() == dict(gpu=3, failed=0, pillow=0) and jrec["fast"] + jrec["sequential"] == 2 and jrec["pillow"] == 2
    half = image.load_images(files, 512, verbose=False, decode="gpu")         # the default: every PNG with Pillow
    assert png.path_record()["gpu"] == 3 and jpeg.path_record()["pillow"] == 2 + 5
    assert len(pil) == len(gpu) == len(half) == len(files)
    for k, (a, b, c) in enumerate(zip(pil, gpu, half)):
        assert np.array_equal(a["true_shape"], b["true_shape"]) and torch.equal(a["img"], b["img"]) and torch.equal(a["img"], c["img"]), k


def test_decode_gray_feeds_augment_views():
    """decode_gray's uint16 depth into augment_views against the same depth uploaded from numpy: the same views, bit for bit"""
    from must3r_amd import train_augment as TA
    depth = P.synthetic(131, 97, 33, "L16g")
    depth[10:20, 30:50] = 0                       # holes
    (dev_depth,) = png.decode_gray([P.pillow_png(depth)], DEV, check=True)
    assert dev_depth.dtype == torch.uint16 and np.array_equal(_np(dev_depth), depth)
    up = torch.from_numpy(depth.view(np.int16)).to(DEV).view(torch.uint16)
    rgb = torch.from_numpy(P.synthetic(131, 97, 34, "RGB8")).to(DEV)
    K = torch.tensor([[120.0, 0, 64.3], [0, 121.0, 47.9], [0, 0, 1]])

    def run(d):
        return TA.augment_views([rgb, rgb], [d, d], [K, K], (64, 48), rng=np.random.default_rng(5), aug_crop=8)

    a, b = run(dev_depth), run(up)
    assert a["depthmap"].dtype == torch.uint16 and tuple(a["depthmap"].shape) == (2, 48, 64) and int(a["depthmap"].view(torch.int16).count_nonzero()) > 0
    for key in ("img", "depthmap", "camera_intrinsics", "true_shape"):
        x, y = (o[key].view(torch.int16) if o[key].dtype == torch.uint16 else o[key] for o in (a, b))
        assert torch.equal(x, y), key
