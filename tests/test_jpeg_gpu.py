"""GPU (-m gpu): the JPEG decoder (must3r_amd.jpeg, csrc/jpeg.hip) against ``numpy.asarray(PIL.Image.open(f).convert("RGB"))``, bit for bit.

Every device buffer of the module is allocated between canaries here (``jpeg._alloc_u8`` is wrapped): the compressed bytes, the output, the path flags and the
scratch; the canaries are checked after every case.  The corpus is tests/jpeg_ref.py's (Pillow's encoder, seeded synthetic images).
"""
import io

import numpy as np
import pytest
import torch

import jpeg_ref as R
from must3r_amd import image, jpeg
from test_jpeg_host import _noise, tile_image

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

    monkeypatch.setattr(jpeg, "_alloc_u8", alloc)
    jpeg.reset_path_record()
    yield held
    torch.cuda.synchronize()
    assert held, "the case allocated nothing through jpeg._alloc_u8"
    for buf, n in held:
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n + ((-n) % 256):] == PATTERN).all()), f"a canary around a buffer of {n} bytes was written"


def _check(datas, names=None):
    outs = jpeg.decode_images(datas, DEV)
    assert len(outs) == len(datas)
    for k, (data, out) in enumerate(zip(datas, outs)):
        want = R.pillow_rgb(data)
        assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == want.shape, (names[k] if names else k, tuple(out.shape), want.shape)
        got = out.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{names[k] if names else k}: {len(bad)} bytes differ from Pillow, the first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 / 2: bit-equality with Pillow and the path record
# ---------------------------------------------------------------------------------------------------------------------------------
def test_corpus_is_bit_equal_to_pillow_and_never_on_the_pillow_path():
    corpus = R.corpus()
    _check([d for _, d in corpus], [n for n, _ in corpus])
    rec = jpeg.path_record()
    print(rec)
    assert rec["pillow"] == 0 and rec["fast"] + rec["sequential"] == len(corpus) == 200


NOISE = [(s, r) for s in ("420", "444") for r in (None, "rows")]


@pytest.fixture(scope="module")
def noise_files():
    img = _noise()
    return {(s, r): R.encode(img, sampling=s, quality=95, restart=r) for s, r in NOISE}


def test_noise_images_take_the_fast_path(noise_files):
    """640 x 480 noise at quality 95: several thousand subsequences, more than one thread block per segment without restart markers"""
    datas = [noise_files[k] for k in NOISE]
    for k, d in zip(NOISE, datas):
        info = jpeg.probe(d)
        assert info["scan_bytes"] // 128 > (2000 if k[1] is None else 0) and info["n_segments"] == (1 if k[1] is None else (30 if k[0] == "420" else 60))
    _check(datas, [str(k) for k in NOISE])
    rec = jpeg.path_record()
    assert rec == dict(fast=4, sequential=0, pillow=0), rec


@pytest.mark.parametrize("value", [128, 0, 255])
def test_constant_images(value):
    """every block is "DC 0, EOB": a periodic stream.  Whichever path they take, the pixels are Pillow's."""
    datas = [R.encode(np.full((h, w, 3), value, np.uint8)) for w, h in ((64, 64), (640, 480))]
    _check(datas)
    rec = jpeg.path_record()
    print(value, rec)
    assert rec["pillow"] == 0 and rec["fast"] + rec["sequential"] == 2


def test_periodic_texture_takes_the_exact_path():
    """an 8 x 8 tile repeated over 640 x 480: the synchronisation never settles (the host emulation, tests/test_jpeg_host.py, shows the same), the verification
    fails and one thread per segment decodes the image again -- alone, and in a batch whose other images stay on the fast path"""
    tile = R.encode(tile_image(), sampling="420", quality=90)
    other = R.encode(R.synthetic(200, 120, 4), sampling="444", quality=80)
    _check([tile])
    assert jpeg.path_record() == dict(fast=0, sequential=1, pillow=0)
    jpeg.reset_path_record()
    _check([other, tile, other])
    assert jpeg.path_record() == dict(fast=2, sequential=1, pillow=0)


def test_smallest_and_widest():
    datas = [R.encode(R.synthetic(1, 1, 3)), R.encode(R.synthetic(4000, 3, 9)), R.encode(R.synthetic(4000, 3, 9), sampling="444", restart="blocks"),
             R.encode(R.synthetic(3, 700, 2, grey=True))]
    _check(datas)
    assert jpeg.path_record()["pillow"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: batch properties
# ---------------------------------------------------------------------------------------------------------------------------------
def _mixed():
    cases = [(97, 61, "420", 75, None), (640, 360, "422", 90, "rows"), (33, 200, "grey", 95, None), (256, 256, "444", 100, "blocks"), (500, 333, "420", 85, None)]
    return [R.encode(R.synthetic(w, h, 40 + i, grey=s == "grey"), sampling=s, quality=q, restart=r) for i, (w, h, s, q, r) in enumerate(cases)]


def test_alone_equals_batch_and_calls_repeat():
    datas = _mixed()
    together = _check(datas)
    again = jpeg.decode_images(datas, DEV)
    for k, d in enumerate(datas):
        (alone,) = jpeg.decode_images([d], DEV)
        assert torch.equal(alone, together[k]) and torch.equal(again[k], together[k]), k
    small = jpeg.decode_images(datas, DEV, chunk_bytes=1)       # one native call per image
    assert all(torch.equal(a, b) for a, b in zip(small, together))


def test_mixed_accepted_refused_and_png_in_order(tmp_path):
    import PIL.Image
    img = R.synthetic(120, 90, 8)
    png = io.BytesIO()
    PIL.Image.fromarray(img).save(png, "PNG")
    path = tmp_path / "file.jpg"
    path.write_bytes(R.encode(R.synthetic(75, 50, 9), sampling="422"))
    items = [R.encode(img), R.encode(img, progressive=True), png.getvalue(), str(path), R.encode(img[..., 0]), path]
    outs = jpeg.decode_images(items, DEV)
    for k, (item, out) in enumerate(zip(items, outs)):
        src = item if isinstance(item, bytes) else open(item, "rb").read()
        assert np.array_equal(out.cpu().numpy(), np.asarray(PIL.Image.open(io.BytesIO(src)).convert("RGB"))), k
    assert jpeg.path_record() == dict(fast=4, sequential=0, pillow=2)


def test_everything_runs_on_the_callers_stream():
    """in the manner of tests/test_stream_order_gpu.py: the reference bits on the default stream; a decoy batch of the same sizes, so that the buffers the allocator
    hands out again hold the decoy's bytes; then the call on a side stream behind a delay.  A copy, memset or launch on another stream runs before the upload
    queued behind the delay and reads the decoy."""
    from test_stream_order_gpu import Delay
    delay = Delay()
    A = [R.encode(R.synthetic(320, 240, 60 + i), sampling=s, quality=90, restart=r) for i, (s, r) in enumerate((("420", None), ("444", "rows"), ("422", None)))]
    B = [R.encode(R.synthetic(320, 240, 90 + i), sampling=s, quality=90, restart=r) for i, (s, r) in enumerate((("420", None), ("444", "rows"), ("422", None)))]
    ref = [t.clone() for t in jpeg.decode_images(A, DEV)]
    decoy = [t.clone() for t in jpeg.decode_images(B, DEV)]
    torch.cuda.synchronize()
    assert all(not torch.equal(a, b) for a, b in zip(ref, decoy))
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        jpeg.decode_images(B, DEV)       # the side stream's own blocks hold the decoy too
        delay.enqueue(60.0)
        done.record()
        outs = jpeg.decode_images(A, DEV)
        premise = not done.query()
        got = [t.clone() for t in outs]
    s.synchronize()
    assert premise, "the delay ended before the call returned on the host: a host synchronisation inside decode_images, or a delay too short"
    for k, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), f"image {k} on a side stream differs from the default-stream bits (the decoy's: {torch.equal(g, decoy[k])})"
    assert jpeg.path_record()["pillow"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: load_images
# ---------------------------------------------------------------------------------------------------------------------------------
def test_load_images_gpu_equals_pil(tmp_path, monkeypatch):
    import PIL.Image
    files = []
    for i, (w, h, s) in enumerate(((640, 480, "420"), (517, 389, "444"), (300, 533, "422"), (1024, 576, "420"), (384, 512, "grey"))):
        files.append(str(tmp_path / f"{i}.jpg"))
        with open(files[-1], "wb") as f:
            f.write(R.encode(R.synthetic(w, h, 70 + i, grey=s == "grey"), sampling=s, quality=88))
    files.append(str(tmp_path / "5.png"))
    PIL.Image.fromarray(R.synthetic(400, 300, 77)).save(files[-1])
    pil = image.load_images(files, 512, verbose=False, decode="pil")
    default = image.load_images(files, 512, verbose=False)
    gpu = image.load_images(files, 512, verbose=False, decode="gpu")
    assert jpeg.path_record() == dict(fast=5, sequential=0, pillow=1)
    monkeypatch.setattr(image, "LOAD_CHUNK_BYTES", 1 << 20)     # several chunks
    chunked = image.load_images(files, 512, verbose=False, decode="gpu")
    assert len(pil) == len(gpu) == len(default) == len(chunked) == len(files)
    for k, (a, b, c, d) in enumerate(zip(pil, gpu, default, chunked)):
        assert np.array_equal(a["true_shape"], b["true_shape"]) and np.array_equal(a["true_shape"], c["true_shape"]), k
        assert a["img"].dtype == torch.float32 and torch.equal(a["img"], b["img"]) and torch.equal(a["img"], c["img"]) and torch.equal(a["img"], d["img"]), k
