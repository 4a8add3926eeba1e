"""No GPU: the PNG decoder's corpus, parser and shared routines (tests/png_cases.py; must3r_amd/csrc/png_parse.hpp, png_inflate.hpp; must3r_amd.png).

1. The corpus holds the stated cases.
2. The parser against Pillow's own size and mode on every corpus file, and its refusals -- each with a reason, none with an exception from C.
3. Seeded byte flips of one file each either parse or give a reason.
4. tests/c/png_check.cpp, a stand-alone program built with -fsanitize=address,undefined and run as a child process with nothing preloaded: the parser and the
   text the kernels compile, sequentially over the corpus (against zlib.decompress and Pillow) and over damaged variants of it, with coverage counters that
   keep the corpus from passing a decoder that gets a rare case wrong.
5. load_images' ``png`` keyword is checked before the device is touched.
"""
import ctypes as C
import io
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as P
from conftest import ROOT
from must3r_amd import _lib, png


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the corpus
# ---------------------------------------------------------------------------------------------------------------------------------
def test_corpus_holds_the_stated_cases():
    names = {n for n, _, _ in P.corpus()}
    sizes = P.size_cases()
    assert len(sizes) == 54 and {(w, h) for _, _, w, h in sizes} == {(w, h) for w in P.WIDTHS for h in P.HEIGHTS}
    assert {f for _, f, _, _ in sizes} == set(P.FORMATS) and all(n in names for n, _, _, _ in sizes)
    for fmt in P.FORMATS:      # every format crosses the 64-row group boundary
        assert {h for _, f, _, h in sizes if f == fmt} >= {64, 65, 130}, fmt
    want = ["big_256x300_L16g", "filters_rotating_RGB8", "level0_stored_only", "stored_0_and_65535", "z_fixed", "z_huffman_only", "z_rle", "level1", "level6",
            "level9", "wbits9", "full_flush_every_3_rows", "period_32768_zlib", "period_32768_far_matches", "crossing_run", "constant", "noise_640x480",
            "idat_of_1_byte_each", "idat_zero_length", "pillow_64k_split", "ancillary_before_and_after"]
    want += [f"filter{ft}_every_row_{fmt}" for ft in range(5) for fmt in ("RGB8", "RGBA8", "L16g", "L8g")] + [f"filter{ft}_on_row0_RGBA8" for ft in (2, 3, 4)]
    want += [f"pillow_{v}_{fmt}" for v in ("level0", "level1", "level6", "level9", "optimize") for fmt in P.FORMATS]
    assert not [n for n in want if n not in names]
    by = {n: d for n, _, d in P.corpus()}
    assert png.probe(by["big_256x300_L16g"])["inflated_bytes"] == 300 * 513 > 4 * 32768
    assert png.probe(by["idat_of_1_byte_each"])["n_idat"] == png.probe(by["idat_of_1_byte_each"])["idat_bytes"] > 20
    assert png.probe(by["idat_zero_length"])["n_idat"] == 6 and png.probe(by["pillow_64k_split"])["n_idat"] > 1
    assert zlib.decompress(P.idat_stream(by["wbits9"])) and P.idat_stream(by["wbits9"])[0] >> 4 == 1
    assert max(png.probe(d)["width"] for d in by.values()) == 640 and max(png.probe(d)["height"] for d in by.values()) == 480


# ---------------------------------------------------------------------------------------------------------------------------------
# 2 / 3: the parser
# ---------------------------------------------------------------------------------------------------------------------------------
def test_parser_agrees_with_pillow():
    import PIL.Image
    for name, kind, data in P.corpus():
        im = PIL.Image.open(io.BytesIO(data))
        info = png.probe(data)
        assert info is not None, (name, png.refusal(data))
        assert (info["width"], info["height"]) == im.size and info["mode"] == im.mode, name
        assert info["inflated_bytes"] == info["height"] * (1 + info["rowbytes"]) == len(P.references()[name][0]), name
        assert info["idat_bytes"] == len(P.idat_stream(data)) and png.refusal(data) is None, name


def _refused(data, *words):
    assert png.probe(data) is None
    reason = png.refusal(data)
    assert isinstance(reason, str) and reason, "a refusal without a reason"
    assert not words or any(w in reason for w in words), reason
    return reason


def _chunks(data):
    """(offset, type, payload length) of every chunk"""
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        out.append((pos, kind, n))
        pos += 12 + n
    return out


def _raw_png(w, h, depth, ct, interlace=0, extra=()):
    bits = depth * {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ct]
    raw = (b"\x00" + bytes((w * bits + 7) // 8)) * h
    return P.SIG + P.ihdr(w, h, depth, ct, interlace) + b"".join(P.chunk(k, p) for k, p in extra) + P.chunk(b"IDAT", zlib.compress(raw)) + P.chunk(b"IEND", b"")


def test_parser_refusals():
    import PIL.Image
    px = P.synthetic(40, 30, 3, "RGB8")
    good = P.write_png(px, filters=4, idat=[100], before=[(b"gAMA", struct.pack(">I", 45455))], after=[(b"tEXt", b"k\x00v")])
    assert png.probe(good)["n_idat"] == 2
    # formats the decoder leaves to Pillow; each is a file Pillow opens
    too_big = P.SIG + P.ihdr(1 << 15, 1 << 14, 8, 0) + P.chunk(b"IDAT", zlib.compress(b"\x00")) + P.chunk(b"IEND", b"")     # 2^29 + 2^14 inflated bytes
    for data, words in ((_raw_png(8, 8, 8, 2, interlace=1), ("Adam7",)), (_raw_png(8, 8, 8, 3, extra=[(b"PLTE", bytes(768))]), ("palette",)),
                        (_raw_png(8, 8, 1, 0), ("bit depth 1",)), (_raw_png(8, 8, 2, 0), ("bit depth 2",)), (_raw_png(8, 8, 4, 0), ("bit depth 4",)),
                        (_raw_png(8, 8, 8, 4), ("grey + alpha",)), (_raw_png(8, 8, 16, 2), ("16-bit RGB",)), (_raw_png(8, 8, 16, 6), ("16-bit RGBA",)),
                        (_raw_png(8, 8, 8, 0, extra=[(b"tRNS", b"\x00\x05")]), ("tRNS",)), (_raw_png(8, 8, 8, 2, extra=[(b"acTL", struct.pack(">II", 1, 0))]), ("acTL",)),
                        (_raw_png(0, 8, 8, 2), ("empty",)), (_raw_png(8, 0, 8, 2), ("empty",)), (too_big, ("inflated bytes",))):
        _refused(data, *words)
    for ok in (_raw_png(8, 8, 8, 2), _raw_png(8, 8, 16, 0), _raw_png(8, 8, 8, 2, extra=[(b"PLTE", bytes(48))])):
        assert png.probe(ok) is not None and PIL.Image.open(io.BytesIO(ok)).size == (8, 8), png.refusal(ok)
    # not a PNG at all
    jpg = io.BytesIO()
    PIL.Image.fromarray(px).save(jpg, "JPEG")
    _refused(jpg.getvalue(), "signature")
    _refused(b"", "signature")
    _refused(P.SIG, "IHDR")
    # cut at every chunk boundary, 4 and 8 bytes into every chunk, in mid-IDAT
    for pos, kind, n in _chunks(good):
        for cut in (pos, pos + 4, pos + 8):
            _refused(good[:cut])
        if kind == b"IDAT":
            _refused(good[:pos + 8 + n // 2], "past the end")
    _refused(good[:-12], "IEND")
    # a length field pointing past the end, in every chunk
    for pos, kind, n in _chunks(good):
        _refused(good[:pos] + struct.pack(">I", len(good)) + good[pos + 4:], "past the end")
        _refused(good[:pos] + b"\xff\xff\xff\xf0" + good[pos + 4:], "past the end")
    # no IDAT; IDAT chunks that are not consecutive; an unknown critical chunk
    ch = _chunks(good)
    first = next(p for p, k, _ in ch if k == b"IDAT")
    iend = next(p for p, k, _ in ch if k == b"IEND")
    after = next(p for p, k, _ in ch if k == b"tEXt")
    _refused(good[:first] + good[after:], "no IDAT")
    _refused(good[:iend] + P.chunk(b"IDAT", b"\x00") + good[iend:], "consecutive")
    _refused(good[:first] + P.chunk(b"ABCD", b"") + good[first:], "critical")
    # the zlib header, in each of the four ways
    z = P.idat_stream(good)

    def with_header(b0, b1):
        return P.write_png(px, stream=bytes([b0, b1]) + z[2:])

    assert png.probe(with_header(z[0], z[1])) is not None
    assert all((b0 << 8 | b1) % 31 == 0 for b0, b1 in ((0x79, 0x18), (0x88, 0x1C), (0x78, 0xBB)))      # the check bits hold: the named field alone is wrong
    _refused(with_header(0x79, 0x18), "CM")
    _refused(with_header(0x88, 0x1C), "CINFO")
    _refused(with_header(0x78, 0xBB), "FDICT")
    _refused(with_header(0x78, 0x9D), "FCHECK")
    _refused(P.write_png(px, stream=z[:5]), "shorter")


def test_parser_handles_arbitrary_bytes_without_exceptions():
    rng = np.random.default_rng(3)
    good = P.write_png(P.synthetic(33, 17, 2, "RGBA8"), filters=(4, 1), idat=40, before=[(b"pHYs", struct.pack(">IIB", 1, 1, 0))])
    parsed = 0
    for k in range(300):
        b = bytearray(good)
        for _ in range(1 + k % 5):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        info = png.probe(bytes(b))
        assert info is not None or png.refusal(bytes(b))
        parsed += info is not None
    assert 0 < parsed < 300


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: the stand-alone program under the host sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def png_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("png_check") / "png_check"
    # the sanitizer runtimes linked into the program itself (clang's default; gcc needs the flags): it runs as it is, with nothing to preload
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    os.path.join(ROOT, "tests", "c", "png_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_ctypes_layout_is_the_headers(png_check):
    out = _run(png_check, ["--sizes"])
    want = f"sizes: info {C.sizeof(_lib.PngInfo)} range {C.sizeof(_lib.PngRange)} image {C.sizeof(_lib.PngImage)} batch {C.sizeof(_lib.PngBatch)}"
    assert want in out, (want, out)


def test_sanitized_program_over_the_corpus(png_check, tmp_path):
    args = []
    for name, kind, data in P.corpus():
        inflated, pixels = P.references()[name]
        fmt = _lib.PNG_OUT_RGB8 if kind == "rgb" else _lib.PNG_OUT_GRAY8 if pixels.dtype == np.uint8 else _lib.PNG_OUT_GRAY16
        path = str(tmp_path / f"{name}.png")
        for suffix, content in (("", data), (".inflated", inflated), (".pixels", np.ascontiguousarray(pixels).astype(pixels.dtype.newbyteorder("<")).tobytes())):
            with open(path + suffix, "wb") as f:
                f.write(content)
        args.append(f"{fmt}:{path}")
    out = _run(png_check, args)
    lines = out.strip().splitlines()
    print(lines[-2])
    assert lines[-1] == f"png_check: OK {len(args)} files, {6 * len(args)} damaged variants", lines[-1]
    assert out.count("inflated equal, adler equal, pixels equal") == len(args)
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[-2])}
    # every rare case is in the corpus: a decoder that gets one of them wrong cannot pass it
    for key in ("stored", "fixed", "dynamic", "matches", "overlapping", "run16", "run17", "run18", "run_crossing", "filter0", "filter1", "filter2", "filter3",
                "filter4", "paeth_tie_a", "paeth_tie_b", "paeth_tie_c", "average_carry"):
        assert stats[key] > 0, (key, stats)
    assert stats["max_distance"] == 32768 and stats["max_length"] == 258, stats
    assert stats["damaged_intact"] == 0, stats        # no damaged variant passes the Adler-32 check


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: load_images
# ---------------------------------------------------------------------------------------------------------------------------------
def test_load_images_png_argument_is_checked_before_the_device():
    from must3r_amd import image
    import inspect
    sig = inspect.signature(image.load_images).parameters
    assert sig["png"].default == "pil" and sig["decode"].default == "pil"
    with pytest.raises(ValueError):
        image.load_images([], 512, decode="gpu", png="cpu")
    with pytest.raises(ValueError):
        image.load_images([], 512, decode="pil", png="gpu")
    with pytest.raises(ValueError):
        image.load_images([], 512, png="gpu")
