"""A small PNG writer and the corpus of the PNG decoder's tests (tests/test_png_host.py, tests/test_png_gpu.py).

The writer is built from ``struct``, ``zlib.crc32`` and ``zlib.compressobj`` and can force the filter type of every row, the deflate strategy and level,
``wbits``, flush points and the IDAT split.  Three streams no encoder writes are assembled by hand from RFC 1951's tables (``DeflateWriter``): stored blocks of
length 0 and 65535, matches at distance 32768 (zlib stops at 32506), and a dynamic header whose zero run crosses from the literal/length lengths into the
distance lengths (zlib codes the two sets apart).  The yardsticks stay ``zlib.decompress`` and Pillow: every file here is one both of them read.

A case is ``(name, kind, data)``; kind "rgb" goes through ``png.decode_images``, kind "gray" through ``png.decode_gray``.
"""
import functools
import io
import struct
import zlib

import numpy as np

FORMATS = ("L8", "RGB8", "RGBA8", "L8g", "L16g")          # the last two through decode_gray
KIND = {"L8": "rgb", "RGB8": "rgb", "RGBA8": "rgb", "L8g": "gray", "L16g": "gray"}
WIDTHS, HEIGHTS = (1, 2, 3, 7, 8, 9, 63, 64, 65), (1, 2, 63, 64, 65, 130)
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def ihdr(w, h, depth, color_type, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace))


def synthetic(w, h, seed, fmt):
    """a smooth surface plus noise in the low bits: matches, literals and every filter have work to do"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = {"L8": 1, "L8g": 1, "L16g": 1, "RGB8": 3, "RGBA8": 4}[fmt]
    if fmt == "L16g":
        return (1000 + 37 * xx + 91 * yy + rng.integers(0, 8, (h, w))).astype(np.uint16)
    img = np.stack([(3 * xx + 5 * yy * (c + 1) + 40 * c + rng.integers(0, 4, (h, w))) & 255 for c in range(ch)], -1).astype(np.uint8)
    return img[..., 0] if ch == 1 else img


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def scanlines(pixels, filters):
    """pixels (HxW or HxWxC, uint8 or uint16) -> the filtered scanlines, one filter-type byte in front of each; ``filters``: an int, or a sequence that
    rotates over the rows"""
    px = np.asarray(pixels)
    h = px.shape[0]
    bpp = (px.shape[2] if px.ndim == 3 else 1) * px.dtype.itemsize
    raw = (px.astype(">u2") if px.dtype == np.uint16 else px).reshape(h, -1).view(np.uint8).astype(np.int32)
    seq = [filters] if isinstance(filters, int) else list(filters)
    out = bytearray()
    for r in range(h):
        ft = seq[r % len(seq)]
        x = raw[r]
        b = raw[r - 1] if r else np.zeros_like(x)
        a, c = (np.concatenate([np.zeros(bpp, np.int32), v])[:v.size] for v in (x, b))   # bpp bytes to the left
        pred = [np.zeros_like(x), a, b, (a + b) >> 1, _paeth(a, b, c)][ft]
        out.append(ft)
        out += ((x - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_every=0, flush_mode=zlib.Z_FULL_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if not flush_every:
        return co.compress(raw) + co.flush()
    out = b""
    for a in range(0, len(raw), flush_every):
        out += co.compress(raw[a:a + flush_every]) + co.flush(flush_mode)
    return out + co.flush()


def write_png(pixels, filters=0, stream=None, idat=None, before=(), after=(), **deflate_args):
    """pixels -> the bytes of a PNG file.  ``stream``: the zlib stream to store in place of ``deflate(scanlines(...))``; ``idat``: None for one IDAT chunk, an
    int for chunks of that many bytes, or a list of chunk lengths (zeros allowed; the rest goes into a last chunk); ``before`` / ``after``: (type, payload) of
    ancillary chunks around the IDAT chunks"""
    px = np.asarray(pixels)
    h, w = px.shape[:2]
    ct = {1: 0, 3: 2, 4: 6}[px.shape[2] if px.ndim == 3 else 1]
    z = deflate(scanlines(px, filters), **deflate_args) if stream is None else stream
    if idat is None:
        parts = [z]
    elif isinstance(idat, int):
        parts = [z[a:a + idat] for a in range(0, len(z), idat)]
    else:
        parts, a = [], 0
        for n in idat:
            parts.append(z[a:a + n])
            a += n
        parts.append(z[a:])
    out = SIG + ihdr(w, h, 8 * px.dtype.itemsize, ct)
    out += b"".join(chunk(k, p) for k, p in before) + b"".join(chunk(b"IDAT", p) for p in parts) + b"".join(chunk(k, p) for k, p in after)
    return out + chunk(b"IEND", b"")


# ---------------------------------------------------------------------------------------------------------------------------------
# deflate by hand: RFC 1951's tables, for the streams no encoder writes
# ---------------------------------------------------------------------------------------------------------------------------------
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CODE_LENGTH_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical(lengths):
    """code lengths -> the canonical codes (RFC 1951 3.2.2)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = []
    for n in lengths:
        codes.append(nxt[n] if n else None)
        nxt[n] += 1 if n else 0
    return codes


class DeflateWriter:
    """bits LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        self.bits(int(format(code, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def stored(self, data, final):
        self.bits(final, 1)
        self.bits(0, 2)
        self.align()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data

    def tokens(self, toks, litlen, dist):
        """literals (ints) and matches ((length, distance)), then the end-of-block code"""
        lc, dc = canonical(litlen), canonical(dist)
        for t in toks:
            if isinstance(t, int):
                self.code(lc[t], litlen[t])
                continue
            length, d = t
            li = max(i for i, b in enumerate(LENGTH_BASE) if b <= length and (length < 258 or i == 28))
            self.code(lc[257 + li], litlen[257 + li])
            self.bits(length - LENGTH_BASE[li], LENGTH_EXTRA[li])
            di = max(i for i, b in enumerate(DIST_BASE) if b <= d)
            self.code(dc[di], dist[di])
            self.bits(d - DIST_BASE[di], DIST_EXTRA[di])
        self.code(lc[256], litlen[256])

    def fixed(self, toks, final):
        self.bits(final, 1)
        self.bits(1, 2)
        self.tokens(toks, FIXED_LITLEN, FIXED_DIST)

    def dynamic(self, toks, litlen, dist, header, cl_lengths, final):
        """``header``: the (code-length symbol, extra value) sequence that spells litlen + dist; ``cl_lengths``: the 19 lengths of the code-length code"""
        self.bits(final, 1)
        self.bits(2, 2)
        ncode = max(i for i, s in enumerate(CODE_LENGTH_ORDER) if cl_lengths[s]) + 1
        self.bits(len(litlen) - 257, 5)
        self.bits(len(dist) - 1, 5)
        self.bits(max(ncode, 4) - 4, 4)
        for s in CODE_LENGTH_ORDER[:max(ncode, 4)]:
            self.bits(cl_lengths[s], 3)
        cc = canonical(cl_lengths)
        for s, extra in header:
            self.code(cc[s], cl_lengths[s])
            if s >= 16:
                self.bits(extra, {16: 2, 17: 3, 18: 7}[s])
        self.tokens(toks, litlen, dist)

    def zlib_stream(self, raw):
        self.align()
        return b"\x78\x01" + bytes(self.out) + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


def stored_stream(raw, sizes):
    """raw as stored blocks of the given sizes (the rest in blocks of up to 65535 bytes)"""
    w, a = DeflateWriter(), 0
    sizes = list(sizes)
    while a < len(raw) or sizes:
        n = sizes.pop(0) if sizes else min(65535, len(raw) - a)
        w.stored(raw[a:a + n], int(a + n >= len(raw) and not sizes))
        a += n
    return w.zlib_stream(raw)


def far_match_stream(raw):
    """raw, whose bytes repeat with period 32768: the first 32768 as literals of a fixed block, the rest as matches at distance 32768, of length 258 while it fits"""
    assert raw[32768:] == raw[:len(raw) - 32768]
    toks, a = list(raw[:32768]), 32768
    while a < len(raw):
        n = min(258, len(raw) - a)
        if 0 < len(raw) - a - n < 3:      # leave a last match of three bytes at least
            n -= 3
        toks.append((n, 32768))
        a += n
    w = DeflateWriter()
    w.fixed(toks, 1)
    return w.zlib_stream(raw)


def crossing_run_stream(raw):
    """raw in one dynamic block whose header codes the zero lengths of literal/length symbols 258, 259 and of distance codes 0, 1 as ONE run of code 17: the run
    crosses the boundary between the two sets.  Literals 0 ... 253 take 8 bits, 254, 255, 256 and length symbol 257 take 9; distance codes 2 and 3 (distances 3
    and 4) take 1 bit.  The data is coded as literals, and as matches of length 3 where the bytes three or four back repeat."""
    litlen = [8] * 254 + [9] * 4 + [0, 0]
    dist = [0, 0, 1, 1]
    header = [(8, 0)] + [(16, 3)] * 42 + [(8, 0)] + [(9, 0)] * 4 + [(17, 1)] + [(1, 0)] * 2     # 1 + 42 * 6 + 1 = 254 eights; 17 with extra 1: a run of 4
    cl = [0] * 19
    cl[1], cl[8], cl[9], cl[16], cl[17] = 3, 2, 2, 2, 3
    toks, a = [], 0
    while a < len(raw):
        d = next((d for d in (3, 4) if a >= d and raw[a:a + 3] == raw[a - d:a - d + 3] and a + 3 <= len(raw)), None)
        if d:
            toks.append((3, d))
            a += 3
        else:
            toks.append(raw[a])
            a += 1
    w = DeflateWriter()
    w.dynamic(toks, litlen, dist, header, cl, 1)
    return w.zlib_stream(raw)


def period_image():
    """255 x 260 grey, stride 256: the rows repeat every 128, so the scanlines (filter type 0) repeat with period 32768 bytes"""
    rows = np.random.default_rng(11).integers(0, 256, (128, 255), dtype=np.uint8)
    return np.concatenate([rows, rows, rows[:4]], 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------------------
def pillow_png(pixels, **save_args):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(np.asarray(pixels)).save(buf, "PNG", **save_args)
    return buf.getvalue()


def size_cases():
    """(name, fmt, w, h): every width by every height, the formats rotating"""
    return [(f"size_{w}x{h}_{FORMATS[(i * len(HEIGHTS) + j) % 5]}", FORMATS[(i * len(HEIGHTS) + j) % 5], w, h) for i, w in enumerate(WIDTHS) for j, h in enumerate(HEIGHTS)]


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, kind, data)]"""
    out = []

    def add(name, fmt, data):
        out.append((name, KIND[fmt], data))

    for k, (name, fmt, w, h) in enumerate(size_cases()):
        add(name, fmt, write_png(synthetic(w, h, k, fmt), filters=(0, 1, 2, 3, 4) if k % 2 else (4, 3, 2, 1, 0)))
    add("big_256x300_L16g", "L16g", write_png(synthetic(256, 300, 100, "L16g"), filters=(1, 4, 2, 3, 0)))
    # filters
    for ft in range(5):
        for fmt in ("RGB8", "RGBA8", "L16g", "L8g"):
            add(f"filter{ft}_every_row_{fmt}", fmt, write_png(synthetic(65, 66, 110 + ft, fmt), filters=ft))
    add("filters_rotating_RGB8", "RGB8", write_png(synthetic(64, 65, 120, "RGB8"), filters=(0, 1, 2, 3, 4)))
    for ft in (2, 3, 4):
        add(f"filter{ft}_on_row0_RGBA8", "RGBA8", write_png(synthetic(9, 3, 130 + ft, "RGBA8"), filters=(ft, 0, 1)))
    # deflate
    img = synthetic(200, 150, 140, "RGB8")
    add("level0_stored_only", "RGB8", write_png(img, filters=1, level=0))
    big = synthetic(256, 300, 141, "L16g")
    raw = scanlines(big, 1)
    add("stored_0_and_65535", "L16g", write_png(big, stream=stored_stream(raw, [0, 65535, 0, 0, 65535, 7])))
    add("z_fixed", "RGB8", write_png(img, filters=4, strategy=zlib.Z_FIXED))
    add("z_huffman_only", "RGB8", write_png(img, filters=4, strategy=zlib.Z_HUFFMAN_ONLY))
    add("z_rle", "RGB8", write_png(img, filters=1, strategy=zlib.Z_RLE))
    for level in (1, 6, 9):
        add(f"level{level}", "RGBA8", write_png(synthetic(200, 150, 142, "RGBA8"), filters=(4, 3, 1), level=level))
    add("wbits9", "RGB8", write_png(img, filters=2, wbits=9))
    add("full_flush_every_3_rows", "RGB8", write_png(img, filters=3, flush_every=3 * (1 + 600)))
    per = period_image()
    add("period_32768_zlib", "L8g", write_png(per, filters=0, level=9))
    add("period_32768_far_matches", "L8g", write_png(per, stream=far_match_stream(scanlines(per, 0))))
    small = synthetic(40, 30, 143, "L8")
    add("crossing_run", "L8", write_png(small, stream=crossing_run_stream(scanlines(small, 1))))
    add("constant", "RGB8", write_png(np.full((120, 160, 3), 77, np.uint8), filters=0))
    add("noise_640x480", "RGB8", write_png(np.random.default_rng(5).integers(0, 256, (480, 640, 3), dtype=np.uint8), filters=0))
    # chunks
    tiny = synthetic(9, 7, 150, "RGB8")
    add("idat_of_1_byte_each", "RGB8", write_png(tiny, filters=4, idat=1))
    add("idat_zero_length", "RGB8", write_png(img, filters=1, idat=[0, 5, 0, 1, 0]))
    add("pillow_64k_split", "RGB8", pillow_png(np.random.default_rng(6).integers(0, 256, (300, 400, 3), dtype=np.uint8)))
    anc = [(b"gAMA", struct.pack(">I", 45455)), (b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), (b"tEXt", b"Comment\x00the corpus of the PNG decoder")]
    add("ancillary_before_and_after", "RGBA8", write_png(synthetic(33, 17, 151, "RGBA8"), filters=4, before=anc, after=[(b"tEXt", b"After\x00the data")]))
    # Pillow's own encoder
    for fmt in ("L8", "L8g", "L16g", "RGB8", "RGBA8"):
        px = synthetic(65, 40, 160, fmt)
        for level in (0, 1, 6, 9):
            add(f"pillow_level{level}_{fmt}", fmt, pillow_png(px, compress_level=level))
        add(f"pillow_optimize_{fmt}", fmt, pillow_png(px, optimize=True))
    assert len({n for n, _, _ in out}) == len(out)
    return tuple(out)


def idat_stream(data):
    """the zlib stream of a file: its IDAT payloads back to back"""
    pos, z = 8, b""
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            z += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return z


def pillow_pixels(data, kind):
    import PIL.Image
    im = PIL.Image.open(io.BytesIO(data))
    return np.asarray(im.convert("RGB")) if kind == "rgb" else np.asarray(im)


@functools.lru_cache(maxsize=None)
def references():
    """{name: (inflated bytes by zlib.decompress, pixels by Pillow)}; computed once, shared by the tests, never written to"""
    out = {}
    for name, kind, data in corpus():
        px = pillow_pixels(data, kind)
        px.setflags(write=False)
        out[name] = (zlib.decompress(idat_stream(data)), px)
    return out
