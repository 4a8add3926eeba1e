"""The yardstick of the JPEG decoder (must3r_amd/csrc/jpeg*.h*, must3r_amd.jpeg): the whole baseline decode restated in numpy -- marker segments, sequential
Huffman decoding, DC prediction, dequantisation, the accurate integer IDCT (13-bit constants, two passes), fancy upsampling of 2x1 / 2x2 chroma and the
16-bit YCbCr -> RGB -- held bit-equal to ``numpy.asarray(PIL.Image.open(f).convert("RGB"))`` by tests/test_jpeg_host.py, and the corpus every JPEG test
decodes: seeded synthetic images (a smooth field plus noise) encoded by Pillow's encoder inside the tests; no JPEG file is committed.

``decode(data, defect=None)``: ``defect`` plants one wrong step ("idct_truncate": the IDCT descales without its rounding term; "nearest_chroma": chroma is
replicated, not interpolated; "color_round": the colour step's rounding term is off by one bit, 2^14 for 2^15 -- a term off by one UNIT changes none of the
256 values a chroma byte can take, so no image could show it) -- each must break the equality with Pillow.
"""
import io

import numpy as np

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
                    50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
SIZES = [(w, h) for h in (1, 7, 8, 9, 16, 17, 33) for w in (1, 7, 8, 9, 16, 17, 33)] + [(48, 64)]
SAMPLINGS = ("444", "422", "420", "grey")
QUALITIES = (30, 75, 95, 100)
RESTARTS = (None, "blocks", "rows")


# ---------------------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------------------
def synthetic(w, h, seed, noise=24.0, grey=False):
    """a smooth field plus noise, uint8 [h, w, 3] (or [h, w])"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = []
    for c in range(1 if grey else 3):
        a, b, p = rng.uniform(0.02, 0.3, 3)
        f = 128 + 70 * np.sin(a * x + p * 5) * np.cos(b * y + c) + 30 * np.sin(0.05 * (x + y) + c)
        ch.append(f + rng.normal(0, noise, (h, w)))
    img = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    return img[..., 0] if grey else img


def encode(img, sampling="420", quality=90, optimize=False, restart=None, **extra):
    import PIL.Image
    kw = dict(quality=quality, optimize=optimize, **extra)
    if img.ndim == 3:
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[sampling]
    if restart == "blocks":
        kw["restart_marker_blocks"] = 1
    elif restart == "rows":
        kw["restart_marker_rows"] = 1
    buf = io.BytesIO()
    PIL.Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_rgb(data):
    import PIL.Image
    return np.asarray(PIL.Image.open(io.BytesIO(data)).convert("RGB"))


def corpus_cases():
    """(name, kwargs of encode, (w, h)): every size with every sampling; quality, optimize and restart rotate so that each value meets each sampling and many
    sizes (200 files)"""
    cases = []
    for i, (w, h) in enumerate(SIZES):
        for s, sampling in enumerate(SAMPLINGS):
            q = QUALITIES[(i + s) % 4]
            opt = bool((i // 4 + s) % 2)
            rst = RESTARTS[(i + 2 * s) % 3]
            cases.append((f"{w}x{h}_{sampling}_q{q}_{'opt' if opt else 'std'}_{rst or 'norst'}", dict(sampling=sampling, quality=q, optimize=opt, restart=rst), (w, h)))
    return cases


_corpus = None


def corpus():
    """[(name, jpeg bytes)], built once per process"""
    global _corpus
    if _corpus is None:
        _corpus = []
        for i, (name, kw, (w, h)) in enumerate(corpus_cases()):
            img = synthetic(w, h, 1000 + i, grey=kw["sampling"] == "grey")
            _corpus.append((name, encode(img, **kw)))
    return _corpus


# ---------------------------------------------------------------------------------------------------------------------------------
# marker segments
# ---------------------------------------------------------------------------------------------------------------------------------
class Unsupported(Exception):
    pass


def parse(data):
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    pos, qt, huff, ri, frame, scan = 2, {}, {}, 0, None, None
    while True:
        if pos + 4 > len(d) or d[pos] != 0xFF:
            raise Unsupported("cut")
        m = d[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        L = (d[pos + 2] << 8) | d[pos + 3]
        s = d[pos + 4:pos + 2 + L]
        if m in (0xC0, 0xC1):
            frame = dict(H=(s[1] << 8) | s[2], W=(s[3] << 8) | s[4], comps=[(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])])
        elif m == 0xC4:
            q = 0
            while q < len(s):
                counts = list(s[q + 1:q + 17])
                n = sum(counts)
                huff[(s[q] >> 4, s[q] & 15)] = (counts, list(s[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDB:
            q = 0
            while q < len(s):
                qt[s[q] & 15] = np.array(list(s[q + 1:q + 65]), dtype=np.int64)
                q += 65
        elif m == 0xDD:
            ri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            scan = [(s[1 + 2 * c], s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]
            pos += 2 + L
            break
        elif m in (0xC2, 0xC3, 0xC9, 0xCA, 0xCB):
            raise Unsupported("not baseline")
        pos += 2 + L
    return dict(frame=frame, qt=qt, huff=huff, ri=ri, scan=scan, ecs=pos)


def _codes(counts, vals):
    """{(length, code): symbol} of the canonical code"""
    table, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            table[(l, code)] = vals[p]
            code += 1
            p += 1
        code <<= 1
    return table


def entropy(data):
    """-> (header dict, int16 [blocks, 64] in row-major order with the DC DIFFERENCE at [0], geometry dict): sequential decoding, one segment after another"""
    hd = parse(data)
    d = bytes(data)
    fr = hd["frame"]
    nc = len(fr["comps"])
    hs, vs = (1, 1) if nc == 1 else (fr["comps"][0][1], fr["comps"][0][2])
    mx, my = -(-fr["W"] // (8 * hs)), -(-fr["H"] // (8 * vs))
    ny = hs * vs
    bpm = 1 if nc == 1 else ny + 2
    slots = [0] * ny + ([1, 2] if nc == 3 else [])
    tabs = {k: _codes(*v) for k, v in hd["huff"].items()}
    # segments: split at RSTn, un-stuff
    segs, cur, i = [], bytearray(), hd["ecs"]
    while True:
        b = d[i]
        if b == 0xFF:
            nx = d[i + 1]
            if nx == 0:
                cur.append(0xFF)
                i += 2
                continue
            if 0xD0 <= nx <= 0xD7:
                segs.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
            if nx == 0xFF:
                i += 1
                continue
            segs.append(bytes(cur))
            break
        cur.append(b)
        i += 1
    mcus = mx * my
    ri = hd["ri"] or mcus
    coef = np.zeros((mcus * bpm, 64), dtype=np.int16)
    blk = 0
    for sidx, seg in enumerate(segs):
        bits = "".join(f"{b:08b}" for b in seg) + "0" * 64
        p = 0
        for _ in range(min(ri, mcus - sidx * ri)):
            for slot in range(bpm):
                c = slots[slot]
                _, td, ta = hd["scan"][c]
                k = 0
                while k < 64:
                    t = tabs[(0, td)] if k == 0 else tabs[(1, ta)]
                    l = 1
                    while (l, int(bits[p:p + l], 2)) not in t:
                        l += 1
                        assert l <= 16
                    sym = t[(l, int(bits[p:p + l], 2))]
                    p += l
                    size = sym & 15
                    v = 0
                    if size:
                        v = int(bits[p:p + size], 2)
                        p += size
                        if v < (1 << (size - 1)):
                            v -= (1 << size) - 1
                    if k == 0:
                        coef[blk, 0] = v
                        k = 1
                    elif size == 0:
                        if sym >> 4 == 15:
                            k += 16
                        else:
                            break
                    else:
                        k += sym >> 4
                        coef[blk, NATURAL[k]] = v
                        k += 1
                blk += 1
    return hd, coef, dict(hs=hs, vs=vs, mx=mx, my=my, ny=ny, bpm=bpm, slots=slots, ri=ri, nc=nc)


# ---------------------------------------------------------------------------------------------------------------------------------
# pixels
# ---------------------------------------------------------------------------------------------------------------------------------
def _idct8(x, axis, shift, truncate):
    """jidctint.c's 8-point pass along ``axis`` of int64 [..., 8, 8]"""
    x = np.moveaxis(x, axis, -1)
    i = [x[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    rnd = 0 if truncate else 1 << (shift - 1)
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    out = np.stack([(o + rnd) >> shift for o in out], -1)
    return np.moveaxis(out, -1, axis)


def planes(data, defect=None):
    """-> (header, geometry, [uint8 plane per component, padded to whole MCUs])"""
    hd, coef, g = entropy(data)
    coef = coef.astype(np.int64).reshape(g["mx"] * g["my"], g["bpm"], 64)
    # DC prediction per component, reset at every restart interval
    for c in range(g["nc"]):
        sl = [s for s in range(g["bpm"]) if g["slots"][s] == c]
        dc = coef[:, sl, 0].reshape(-1)
        per = len(sl) * g["ri"]
        for a in range(0, dc.size, per):
            dc[a:a + per] = np.cumsum(dc[a:a + per])
        coef[:, sl, 0] = dc.reshape(-1, len(sl))
    out = []
    for c in range(g["nc"]):
        sl = [s for s in range(g["bpm"]) if g["slots"][s] == c]
        q = np.zeros(64, dtype=np.int64)
        q[NATURAL] = hd["qt"][hd["frame"]["comps"][c][3]]
        blocks = (coef[:, sl, :] * q).reshape(g["my"], g["mx"], len(sl), 8, 8)
        ws = _idct8(blocks, -2, 11, defect == "idct_truncate")      # columns
        px = _idct8(ws, -1, 18, defect == "idct_truncate")          # rows
        px = np.clip(px + 128, 0, 255).astype(np.uint8)
        h, v = (g["hs"], g["vs"]) if c == 0 else (1, 1)
        px = px.reshape(g["my"], g["mx"], v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(g["my"] * v * 8, g["mx"] * h * 8)
        out.append(px)
    return hd, g, out


def _upsample(p, mode, W, H, nearest):
    """jdsample.c: chroma plane -> int64 [H, W]"""
    if mode == "444":
        return p[:H, :W].astype(np.int64)
    dw = (W + 1) // 2
    if mode == "422":
        rows = p[:H, :dw].astype(np.int64)
    else:
        dh = (H + 1) // 2
        rows = p[:dh, :dw].astype(np.int64)
    if nearest or dw <= 2:
        up = np.repeat(rows, 2, axis=1)
        if mode == "420":
            up = np.repeat(up, 2, axis=0)
        return up[:H, :W]
    if mode == "422":
        left = np.concatenate([rows[:, :1], rows[:, :-1]], 1)
        right = np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
        even, odd = (3 * rows + left + 1) >> 2, (3 * rows + right + 2) >> 2
        even[:, 0], odd[:, -1] = rows[:, 0], rows[:, -1]
        up = np.stack([even, odd], -1).reshape(rows.shape[0], -1)
        return up[:H, :W]
    above = np.concatenate([rows[:1], rows[:-1]], 0)
    below = np.concatenate([rows[1:], rows[-1:]], 0)
    res = []
    for other in (above, below):
        cs = 3 * rows + other
        left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        even, odd = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        res.append(np.stack([even, odd], -1).reshape(rows.shape[0], -1))
    up = np.stack(res, 1).reshape(2 * rows.shape[0], -1)
    return up[:H, :W]


def decode(data, defect=None):
    """-> uint8 [H, W, 3], what Pillow's open().convert("RGB") gives"""
    hd, g, pl = planes(data, defect)
    W, H = hd["frame"]["W"], hd["frame"]["H"]
    y = pl[0][:H, :W].astype(np.int64)
    if g["nc"] == 1:
        return np.stack([y, y, y], -1).astype(np.uint8)
    mode = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[(g["hs"], g["vs"])]
    cb = _upsample(pl[1], mode, W, H, defect == "nearest_chroma") - 128
    cr = _upsample(pl[2], mode, W, H, defect == "nearest_chroma") - 128
    half = 1 << (14 if defect == "color_round" else 15)
    r = y + ((91881 * cr + half) >> 16)
    gch = y + ((-22554 * cb - 46802 * cr + half) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.clip(np.stack([r, gch, b], -1), 0, 255).astype(np.uint8)
