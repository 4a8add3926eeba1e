"""CPU: the numpy emulations of tests/augment_ref.py (the arithmetic csrc/train_augment.hip implements) against the Pillow calls they stand for, the geometry chain
of must3r_amd/train_augment.py against its restatement and against its own meaning, and the ABI surface of must3r_hip_augment_color / must3r_hip_augment_depth:
symbols, descriptor layouts, the table inversion, and that every refusal returns before anything is uploaded or launched (there is no GPU here to launch on)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

import augment_ref as AR
from conftest import ROOT
from must3r_amd import _lib, train_augment as TA

BLEND_FACTORS = (0, 0.5, 0.73, 0.9999, 1, 1.2345678, 1.5)


@pytest.fixture(scope="module")
def all_colours():
    """every 24-bit triple once, as a 4096 x 4096 x 3 image"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulations equal Pillow
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rgb_to_hsv_equals_pillow_on_all_colours(all_colours):
    pil = np.asarray(Image.fromarray(all_colours, "RGB").convert("HSV"))
    assert int((pil != AR.rgb_to_hsv_np(all_colours)).any(-1).sum()) == 0


def test_hsv_to_rgb_equals_pillow_on_all_triples(all_colours):
    pil = np.asarray(Image.fromarray(all_colours, "HSV").convert("RGB"))
    assert int((pil != AR.hsv_to_rgb_np(all_colours)).any(-1).sum()) == 0


def test_luma_equals_pillow_on_all_colours(all_colours):
    assert np.array_equal(np.asarray(Image.fromarray(all_colours, "RGB").convert("L")), AR.luma_np(all_colours))


@pytest.mark.parametrize("f", BLEND_FACTORS)
def test_blend_equals_pillow_on_all_byte_pairs(f):
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    b = np.ascontiguousarray(a.T)
    pil = np.asarray(Image.blend(Image.fromarray(a, "L"), Image.fromarray(b, "L"), f))
    assert np.array_equal(pil, AR.blend_np(a, b, f))


def test_contrast_mean_equals_pillow_at_the_rounding_boundary():
    below, above = AR.contrast_boundary_images()
    means = []
    for img in (below, above):
        L = AR.luma_np(img)
        assert np.array_equal(L, img[..., 0])
        m = AR.contrast_mean(L.astype(np.int64).sum(), L.size)
        means.append(m)
        for f in (0.5, 1.5):
            pil = np.asarray(ImageEnhance.Contrast(Image.fromarray(img, "RGB")).enhance(float(np.float32(f))))
            assert np.array_equal(pil, AR.apply_op_np(img, AR.CONTRAST, f))
            assert np.array_equal(pil, AR.blend_np(np.full_like(img, m), img, f))
    assert means == [100, 101]


def test_whole_jitter_emulation_equals_pillow():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    for trial in range(12):
        order = [int(i) for i in rng.permutation(4)]
        factors = [float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5)), float(rng.uniform(-0.1, 0.1))]
        flags = [int(b) for b in rng.integers(0, 2, size=4)] if trial % 2 else [1, 1, 1, 1]
        assert np.array_equal(AR.jitter_pil(img, order, factors, flags), AR.jitter_np(img, order, factors, flags)), (order, factors, flags)


def test_hue_shift_is_the_stated_one():
    assert [AR.hue_shift(f) for f in (0.0, 0.1, -0.1, 0.5, -0.5, 0.003, -0.003)] == [0, 25, 256 - 25, 127, 256 - 127, 0, 0]


def test_table_inversion_is_exact():
    """u = int(127.5f v + 127.5f + 0.5f), each operation rounded to fp32, gives u back for all 256 entries of the resampler's table"""
    assert AR.NORM_TABLE.dtype == np.float32 and np.array_equal(AR.invert_norm(AR.NORM_TABLE), np.arange(256))
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    assert np.array_equal(AR.img_norm_np(u8)[0, 0].view(np.uint32), AR.NORM_TABLE.view(np.uint32))
    assert np.array_equal(AR.NORM_TABLE, ((torch.arange(256).float() / 255 - 0.5) / 0.5).numpy())


# ---------------------------------------------------------------------------------------------------------------------------------
# the geometry chain
# ---------------------------------------------------------------------------------------------------------------------------------
def _K(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def _sweep():
    for (W, H) in ((131, 97), (97, 131), (120, 120), (52, 40), (640, 480), (1752, 1168), (1168, 1752), (100, 105)):
        for (dx, dy) in ((0.0, 0.0), (0.07, -0.04), (-0.11, 0.09), (0.2, 0.2)):
            for res in ((64, 48), (48, 48), (512, 384)):
                for aug_crop in (0, 1, 8):
                    for seed in (None, 0, 1):
                        yield W, H, _K(0.9 * max(W, H), W / 2 + dx * W, H / 2 + dy * H), res, aug_crop, seed


def test_geometry_equals_its_restatement_and_stays_inside():
    n = swapped = drawn = lanczos = 0
    for W, H, K, res, aug_crop, seed in _sweep():
        if aug_crop > 1 and seed is None:
            with pytest.raises(ValueError, match="rng"):
                TA.crop_resize_geometry(W, H, K, res, None, aug_crop)
            continue
        rngs = [None if seed is None else np.random.default_rng(seed) for _ in range(2)]
        g = TA.crop_resize_geometry(W, H, K, res, rngs[0], aug_crop)
        r = AR.geometry(W, H, K, res, rngs[1], aug_crop)
        assert g.crop1 == r.crop1 and g.size1 == r.size1 and g.resized == r.resized and g.window == r.window and g.out == r.out and g.scale == r.scale
        assert np.array_equal(g.K, r.K) and (g.mode == _lib.RESAMPLE_PIL_LANCZOS) == r.lanczos == (g.scale < 1)
        # the first crop: inside the frame, the principal point within half a pixel of its centre
        l1, t1, r1, b1 = g.crop1
        assert 0 <= l1 < r1 <= W and 0 <= t1 < b1 <= H and g.size1 == (r1 - l1, b1 - t1)
        assert abs(K[0, 2] - l1 - g.size1[0] / 2) <= 0.5 and abs(K[1, 2] - t1 - g.size1[1] / 2) <= 0.5
        # the window: the resolution, possibly swapped, inside the rescaled image
        l, t, rr, bb = g.window
        assert sorted(g.out) == sorted(res) and (rr - l, bb - t) == g.out and 0 <= l and 0 <= t and rr <= g.resized[0] and bb <= g.resized[1]
        if g.size1[1] > 1.1 * g.size1[0]:
            assert g.portrait or res[0] == res[1]
        near_square = 0.9 < g.size1[1] / g.size1[0] < 1.1
        if not near_square or seed is None:
            assert g.portrait == (g.size1[1] > 1.1 * g.size1[0] and res[0] != res[1])
        drawn += near_square and seed is not None and res[0] != res[1]
        swapped += g.portrait
        lanczos += g.mode == _lib.RESAMPLE_PIL_LANCZOS
        n += 1
    assert n > 500 and swapped > 50 and drawn > 20 and 0 < lanczos < n


def test_a_point_projects_through_the_chain_to_within_a_pixel():
    """a 3-D point projected with the source K lands at p; the chain -- first crop, rescale about pixel corners (a pixel's centre is at its index + 0.5), window
    -- maps p to (p + 0.5 - crop1) * scale - 0.5 - window; the returned K projects the same point there to within 1 px (the rescaled size is floored and the
    window's corner rounded: under half a pixel each)"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for W, H, K, res, aug_crop, seed in _sweep():
        if seed is None and aug_crop > 1:
            continue
        g = TA.crop_resize_geometry(W, H, K, res, None if seed is None else np.random.default_rng(seed), aug_crop)
        X = np.concatenate([rng.uniform(-0.3, 0.3, size=(16, 2)), rng.uniform(1.0, 4.0, size=(16, 1))], axis=1)
        p = (K @ X.T).T
        p = p[:, :2] / p[:, 2:]
        q = (g.K @ X.T).T
        q = q[:, :2] / q[:, 2:]
        chain = (p + 0.5 - np.array(g.crop1[:2])) * g.scale - 0.5 - np.array(g.window[:2])
        worst = max(worst, float(np.abs(q - chain).max()))
    print(f"projection through the chain against the returned K: worst difference {worst:.3f} px")
    assert worst <= 1.0


def test_geometry_refusals():
    with pytest.raises(ValueError, match="border"):
        TA.crop_resize_geometry(100, 80, _K(90, 15, 40), (64, 48))
    with pytest.raises(ValueError, match="border"):
        TA.crop_resize_geometry(100, 80, _K(90, 50, 70), (64, 48))
    with pytest.raises(ValueError, match="w >= h"):
        TA.crop_resize_geometry(100, 80, _K(90, 50, 40), (48, 64))
    with pytest.raises(ValueError, match="border"):
        AR.geometry(100, 80, _K(90, 15, 40), (64, 48))
    with pytest.raises(ValueError, match="stored shape"):
        TA.stored_shape([TA.crop_resize_geometry(131, 97, _K(100, 65, 48), (64, 48)), TA.crop_resize_geometry(97, 131, _K(100, 48, 65), (64, 48))], landscape=False)
    assert TA.stored_shape([TA.crop_resize_geometry(131, 97, _K(100, 65, 48), (64, 48)), TA.crop_resize_geometry(97, 131, _K(100, 48, 65), (64, 48))]) == (48, 64)


def test_depth_gather_of_the_yardstick_is_nearest_neighbour():
    g = AR.geometry(131, 97, _K(100, 70, 45), (64, 48))
    depth = np.arange(97 * 131, dtype=np.float32).reshape(97, 131)
    d = AR.depth_gather(depth, g)
    assert d.shape == (48, 64)
    ys, xs = np.divmod(d.astype(np.int64), 131)
    (l1, t1, r1, b1) = g.crop1
    assert xs.min() >= l1 and xs.max() < r1 and ys.min() >= t1 and ys.max() < b1
    assert (np.diff(xs, axis=1) >= 0).all() and (np.diff(ys, axis=0) >= 0).all() and (np.diff(xs, axis=0) == 0).all()
    # an identity geometry reads every pixel once
    ident = AR.geometry(64, 48, _K(60, 32, 24), (64, 48))
    assert ident.crop1 == (0, 0, 64, 48) and ident.window == (0, 0, 64, 48)
    full = np.arange(48 * 64, dtype=np.float32).reshape(48, 64)
    assert np.array_equal(AR.depth_gather(full, ident), full)


def test_jitter_params_draw_in_the_stated_order():
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    order, factors = TA.get_jitter_params(0.5, 0.5, 0.5, 0.1, generator=g1)
    assert order == torch.randperm(4, generator=g2).tolist()
    want = [float(torch.empty(1).uniform_(lo, hi, generator=g2)) for lo, hi in ((0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (-0.1, 0.1))]
    assert factors == want and all(0.5 <= f <= 1.5 for f in factors[:3]) and -0.1 <= factors[3] <= 0.1
    with pytest.raises(ValueError):
        TA.get_jitter_params(hue=0.6)


def test_synthetic_raw_scenes():
    ds = TA.SyntheticRawScenes(2, 4, [(97, 131), (131, 97), (120, 120), (40, 52)], seed=1)
    views = ds[1]
    assert len(ds) == 2 and [tuple(v["img"].shape) for v in views] == [(97, 131, 3), (131, 97, 3), (120, 120, 3), (40, 52, 3)]
    for v in views:
        H, W = v["depthmap"].shape
        assert v["img"].dtype == torch.uint8 and v["depthmap"].dtype == torch.float32 and v["img"].is_contiguous()
        K = v["camera_intrinsics"]
        assert abs(float(K[0, 2]) - W / 2) > 0.04 * W and abs(float(K[1, 2]) - H / 2) > 0.02 * H          # off-centre
        g = TA.crop_resize_geometry(W, H, K.numpy(), (64, 48))
        assert g.size1 != (W, H)
    assert bool((views[0]["depthmap"] < 0).any()) and bool((views[0]["depthmap"] == 0).any())
    raw = TA.SyntheticRawScenes(1, 2, [(40, 52)], raw_depth=True)[0][0]
    assert raw["depthmap"].dtype == torch.uint16 and raw["depth_scale"].tolist() == [1000.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the ABI surface
# ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        return f.read()


def _fields(h, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [re.sub(r"\[\d+\]", "", first.split()[-1].lstrip("*"))] + [r.strip() for r in rest]
    return fields


def test_abi_surface_of_the_augmentation():
    h = _header()
    assert _lib.ABI_VERSION == 21 and re.search(r"#define\s+MUST3R_HIP_ABI_VERSION\s+21\b", h)
    block = h[h.index("/* ABI 21, additive.  Training augmentation"):h.index("/* debug: lane -> element mapping")]
    for name, proto in (("must3r_hip_augment_color", (C.c_int, [C.POINTER(_lib.AugmentColorArgs)])),
                        ("must3r_hip_augment_depth", (C.c_int, [C.POINTER(_lib.AugmentDepthArgs)])),
                        ("must3r_hip_augment_color_scratch_bytes", (C.c_size_t, [C.c_int, C.c_int, C.c_int])),
                        ("must3r_hip_augment_depth_scratch_bytes", (C.c_size_t, [C.c_int]))):
        assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == proto
        fn = getattr(_lib.load(), name)
        assert fn.argtypes == proto[1] and fn.restype == proto[0]
        assert re.search(r"\b%s\s*\(" % name, block)
    for name in ("color", "depth"):
        assert re.search(r"\bint\s+must3r_hip_augment_%s\s*\(\s*const\s+must3r_hip_augment_%s_args\s*\*\s*a\s*\)\s*;" % (name, name), h)
    # no entry point of the block takes a trailing stream: the stream travels in the descriptors
    assert not re.search(r"void\*\s*stream\s*\)", block) and block.count("void* stream;") == 2
    for struct, cls in (("must3r_hip_augment_color_view", _lib.AugmentColorView), ("must3r_hip_augment_color_args", _lib.AugmentColorArgs),
                        ("must3r_hip_augment_depth_view", _lib.AugmentDepthView), ("must3r_hip_augment_depth_args", _lib.AugmentDepthArgs)):
        assert _fields(h, struct) == [n for n, _ in cls._fields_], struct
    V, A, D, DA = _lib.AugmentColorView, _lib.AugmentColorArgs, _lib.AugmentDepthView, _lib.AugmentDepthArgs
    assert C.sizeof(V) == 8 + 3 * 4 + 3 * 16 + 4 and (V.src_offset.offset, V.h.offset, V.portrait.offset, V.order.offset, V.apply.offset, V.factor.offset) \
        == (0, 8, 16, 20, 36, 52)
    assert C.sizeof(A) == 6 * 8 + 4 * 4 + 8 and (A.src_elems.offset, A.views.offset, A.out.offset, A.scratch_bytes.offset, A.V.offset, A.stream.offset) \
        == (8, 16, 24, 40, 48, 64)
    assert C.sizeof(D) == 16 + 14 * 4 and (D.row_stride.offset, D.H.offset, D.crop_x.offset, D.resize_w.offset, D.win_x.offset, D.portrait.offset) \
        == (8, 16, 24, 40, 48, 64)
    assert C.sizeof(DA) == 4 * 8 + 4 * 4 + 8 and (DA.out.offset, DA.scratch_bytes.offset, DA.V.offset, DA.depth_u16.offset, DA.stream.offset) == (8, 24, 32, 44, 48)
    assert int(re.search(r"#define\s+MUST3R_AUG_TILE\s+(\d+)", h).group(1)) == _lib.AUG_TILE
    assert re.search(r"MUST3R_AUG_BRIGHTNESS = 0, MUST3R_AUG_CONTRAST = 1, MUST3R_AUG_SATURATION = 2, MUST3R_AUG_HUE = 3", h)
    assert (_lib.AUG_BRIGHTNESS, _lib.AUG_CONTRAST, _lib.AUG_SATURATION, _lib.AUG_HUE) == (AR.BRIGHTNESS, AR.CONTRAST, AR.SATURATION, AR.HUE) == (0, 1, 2, 3)
    with open(os.path.join(ROOT, "must3r_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS\s*=.*\btrain_augment\.hip\b", mk, flags=re.M) and re.search(r"^build/train_augment\.o: FLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    with open(os.path.join(ROOT, "must3r_amd", "csrc", "train_augment.hip")) as f:
        src = f.read()
    assert 'extern "C" int must3r_hip_augment_color(' in src and 'extern "C" int must3r_hip_augment_depth(' in src and "atomicAdd" not in src


def _err(lib):
    return lib.must3r_hip_last_error().decode()


def _color_call():
    """a descriptor that would pass every check: host memory stands in for the device pointers, which a refused call never reads"""
    buf = (C.c_float * 8192)()
    base = (C.addressof(buf) + 255) & ~255
    tab = (_lib.AugmentColorView * 2)()
    for i, t in enumerate(tab):
        t.src_offset, t.h, t.w = i * 3 * 48, 4, 12
        t.order[:] = [3, 1, 0, 2]
        t.apply[:] = [1, 1, 1, 1]
        t.factor[:] = [1.2, 0.8, 1.1, 0.05]
    a = _lib.AugmentColorArgs()
    a.src, a.src_elems, a.views, a.out, a.scratch, a.scratch_bytes = base, 2 * 3 * 48, tab, base + 4096, base + 8192, 4096
    a.V, a.Hs, a.Ws = 2, 4, 12
    return a, tab, buf


def test_augment_color_refuses_before_touching_anything():
    lib = _lib.load()
    call = lib.must3r_hip_augment_color
    assert call(None) != 0 and "null" in _err(lib)
    assert lib.must3r_hip_augment_color_scratch_bytes(2, 4, 12) == 512 and lib.must3r_hip_augment_color_scratch_bytes(0, 4, 12) == 0
    big = lib.must3r_hip_augment_color_scratch_bytes(300, 384, 512)               # the table, and a uint32 per view and 64 x 64 tile for the contrast sums
    assert big % 256 == 0 and 300 * 6 * 8 * 4 < big < 300 * 6 * 8 * 4 + 300 * 128

    def refused(what, **change):
        a, tab, buf = _color_call()
        for k, v in change.items():
            if k.startswith("v_"):
                f = getattr(tab[1], k[2:])
                if hasattr(f, "__len__"):
                    f[:] = v
                else:
                    setattr(tab[1], k[2:], v)
            else:
                setattr(a, k, v)
        assert call(C.byref(a)) != 0 and what in _err(lib), (what, _err(lib))

    for field in ("src", "views", "out", "scratch"):
        refused("null", **{field: None})
    refused("V must be", V=0)
    refused("V must be", V=65536)
    refused("positive", Hs=0)
    refused("aligned", src=_color_call()[0].src + 2)
    refused("256-byte", scratch=_color_call()[0].scratch + 16)
    refused("scratch is smaller", scratch_bytes=511)
    refused("bad order", v_order=[0, 1, 2, 2])
    refused("bad order", v_order=[0, 1, 2, 4])
    refused("bad flags", v_apply=[0, 1, 2, 0])
    refused("bad flags", v_portrait=2)
    refused("finite", v_factor=[float("nan"), 1, 1, 0])
    refused("hue factor", v_factor=[1, 1, 1, 0.51])
    refused("mixed stored shape", v_h=12, v_w=4)                      # a portrait view that is not flagged
    refused("mixed stored shape", v_portrait=1)                       # a landscape view that is
    refused("mixed stored shape", v_w=8)
    refused("inside src", v_src_offset=2 * 3 * 48 - 3 * 48 + 1)
    refused("inside src", v_src_offset=-1)


def _depth_call():
    buf = (C.c_float * 4096)()
    base = (C.addressof(buf) + 255) & ~255
    tab = (_lib.AugmentDepthView * 2)()
    for t in tab:
        t.src, t.row_stride, t.H, t.W = base, 20, 10, 20
        t.crop_x, t.crop_y, t.crop_w, t.crop_h = 2, 1, 16, 8
        t.resize_w, t.resize_h = 14, 7
        t.win_x, t.win_y, t.out_w, t.out_h = 1, 1, 12, 4
    a = _lib.AugmentDepthArgs()
    a.views, a.out, a.scratch, a.scratch_bytes = tab, base + 2048, base + 4096, 256
    a.V, a.Hs, a.Ws = 2, 4, 12
    return a, tab, buf


def test_augment_depth_refuses_before_touching_anything():
    lib = _lib.load()
    call = lib.must3r_hip_augment_depth
    assert call(None) != 0 and "null" in _err(lib)
    assert lib.must3r_hip_augment_depth_scratch_bytes(2) == 256 and lib.must3r_hip_augment_depth_scratch_bytes(0) == 0

    def refused(what, **change):
        a, tab, buf = _depth_call()
        for k, v in change.items():
            setattr(tab[1] if k.startswith("v_") else a, k[2:] if k.startswith("v_") else k, v)
        assert call(C.byref(a)) != 0 and what in _err(lib), (what, _err(lib))

    for field in ("views", "out", "scratch", "v_src"):
        refused("null", **{field: None})
    refused("bad flags", depth_u16=2)
    refused("bad flags", v_portrait=-1)
    refused("V must be", V=-1)
    refused("aligned", out=_depth_call()[0].out + 2)
    refused("aligned", v_src=_depth_call()[0].out + 1, depth_u16=1)
    refused("scratch is smaller", scratch_bytes=255)
    refused("mixed stored shape", v_out_w=4, v_out_h=12)
    refused("mixed stored shape", Ws=16)
    refused("row stride", v_row_stride=19)
    refused("crop does not lie inside", v_crop_x=5)
    refused("crop does not lie inside", v_crop_y=-1)
    refused("resize must be positive", v_resize_w=0)
    refused("window does not lie inside", v_win_x=3)
    refused("window does not lie inside", v_win_y=-1)


def test_python_side_refuses_cpu_tensors_and_mixed_shapes():
    with pytest.raises(RuntimeError, match="no CPU path"):
        TA.augment_color(torch.zeros(3 * 48), [dict(offset=0, h=4, w=12, portrait=False)], 4, 12)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TA.augment_depth([torch.zeros(10, 20)], [AR.geometry(20, 10, _K(20, 10, 5), (8, 4))], 4, 8)
    frames = [np.zeros((97, 131, 3), np.uint8), np.zeros((131, 97, 3), np.uint8)]
    with pytest.raises(ValueError, match="stored shape"):
        TA.augment_views(frames, [f[..., 0].astype(np.float32) for f in frames], [_K(100, 65, 48), _K(100, 48, 65)], (64, 48), landscape=False)
    with pytest.raises(ValueError, match="depth map of shape"):
        TA.augment_views(frames[:1], [np.zeros((4, 4), np.float32)], [_K(100, 65, 48)], (64, 48))
