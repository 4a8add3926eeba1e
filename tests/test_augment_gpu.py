"""GPU (-m gpu): the training augmentation (must3r_amd/train_augment.py, csrc/train_augment.hip) against tests/augment_ref.py -- the real Pillow calls and the
stated geometry and depth formulas.  Every comparison is torch.equal: no tolerance is involved."""
import itertools

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import augment_ref as AR
from must3r_amd import train_augment as TA, train_data as TD

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _src(images):
    """the resampler's output for these uint8 HxWx3 images: their ImgNorm planes, end to end -> (flat fp32 tensor on the GPU, offsets)"""
    planes = [AR.img_norm_np(im).reshape(-1) for im in images]
    offsets = np.concatenate([[0], np.cumsum([p.size for p in planes])])[:-1]
    return torch.from_numpy(np.concatenate(planes)).to(DEV), [int(o) for o in offsets]


def _color(images, params, portrait=None, Hs=None, Ws=None):
    """one launch of the colour kernel on ``images`` with ``params[v] = (order, factors, flags)`` or None -> the batch on the CPU"""
    src, offsets = _src(images)
    portrait = portrait or [False] * len(images)
    views = []
    for im, off, jp, pt in zip(images, offsets, params, portrait):
        v = dict(offset=off, h=im.shape[0], w=im.shape[1], portrait=pt)
        if jp is not None:
            v.update(order=jp[0], factors=jp[1], flags=jp[2])
        views.append(v)
    h, w = images[0].shape[:2]
    Hs, Ws = (Hs, Ws) if Hs else ((w, h) if portrait[0] else (h, w))
    out = TA.augment_color(src, views, Hs, Ws)
    torch.cuda.synchronize()
    return out.cpu()


def _color_ref(im, jp, portrait=False):
    u8 = im if jp is None else AR.jitter_pil(im, *jp)
    x = AR.img_norm_np(u8)
    return torch.from_numpy(np.ascontiguousarray(x.swapaxes(1, 2)) if portrait else x)


def _random_image(seed, h, w):
    """smooth ramps plus noise: every byte value occurs, and saturated and grey pixels too"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    base = np.stack([(xs * 255 // max(w - 1, 1)), (ys * 255 // max(h - 1, 1)), ((xs + ys) * 255 // (h + w - 2))], axis=-1)
    img = np.clip(base + rng.integers(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)
    img[:4, :4] = rng.integers(0, 256, size=(4, 4, 1))       # greys
    img[4:6, :6] = (255, 0, 0)
    img[6:8, :6] = 0
    img[8:10, :6] = 255
    return img


# ---------------------------------------------------------------------------------------------------------------------------------
# colour
# ---------------------------------------------------------------------------------------------------------------------------------
def test_all_24_orders_in_one_launch():
    """24 views, one per order of the four operations; factors at the ends of ColorJitter(0.5, 0.5, 0.5, 0.1)'s ranges and inside them; every third view is a
    portrait 64 x 48 image stored as 48 x 64"""
    ends = ([0.5, 1.5, 0.77, 1.3141592], [1.5, 0.5, 1.23, 0.6180339], [0.5, 1.5, 1.0, 1.4142135], [-0.1, 0.1, 0.04, -0.0733])
    images, params, portrait = [], [], []
    for i, order in enumerate(itertools.permutations(range(4))):
        pt = i % 3 == 2
        images.append(_random_image(i, 64, 48) if pt else _random_image(i, 48, 64))
        params.append((list(order), [ends[k][(i + k) % 4] for k in range(4)], (1, 1, 1, 1)))
        portrait.append(pt)
    assert len(images) == 24
    got = _color(images, params, portrait, 48, 64)
    assert got.shape == (24, 3, 48, 64)
    for i in range(24):
        assert torch.equal(got[i], _color_ref(images[i], params[i], portrait[i])), (i, params[i])


def test_each_operation_alone_and_none():
    img = _random_image(100, 48, 64)
    factors = [1.37, 0.66, 1.45, -0.09]
    params = [([0, 1, 2, 3], factors, tuple(int(k == op) for k in range(4))) for op in range(4)]
    params += [([2, 0, 3, 1], factors, (0, 0, 0, 0)), None]
    got = _color([img] * 6, params)
    for i in range(4):
        assert torch.equal(got[i], _color_ref(img, params[i])), TA.OPS[i]
        assert not torch.equal(got[i], got[5]), TA.OPS[i]
    copy = torch.from_numpy(AR.img_norm_np(img))
    assert torch.equal(got[4], copy) and torch.equal(got[5], copy)                  # every flag off: a copy


def test_odd_sizes_and_partial_tiles():
    """65 x 129 (landscape) and 129 x 65 (portrait): two tiles down, three across, the last of each one pixel wide"""
    a, b = _random_image(7, 65, 129), _random_image(8, 129, 65)
    params = [([1, 3, 0, 2], [1.2, 1.4, 0.7, 0.05], (1, 1, 1, 1)), ([3, 2, 1, 0], [0.8, 0.6, 1.3, -0.02], (1, 1, 1, 1))]
    got = _color([a, b], params, [False, True], 65, 129)
    assert torch.equal(got[0], _color_ref(a, params[0])) and torch.equal(got[1], _color_ref(b, params[1], True))
    alone = _color([b], params[1:], [True], 65, 129)
    assert torch.equal(alone[0], got[1])                                            # the same bits alone and in a batch


def test_all_colours_through_hue_and_saturation():
    """the 4096 x 4096 image of all 2^24 colours: where the device's fp32 division and fp64 arithmetic could differ from the host's"""
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    params = [([0, 1, 2, 3], [1.0, 1.0, 1.0, 0.1], (0, 0, 0, 1)), ([0, 1, 2, 3], [1.0, 1.0, 1.37, 0.0], (0, 0, 1, 0))]
    src = torch.from_numpy(AR.img_norm_np(img).reshape(-1)).to(DEV)
    views = [dict(offset=0, h=4096, w=4096, portrait=False, order=p[0], factors=p[1], flags=p[2]) for p in params]
    out = TA.augment_color(src, views, 4096, 4096)
    for i, name in enumerate(("hue", "saturation")):
        ref = torch.from_numpy(AR.img_norm_np(AR.jitter_pil(img, *params[i]))).to(DEV)
        assert torch.equal(out[i], ref), name


def test_contrast_mean_at_the_rounding_boundary():
    below, above = AR.contrast_boundary_images()
    images = [below, below, above, above]
    params = [([0, 1, 2, 3], [1.0, f, 1.0, 0.0], (0, 1, 0, 0)) for f in (0.5, 1.5, 0.5, 1.5)]
    got = _color(images, params)
    for i in range(4):
        assert torch.equal(got[i], _color_ref(images[i], params[i])), i
    assert not torch.equal(got[0], got[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# depth
# ---------------------------------------------------------------------------------------------------------------------------------
def _K(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def _raw_depth(seed, H, W, u16):
    rng = np.random.default_rng(seed)
    if u16:
        d = rng.integers(1, 65536, size=(H, W)).astype(np.uint16)
        d[rng.random((H, W)) < 0.1] = 0
        return d
    d = rng.uniform(0.5, 9.0, size=(H, W)).astype(np.float32)
    d[rng.random((H, W)) < 0.1] = 0.0                 # holes
    d[: H // 4][rng.random((H // 4, W)) < 0.5] = -1.0  # sky
    return d


@pytest.mark.parametrize("u16", [False, True], ids=["fp32", "uint16"])
def test_depth_gather_with_canaries(u16):
    """97 x 131 -> 48 x 64 and a portrait 160 x 120 -> 64 x 48 stored as 48 x 64, in one launch, the output inside a buffer of canaries"""
    cases = [(97, 131, _K(110.0, 70.3, 45.1)), (160, 120, _K(140.0, 57.2, 84.9))]
    raws = [_raw_depth(i + 10 * u16, H, W, u16) for i, (H, W, _) in enumerate(cases)]
    geoms = [TA.crop_resize_geometry(W, H, K, (64, 48)) for H, W, K in cases]
    assert [g.portrait for g in geoms] == [False, True] and all(g.crop1[0] > 0 or g.crop1[1] > 0 for g in geoms)
    dtype, canary = (torch.uint16, 0xABCD) if u16 else (torch.float32, -777.0)
    pad, n = 1024, 2 * 48 * 64
    buf = torch.full((n + 2 * pad,), canary, dtype=torch.int32 if u16 else dtype).to(dtype).to(DEV)
    devs = [torch.from_numpy(r.astype(np.int32)).to(torch.uint16).to(DEV) if u16 else torch.from_numpy(r).to(DEV) for r in raws]
    out = TA.augment_depth(devs, geoms, 48, 64, out=buf[pad:pad + n].view(2, 48, 64))
    torch.cuda.synchronize()
    host = buf.cpu().view(torch.int16 if u16 else dtype).numpy()
    want_canary = np.array([canary], dtype=np.uint16).view(np.int16)[0] if u16 else np.float32(canary)
    assert (host[:pad] == want_canary).all() and (host[pad + n:] == want_canary).all()
    got = host[pad:pad + n].reshape(2, 48, 64)
    for i, (H, W, K) in enumerate(cases):
        ref = AR.depth_gather(raws[i], AR.geometry(W, H, K, (64, 48)))
        ref = ref.T if i == 1 else ref
        assert ref.shape == (48, 64) and np.array_equal(got[i].view(np.uint16) if u16 else got[i], ref), i
    if not u16:
        assert (got < 0).any() and (got == 0).any() and out.dtype == torch.float32


def test_depth_without_landscape_keeps_the_portrait_orientation():
    H, W, K = 160, 120, _K(140.0, 57.2, 84.9)
    raw = _raw_depth(3, H, W, False)
    g = TA.crop_resize_geometry(W, H, K, (64, 48))
    out = TA.augment_depth([torch.from_numpy(raw).to(DEV)], [g], 64, 48, landscape=False)
    assert np.array_equal(out[0].cpu().numpy(), AR.depth_gather(raw, AR.geometry(W, H, K, (64, 48))))


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole pipeline
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = [(97, 131), (131, 97), (120, 120), (40, 52)]        # (H, W); the last is an upscale: BICUBIC
RES = (64, 48)
KEYS = ("img", "depthmap", "camera_intrinsics", "true_shape")


@pytest.fixture(scope="module")
def raw_views():
    views = TA.SyntheticRawScenes(1, 4, SIZES, seed=11)[0]
    gen = torch.Generator().manual_seed(21)
    jps = [TA.get_jitter_params(0.5, 0.5, 0.5, 0.1, generator=gen) for _ in views]
    return views, jps


def _reference(views, jps, seed, landscape, aug_crop=8):
    """the yardstick view by view, drawing from one generator in the order of the views; also the generator's state in front of each view"""
    rng = np.random.default_rng(seed)
    out, states = [], []
    for v, jp in zip(views, jps):
        states.append(rng.bit_generator.state)
        out.append(AR.view_ref(v["img"].numpy(), v["depthmap"].numpy(), v["camera_intrinsics"].numpy(), RES, rng, aug_crop,
                               None if jp is None else (jp[0], jp[1], (1, 1, 1, 1)), landscape))
    return out, states


def _augment(views, jps, rng, landscape, aug_crop=8):
    out = TA.augment_views([v["img"].numpy() for v in views], [v["depthmap"] for v in views], [v["camera_intrinsics"] for v in views], RES, rng=rng,
                           aug_crop=aug_crop, jitter_params=jps, landscape=landscape)
    torch.cuda.synchronize()
    return {k: out[k].cpu() for k in KEYS}


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(got, i, ref):
    """the keys whose bits differ"""
    return [k for k in KEYS if got[k][i].shape != ref[k].shape or got[k][i].dtype != ref[k].dtype or not torch.equal(_bits(got[k][i]), _bits(ref[k]))]


def test_whole_pipeline_stored_landscape(raw_views):
    views, jps = raw_views
    ref, states = _reference(views, jps, 5, True)
    modes = {r["geometry"].lanczos for r in ref}
    assert modes == {True, False} and not ref[3]["geometry"].lanczos and ref[1]["true_shape"].tolist() == [64, 48] and ref[0]["true_shape"].tolist() == [48, 64]
    got = _augment(views, jps, np.random.default_rng(5), True)
    assert got["img"].shape == (4, 3, 48, 64) and got["depthmap"].shape == (4, 48, 64) and got["camera_intrinsics"].dtype == torch.float32
    assert got["true_shape"].dtype == torch.int32
    for i in range(4):
        assert not _same(got, i, ref[i]), (i, _same(got, i, ref[i]))
    again = _augment(views, jps, np.random.default_rng(5), True)
    assert all(torch.equal(got[k], again[k]) for k in KEYS)                         # two runs, the same bits
    for i in range(4):                                                              # a view alone: the same bits as in the batch
        rng = np.random.default_rng(0)
        rng.bit_generator.state = states[i]
        alone = _augment(views[i:i + 1], jps[i:i + 1], rng, True)
        assert all(torch.equal(alone[k][0], got[k][i]) for k in KEYS), i


def test_whole_pipeline_in_true_orientation(raw_views):
    views, jps = raw_views
    ref, states = _reference(views, jps, 5, False)
    shapes = [tuple(r["img"].shape[1:]) for r in ref]
    assert shapes[0] == shapes[3] == (48, 64) and shapes[1] == (64, 48)
    for group in ([0, 3], [1], [2]):
        sub, sub_jps = [views[i] for i in group], [jps[i] for i in group]
        if len(group) == 2:          # views 0 and 3 draw one after the other in this call: the reference draws for them alone, in that order
            sub_ref, _ = _reference(sub, sub_jps, 5, False)
            rng = np.random.default_rng(5)
        else:
            sub_ref = [ref[group[0]]]
            rng = np.random.default_rng(0)
            rng.bit_generator.state = states[group[0]]
        got = _augment(sub, sub_jps, rng, False)
        for j in range(len(group)):
            assert not _same(got, j, sub_ref[j]), (group, j, _same(got, j, sub_ref[j]))
    with pytest.raises(ValueError, match="stored shape"):
        _augment(views[:2], jps[:2], np.random.default_rng(5), False)


def test_uint16_depth_and_no_jitter(raw_views):
    views = TA.SyntheticRawScenes(1, 4, SIZES, seed=12, raw_depth=True)[0]
    ref, _ = _reference(views, [None] * 4, 9, True)
    got = _augment(views, None, np.random.default_rng(9), True)
    assert got["depthmap"].dtype == torch.uint16
    for i in range(4):
        assert not _same(got, i, ref[i]), (i, _same(got, i, ref[i]))


# ---------------------------------------------------------------------------------------------------------------------------------
# through the loop's front
# ---------------------------------------------------------------------------------------------------------------------------------
def test_collate_views_of_an_augmented_batch():
    raw = TA.SyntheticRawScenes(2, 4, SIZES, seed=13, memory_num_views=2)
    jitter = (0.5, 0.5, 0.5, 0.1)
    ds = TA.AugmentedScenes(raw, RES, aug_crop=8, jitter=jitter, seed=3)
    ds.set_epoch(1)
    batch = next(iter(DataLoader(ds, batch_size=2)))
    assert len(batch) == 4 and batch[0]["img"].shape == (2, 3, 48, 64) and batch[0]["img"].is_cuda and "pts3d" not in batch[0]
    imgs, ts, gt = TD.collate_views(batch, DEV)
    refs = []
    for idx in range(2):
        rng, gen = ds.generators(idx)
        scene = []
        for v in raw[idx]:
            order, factors = TA.get_jitter_params(*jitter, generator=gen)      # (augment_views draws every view's geometry first, then every view's jitter:
            scene.append((v, (order, factors, (1, 1, 1, 1))))                  #  two generators, so the order between them does not matter)
        refs.append([AR.view_ref(v["img"].numpy(), v["depthmap"].numpy(), v["camera_intrinsics"].numpy(), RES, rng, 8, jp, True) for v, jp in scene])
    stack = lambda key: torch.stack([torch.stack([r[key] for r in scene]) for scene in refs])          # noqa: E731
    assert torch.equal(imgs.cpu(), stack("img")) and torch.equal(ts.cpu(), stack("true_shape"))
    assert {tuple(t) for t in ts.cpu().view(-1, 2).tolist()} == {(48, 64), (64, 48)}
    pose = torch.stack([torch.stack([v["camera_pose"] for v in raw[idx]]) for idx in range(2)])
    want = TD.ground_truth(stack("depthmap").to(DEV), stack("camera_intrinsics").to(DEV), pose.to(DEV), stack("true_shape").to(DEV))
    for i, g in enumerate(gt):
        assert set(g) == set(TD.GT_KEYS)
        for key in ("pts3d", "valid_mask", "sky_mask"):
            assert torch.equal(g[key], want[key][:, i]), (i, key)
        assert torch.equal(g["camera_pose"].cpu(), pose[:, i]) and g["memory_num_views"].tolist() == [2, 2] and g["is_metric_scale"].tolist() == [True, True]
    assert bool(gt[0]["valid_mask"].any()) and bool(gt[0]["sky_mask"].any()) and not bool(gt[0]["valid_mask"].all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the stream: the event method of tests/test_stream_order_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
def _on_delayed_side_stream(inputs, A, B, call):
    """``inputs`` hold the decoy B; on a side stream: a delay, copies of A into the inputs, the call, clones of its outputs, B back -- queued without a host
    synchronisation.  -> (the clones, whether the delay was still running when the call had returned on the host)"""
    import test_stream_order_gpu as SO
    delay = SO.Delay()
    for t, b in zip(inputs, B):
        t.copy_(b)
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(40.0)
        done.record()
        for t, a in zip(inputs, A):
            t.copy_(a)
        outs = call()
        premise = not done.query()
        got = [o.clone() for o in outs]
        for t, b in zip(inputs, B):
            t.copy_(b)
    s.synchronize()
    return got, premise


def test_both_entry_points_run_on_the_callers_stream():
    imgs = [_random_image(40 + i, 48, 64) for i in range(4)]
    params = [([1, 3, 0, 2], [1.2, 1.4, 0.7, 0.05], (1, 1, 1, 1))] * 2
    srcA, off = _src(imgs[:2])
    srcB, _ = _src(imgs[2:])
    views = [dict(offset=o, h=48, w=64, portrait=False, order=p[0], factors=p[1], flags=p[2]) for o, p in zip(off, params)]
    geoms = [TA.crop_resize_geometry(131, 97, _K(110.0, 70.3, 45.1), RES)]
    dA, dB = (torch.from_numpy(_raw_depth(s, 97, 131, False)).to(DEV) for s in (1, 2))
    src, depth = torch.empty_like(srcA), torch.empty_like(dA)

    def call():
        return [TA.augment_color(src, views, 48, 64), TA.augment_depth([depth], geoms, 48, 64)]

    src.copy_(srcA)
    depth.copy_(dA)
    ref = [o.clone() for o in call()]
    src.copy_(srcB)
    depth.copy_(dB)
    decoy = [o.clone() for o in call()]
    torch.cuda.synchronize()
    assert not torch.equal(ref[0], decoy[0]) and not torch.equal(ref[1], decoy[1])
    got, premise = _on_delayed_side_stream([src, depth], [srcA, dA], [srcB, dB], call)
    assert premise, "the delay ended before the calls had returned on the host: too short, or a host synchronisation inside them"
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
