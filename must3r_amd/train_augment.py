"""Training augmentation on the device: a raw dataset frame -- its own size, depth map and intrinsics -- becomes a view of the training batch::

    out = augment_views(frames, depths, intrinsics, resolution=(512, 384), rng=rng, aug_crop=16, jitter=(0.5, 0.5, 0.5, 0.1))
    dataset = AugmentedScenes(raw_dataset, (512, 384), aug_crop=16, jitter=(0.5, 0.5, 0.5, 0.1))      # items are what train_data.collate_views takes

The reference's datasets do this per view on the host: dust3r's ``BaseStereoViewDataset._crop_resize_if_necessary`` with ``cropping.py`` (PIL crop and resize of the
image, cv2 nearest-neighbour resize of the depth map, the intrinsics carried along), the transform ``Compose([ColorJitter(0.5, 0.5, 0.5, 0.1), ImgNorm])`` on the PIL
image, and ``transpose_to_landscape``.  Here the host does the geometry alone, in float64 numpy, and the pixels never leave the device:

* ``crop_resize_geometry`` is the chain of crops and scales for one frame.  dust3r is not a dependency of this project: the chain is restated from memory, the
  restatement is the definition, and tests/augment_ref.py states it a second time.  The yardstick is that stated chain, not dust3r.
* The image goes through ``must3r_hip_resample`` in its Pillow modes (LANCZOS when the frame shrinks, BICUBIC otherwise; bit-exact with ``Image.resize``), crop =
  the first crop, resize = the rescaled size, window = the final crop: at most two calls for a batch of any mix of sizes, one per mode present.
* ``must3r_hip_augment_color`` (csrc/train_augment.hip) applies the colour jitter to the whole batch in one launch per pass and writes the ImgNorm image; its
  arithmetic is Pillow's, through which torchvision's PIL backend works, and tests/augment_ref.py compares it with the Pillow calls bit for bit.
  ``get_jitter_params`` draws a view's parameters as ``ColorJitter.get_params`` is recalled to: ``torch.randperm(4)``, then one ``uniform_`` each for brightness,
  contrast, saturation and hue.  Only that order is claimed: torchvision is not a dependency, so parity with its random stream is not tested.
* ``must3r_hip_augment_depth`` gathers the depth maps through the same geometry by nearest neighbour (OpenCV's ``INTER_NEAREST`` with an explicit size as
  recalled; cv2 is no dependency either, the formula in include/must3r_hip.h is the definition), fp32 or uint16, sky and holes untouched.
* With ``landscape`` a portrait view is written with its axes swapped by both kernels: ``train_data``'s convention -- ``true_shape`` = (W, H), the intrinsics
  those of the true image.

Nothing is read back, all work is on the current stream, and a view's bits are the same alone and in a batch.

``SyntheticRawScenes`` shows the scenes of ``train_data.SyntheticDepthScenes`` as raw frames of mixed sizes and orientations with off-centre principal points.

Not built: the dataset classes and samplers, ``train(args)``, DDP and ``--amp fp16``, JPEG decoding (frames arrive decoded, as uint8), and any augmentation other
than crop, resize and this colour jitter.  CPU tensors raise."""
import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _lib, image as _image
from ._train_common import _dev, _ptr, _scratch, _stream

OPS = ("brightness", "contrast", "saturation", "hue")     # _lib.AUG_*: the index of an operation


@dataclasses.dataclass
class Geometry:
    """What ``crop_resize_geometry`` decides for one frame, corners as (left, top, right, bottom), sizes as (width, height)."""
    crop1: tuple        # the first crop in the raw frame, centred on the principal point
    size1: tuple        # its size
    scale: float
    resized: tuple      # the size the first crop is rescaled to
    mode: int           # _lib.RESAMPLE_PIL_LANCZOS when scale < 1, else _lib.RESAMPLE_PIL_BICUBIC
    window: tuple       # the final crop inside the rescaled image
    out: tuple          # its size: the resolution, swapped for a portrait frame
    K: np.ndarray       # float64 [3, 3], the intrinsics of the window

    @property
    def portrait(self):
        return self.out[1] > self.out[0]


def camera_matrix_of_crop(K, in_size, out_size, scaling=1.0):
    """The intrinsics of the centred ``out_size`` crop of an image of ``in_size`` scaled by ``scaling`` (pixel centres at half integers)."""
    K = np.array(K, dtype=np.float64)
    margins = np.asarray(in_size, dtype=np.float64) * scaling - np.asarray(out_size, dtype=np.float64)
    assert np.all(margins >= 0.0), (in_size, out_size, scaling)
    offset = 0.5 * margins
    K[:2, 2] += 0.5
    K[:2, :] *= scaling
    K[:2, 2] -= offset
    K[:2, 2] -= 0.5
    return K


def crop_resize_geometry(W, H, K, resolution, rng=None, aug_crop=0):
    """dust3r's ``_crop_resize_if_necessary`` for a ``W`` x ``H`` frame with intrinsics ``K`` and the target ``resolution = (w, h)``, ``w >= h``, as restated in
    the module docstring's sense: the first crop centres the principal point, a portrait crop swaps the resolution (a near-square one on ``rng.integers(2)``,
    drawn only when ``rng`` is given), the crop is rescaled so that it covers the resolution (plus ``rng.integers(0, aug_crop)`` pixels on both axes when
    ``aug_crop > 1``) and the centred window of the resolution is cut out.  -> ``Geometry``.  ``ValueError``: a principal point too near the border
    (``min(cx, W - cx) <= W / 5`` or the like in y), ``w < h``, a window outside the rescaled image, ``aug_crop > 1`` without ``rng``."""
    W, H = int(W), int(H)
    K = np.array(K, dtype=np.float64)
    if K.shape != (3, 3) or W <= 0 or H <= 0:
        raise ValueError(f"crop_resize_geometry: a {W} x {H} frame with intrinsics of shape {K.shape}")
    w, h = (int(v) for v in resolution)
    if not w >= h > 0:
        raise ValueError(f"crop_resize_geometry: resolution {tuple(resolution)} is (w, h) with w >= h")
    if aug_crop > 1 and rng is None:
        raise ValueError("crop_resize_geometry: aug_crop draws from rng")
    # the first crop
    cx, cy = (int(v) for v in np.round(K[:2, 2]))
    mx, my = min(cx, W - cx), min(cy, H - cy)
    if not (mx > W / 5 and my > H / 5):
        raise ValueError(f"crop_resize_geometry: principal point ({cx}, {cy}) too close to the border of the {W} x {H} frame")
    crop1 = (cx - mx, cy - my, cx + mx, cy + my)
    K[0, 2] -= crop1[0]
    K[1, 2] -= crop1[1]
    W, H = 2 * mx, 2 * my
    # the orientation
    if H > 1.1 * W:
        w, h = h, w
    elif 0.9 < H / W < 1.1 and w != h and rng is not None:
        if rng.integers(2):
            w, h = h, w
    # the rescale
    target = np.array([w, h], dtype=np.float64)
    if aug_crop > 1:
        target = target + rng.integers(0, aug_crop)
    size1 = np.array([W, H], dtype=np.float64)
    scale = float(np.max(target / size1)) + 1e-8
    resized = np.floor(size1 * scale).astype(int)
    mode = _lib.RESAMPLE_PIL_LANCZOS if scale < 1 else _lib.RESAMPLE_PIL_BICUBIC
    K = camera_matrix_of_crop(K, (W, H), resized, scaling=scale)
    # the final crop
    K2 = camera_matrix_of_crop(K, resized, (w, h), scaling=1)
    l, t = (int(v) for v in np.int32(np.round(K[:2, 2] - K2[:2, 2])))
    window = (l, t, l + w, t + h)
    K[0, 2] -= l
    K[1, 2] -= t
    if l < 0 or t < 0 or window[2] > resized[0] or window[3] > resized[1]:
        raise ValueError(f"crop_resize_geometry: the window {window} does not lie inside the {resized[0]} x {resized[1]} rescaled image")
    return Geometry(crop1, (W, H), scale, (int(resized[0]), int(resized[1])), mode, window, (w, h), K)


def get_jitter_params(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.1, generator=None):
    """One view's parameters as ``ColorJitter(brightness, contrast, saturation, hue).get_params`` draws them: ``torch.randperm(4)``, then one
    ``torch.empty(1).uniform_(lo, hi)`` each for brightness, contrast and saturation in ``[max(0, 1 - v), 1 + v]`` and hue in ``[-hue, hue]`` -> ``(order,
    factors)``, both by ``OPS``' indices.  (Only this order of draws is claimed, not torchvision's stream.)"""
    if min(brightness, contrast, saturation, hue) < 0 or hue > 0.5:
        raise ValueError("get_jitter_params: magnitudes are non-negative, hue at most 0.5")
    order = [int(i) for i in torch.randperm(4, generator=generator)]
    factors = [float(torch.empty(1).uniform_(max(0.0, 1.0 - v), 1.0 + v, generator=generator)) for v in (brightness, contrast, saturation)]
    factors.append(float(torch.empty(1).uniform_(-hue, hue, generator=generator)))
    return order, factors


class _Prepared:
    """A descriptor with its table, its scratch and the tensors it points to: ``run()`` queues the call on the current stream and returns the output.  (The
    two wrappers below prepare and run once; scripts/bench_augment.py runs a prepared call many times, so that its events see the launches and not the host's
    work on the table.)"""

    def __init__(self, entry, a, table, nbytes, dev, out, keep):
        self.entry, self.a, self.table, self.dev, self.out, self.keep = entry, a, table, dev, out, keep
        with torch.cuda.device(dev):
            self.scratch = _scratch(nbytes, dev)
        a.views, a.scratch, a.scratch_bytes = table, _ptr(self.scratch), nbytes

    def run(self):
        with torch.cuda.device(self.dev):
            self.a.stream = _stream(self.dev)
            _lib.check(self.entry(C.byref(self.a)))
        return self.out


def _out(out, shape, dtype, dev, who):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not out.is_cuda or tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"{who}: out is a contiguous {dtype} tensor of shape {shape} on the GPU")
    return out


def augment_color(src, views, Hs, Ws, out=None):
    """``must3r_hip_augment_color`` (``prepare_color(...).run()``): ``src`` the resampler's fp32 output (flat, on the GPU), ``views`` a list of dicts -- ``offset`` (elements into ``src``),
    ``h``, ``w``, ``portrait``, and optionally ``order``, ``factors`` and ``flags`` by ``OPS``' indices (no ``order``: nothing is applied) -> the ImgNorm batch
    fp32 ``[V, 3, Hs, Ws]`` (written into ``out`` where one is given)."""
    return prepare_color(src, views, Hs, Ws, out).run()


def prepare_color(src, views, Hs, Ws, out=None):
    _dev(src, "augment_color: src")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("augment_color: src is a contiguous fp32 tensor")
    V = len(views)
    table = (_lib.AugmentColorView * max(V, 1))()
    for t, v in zip(table, views):
        t.src_offset, t.h, t.w, t.portrait = int(v["offset"]), int(v["h"]), int(v["w"]), int(bool(v["portrait"]))
        order = v.get("order")
        t.order[:] = [int(i) for i in order] if order is not None else [0, 1, 2, 3]
        t.apply[:] = [int(f) for f in v.get("flags", (1, 1, 1, 1))] if order is not None else [0, 0, 0, 0]
        t.factor[:] = [float(f) for f in v["factors"]] if order is not None else [1.0, 1.0, 1.0, 0.0]
    out = _out(out, (V, 3, int(Hs), int(Ws)), torch.float32, src.device, "augment_color")
    lib = _lib.load()
    a = _lib.AugmentColorArgs()
    a.src, a.src_elems, a.out = _ptr(src), src.numel(), _ptr(out)
    a.V, a.Hs, a.Ws = V, int(Hs), int(Ws)
    return _Prepared(lib.must3r_hip_augment_color, a, table, lib.must3r_hip_augment_color_scratch_bytes(V, int(Hs), int(Ws)), src.device, out, src)


def augment_depth(depths, geometries, Hs, Ws, landscape=True, out=None):
    """``must3r_hip_augment_depth`` (``prepare_depth(...).run()``): ``depths`` a list of raw depth maps ``[H, W]`` on the GPU, all fp32 or all uint16 (rows may be strided), ``geometries``
    their ``Geometry`` -> ``[V, Hs, Ws]`` of the same dtype (written into ``out`` where one is given), a portrait view with its axes swapped when ``landscape``."""
    return prepare_depth(depths, geometries, Hs, Ws, landscape, out).run()


def prepare_depth(depths, geometries, Hs, Ws, landscape=True, out=None):
    V = len(depths)
    if V == 0 or len(geometries) != V:
        raise ValueError("augment_depth: one geometry per depth map, and at least one")
    dtype = depths[0].dtype
    if dtype not in (torch.float32, torch.uint16):
        raise ValueError(f"augment_depth: depth of dtype {dtype}, expected fp32 or uint16")
    table = (_lib.AugmentDepthView * V)()
    keep = []
    for t, d, g in zip(table, depths, geometries):
        _dev(d, "augment_depth: depth")
        if d.ndim != 2 or d.dtype != dtype or d.numel() == 0:
            raise ValueError(f"augment_depth: a depth map of shape {tuple(d.shape)} and dtype {d.dtype}, expected {dtype} [H, W]")
        if d.stride(1) != 1:
            d = d.contiguous()
        keep.append(d)
        t.src, t.row_stride, t.H, t.W = d.data_ptr(), int(d.stride(0)) if d.shape[0] > 1 else int(d.shape[1]), int(d.shape[0]), int(d.shape[1])
        t.crop_x, t.crop_y, t.crop_w, t.crop_h = g.crop1[0], g.crop1[1], g.size1[0], g.size1[1]
        t.resize_w, t.resize_h = g.resized
        t.win_x, t.win_y, t.out_w, t.out_h = g.window[0], g.window[1], g.out[0], g.out[1]
        t.portrait = int(landscape and g.portrait)
    dev = depths[0].device
    out = _out(out, (V, int(Hs), int(Ws)), dtype, dev, "augment_depth")
    lib = _lib.load()
    a = _lib.AugmentDepthArgs()
    a.out, a.V, a.Hs, a.Ws, a.depth_u16 = _ptr(out), V, int(Hs), int(Ws), int(dtype == torch.uint16)
    return _Prepared(lib.must3r_hip_augment_depth, a, table, lib.must3r_hip_augment_depth_scratch_bytes(V), dev, out, keep)


def stored_shape(geometries, landscape=True):
    """(Hs, Ws) of a batch of views, a portrait view counted with its axes swapped when ``landscape``; ``ValueError`` when the views do not share one."""
    shapes = {(g.out[0], g.out[1]) if landscape and g.portrait else (g.out[1], g.out[0]) for g in geometries}
    if len(shapes) != 1:
        raise ValueError(f"augment_views: the views of a batch must share one stored shape, got {sorted(shapes)} (h, w)"
                         + ("" if landscape else "; landscape=True stores a portrait view with its axes swapped"))
    return shapes.pop()


def _to_device(x, dev, what):
    """a numpy array or CPU tensor through pinned memory (``image._upload_u8``'s way); a CUDA tensor as it is"""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"augment_views: {what} is a numpy array or a tensor")
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t)
    return host.to(dev, non_blocking=True)


def augment_views(frames, depths, intrinsics, resolution, rng=None, aug_crop=0, jitter=None, jitter_params=None, generator=None, landscape=True,
                  device=None):
    """``V`` raw views to one training batch.  ``frames``: a list of HxWx3 uint8 (numpy arrays go through pinned memory, CUDA tensors are used as they are);
    ``depths``: their HxW depth maps, all fp32 or all uint16; ``intrinsics``: their 3x3 matrices; ``resolution = (w, h)``, ``w >= h``.  ``rng`` (a numpy
    ``Generator``) and ``aug_crop`` are ``crop_resize_geometry``'s, drawn view by view.  The colour jitter of a view is ``jitter_params[v]`` = ``(order,
    factors)`` or ``(order, factors, flags)`` by ``OPS``' indices (``None``: none for that view), else drawn by ``jitter_params(*jitter, generator)`` view
    by view when ``jitter = (brightness, contrast, saturation, hue)`` is given, else none.  -> a dict on the device: ``img`` fp32 ``[V, 3, Hs, Ws]`` (ImgNorm),
    ``depthmap`` ``[V, Hs, Ws]`` in the depths' dtype, ``camera_intrinsics`` fp32 ``[V, 3, 3]`` and ``true_shape`` int32 ``[V, 2]`` (h, w): the depth form
    ``train_data.collate_views`` and ``ground_truth`` take.  With ``landscape`` a portrait view is stored with its axes swapped; a batch whose views do not
    share one stored shape raises before anything is launched."""
    V = len(frames)
    if V == 0 or len(depths) != V or len(intrinsics) != V:
        raise ValueError("augment_views: one depth map and one intrinsics matrix per frame, and at least one frame")
    if jitter_params is not None and len(jitter_params) != V:
        raise ValueError("augment_views: jitter_params has one entry per view")
    for f, d in zip(frames, depths):
        if len(f.shape) != 3 or f.shape[2] != 3 or tuple(d.shape) != tuple(f.shape[:2]):
            raise ValueError(f"augment_views: a frame of shape {tuple(f.shape)} with a depth map of shape {tuple(d.shape)}, expected HxWx3 and HxW")
        if not str(f.dtype).endswith("uint8"):
            raise ValueError(f"augment_views: frames are uint8, got {f.dtype}")
    geoms = [crop_resize_geometry(f.shape[1], f.shape[0], np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64), resolution, rng, aug_crop)
             for f, K in zip(frames, intrinsics)]
    Hs, Ws = stored_shape(geoms, landscape)
    if jitter_params is None:
        jitter_params = [get_jitter_params(*jitter, generator=generator) for _ in range(V)] if jitter is not None else [None] * V
    if device is None:
        cuda = [x for x in (*frames, *depths) if isinstance(x, torch.Tensor) and x.is_cuda]
        device = cuda[0].device if cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("must3r_amd training: augment_views works on the GPU (there is no CPU path)")
    with torch.cuda.device(dev):
        srcs = [_to_device(f, dev, "a frame").contiguous() for f in frames]
        raws = [_to_device(d, dev, "a depth map") for d in depths]
        # the image: crop, Pillow resize and window, one call per mode present
        views, descs, off = [], {}, 0
        for v, (src, g) in enumerate(zip(srcs, geoms)):
            H, W = int(src.shape[0]), int(src.shape[1])
            (w, h), jp = g.out, jitter_params[v]
            descs.setdefault(g.mode, []).append(_image._desc(src, _lib.IMG_U8_HWC, 3, H, W, W * 3, 0, (g.crop1[1], g.crop1[0], g.size1[1], g.size1[0]),
                                                             (g.resized[1], g.resized[0]), (g.window[1], g.window[0], h, w), off))
            view = dict(offset=off, h=h, w=w, portrait=landscape and g.portrait)
            if jp is not None:
                view.update(order=jp[0], factors=jp[1], flags=jp[2] if len(jp) > 2 else (1, 1, 1, 1))
            views.append(view)
            off += 3 * h * w
        mid = torch.empty((off,), dtype=torch.float32, device=dev)
        for mode in sorted(descs):
            _image._resample(mode, descs[mode], mid, srcs)
        img = augment_color(mid, views, Hs, Ws)
        depth = augment_depth(raws, geoms, Hs, Ws, landscape)
        K = _to_device(torch.from_numpy(np.stack([g.K for g in geoms]).astype(np.float32)), dev, "K")
        true_shape = _to_device(torch.tensor([[g.out[1], g.out[0]] for g in geoms], dtype=torch.int32), dev, "true_shape")
    return dict(img=img, depthmap=depth, camera_intrinsics=K, true_shape=true_shape)


class AugmentedScenes:
    """A dataset of raw scenes seen through ``augment_views``.  ``raw_dataset[i]`` is a list of raw view dicts: ``img`` uint8 HxWx3, ``depthmap`` HxW (fp32, or
    uint16 with ``depth_scale``), ``camera_intrinsics`` 3x3, ``camera_pose`` 4x4, and optionally ``depth_scale``, ``is_metric_scale`` and ``memory_num_views``.
    ``dataset[i]`` is the list of view dicts ``train_data.collate_views`` takes, on the device: ``img`` fp32 ``[3, Hs, Ws]``, ``depthmap`` ``[Hs, Ws]``,
    ``camera_intrinsics``, ``true_shape``; ``camera_pose``, ``depth_scale``, ``is_metric_scale`` and ``memory_num_views`` pass through.  The draws of item ``i``
    in epoch ``e`` come from generators seeded with (``seed``, ``e``, ``i``): an item does not depend on the order in which items are asked for."""

    def __init__(self, raw_dataset, resolution, aug_crop=0, jitter=None, seed=0, landscape=True, device=None):
        self.raw, self.resolution, self.aug_crop, self.jitter = raw_dataset, tuple(resolution), int(aug_crop), jitter
        self.seed, self.landscape, self.device, self.epoch = int(seed), bool(landscape), device, 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        if hasattr(self.raw, "set_epoch"):
            self.raw.set_epoch(epoch)

    def __len__(self):
        return len(self.raw)

    def generators(self, idx):
        """(numpy Generator for the geometry, torch Generator for the jitter) of item ``idx`` in the current epoch"""
        return (np.random.default_rng([self.seed, self.epoch, int(idx)]),
                torch.Generator().manual_seed((self.seed * 1000003 + self.epoch) * 1000003 + int(idx)))

    def __getitem__(self, idx):
        raw = self.raw[idx]
        rng, gen = self.generators(idx)
        out = augment_views([v["img"] for v in raw], [v["depthmap"] for v in raw], [v["camera_intrinsics"] for v in raw], self.resolution, rng=rng,
                            aug_crop=self.aug_crop, jitter=self.jitter, generator=gen, landscape=self.landscape, device=self.device)
        views = []
        for i, v in enumerate(raw):
            view = {k: out[k][i] for k in ("img", "depthmap", "camera_intrinsics", "true_shape")}
            view["camera_pose"] = torch.as_tensor(v["camera_pose"], dtype=torch.float32)
            for k in ("depth_scale", "is_metric_scale", "memory_num_views"):
                if k in v:
                    view[k] = torch.as_tensor(v[k])
            views.append(view)
        return views


class SyntheticRawScenes:
    """The scenes of ``train_data.SyntheticDepthScenes`` as raw frames: view ``v`` of a scene is the top-left ``sizes[v % len(sizes)] = (H, W)`` part of a
    square synthetic view of side ``max(sizes)``, with its principal point ``offcentre`` (a fraction of the size, the sign alternating with ``v``) away from
    the centre.  ``dataset[i]`` is a list of ``n_views`` dicts: ``img`` uint8 ``[H, W, 3]``, ``depthmap`` fp32 ``[H, W]`` (0: invalid, -1: sky; ``raw_depth``:
    uint16 millimetres with ``depth_scale``), ``camera_intrinsics`` fp32 ``[3, 3]``, ``camera_pose``, ``is_metric_scale`` and ``memory_num_views``."""

    def __init__(self, n_scenes, n_views, sizes, seed=0, raw_depth=False, offcentre=(0.06, 0.04), memory_num_views=None):
        from .train_data import SyntheticDepthScenes
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        side = max(max(s) for s in self.sizes)
        self.base = SyntheticDepthScenes(n_scenes, n_views, side, side, seed=seed, uint8_img=True, raw_depth=raw_depth, memory_num_views=memory_num_views)
        self.offcentre = (float(offcentre[0]), float(offcentre[1]))

    def set_epoch(self, epoch):
        pass

    def __len__(self):
        return len(self.base)

    def __getitem__(self, idx):
        views = []
        for v, b in enumerate(self.base[idx]):
            H, W = self.sizes[v % len(self.sizes)]
            sign = -1.0 if v % 2 else 1.0
            K = b["camera_intrinsics"].clone()
            K[0, 2] = W / 2 + sign * self.offcentre[0] * W
            K[1, 2] = H / 2 - sign * self.offcentre[1] * H
            view = dict(img=b["img"][:, :H, :W].permute(1, 2, 0).contiguous(), depthmap=b["depthmap"][:H, :W].contiguous(), camera_intrinsics=K,
                        camera_pose=b["camera_pose"], is_metric_scale=b["is_metric_scale"], memory_num_views=b["memory_num_views"])
            if "depth_scale" in b:
                view["depth_scale"] = b["depth_scale"]
            views.append(view)
        return views
