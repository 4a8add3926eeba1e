"""The data side of a training step: ground truth from depth on the device, and the reference's batch brought into the form the loop needs::

    imgs, true_shape, gt = collate_views(batch, device)           # batch: the loader's list of n view dicts of [B, ...] tensors
    loss, details = criterion(gt, predictions)                    # train_losses.ConfLoss(Regr3D(...))

The reference's datasets compute ``pts3d``, ``valid_mask`` and ``sky_mask`` per view in numpy (must3r_base_dataset.py:185-198) and its criterion stacks and
uploads them: 14 bytes per pixel through the host, where the depth map they come from is 4 (fp32) or 2 (the raw 16-bit files).  Here a loader may hand over
``depthmap`` and ``camera_intrinsics`` instead, and ``ground_truth`` (``must3r_hip_gt_from_depth``, include/must3r_hip.h "ABI 21, additive",
csrc/train_data.hip) builds the three tensors for the whole batch in one launch.  The arithmetic is fixed (the header states it) so that
tests/train_data_ref.py reproduces it bit for bit on the CPU; it is dust3r's ``depthmap_to_absolute_camera_coordinates`` as restated from memory -- the
yardstick is the stated formula, not dust3r.

A portrait view of a batch stored landscape (dust3r's ``transpose_to_landscape``: ``true_shape`` = (W, H)) is stored with its axes swapped; the intrinsics stay
those of the true image and the kernel swaps the pixel coordinates instead of the data.  Which views those are is computed on the device from ``true_shape``
(``height > width``, the flags of ``train_encoder.patch_rows``): nothing is read back.

``SyntheticDepthScenes`` shows the scenes of ``synthetic.SyntheticScenes`` through depth, intrinsics and pose, for tests and scripts/bench_train_data.py.

Crop, resize and colour augmentation of raw frames into this depth form are ``train_augment``'s.  Not built: the dataset classes and samplers.  CPU tensors
raise in ``ground_truth``.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._train_common import _dev, _ptr, _stream

GT_KEYS = ("pts3d", "valid_mask", "sky_mask", "camera_pose", "is_metric_scale", "true_shape", "memory_num_views")


def gt_from_depth(depth, K, c2w, transposed=None, depth_scale=None, want=(True, True, True), count=False):
    """``must3r_hip_gt_from_depth`` on ``V`` views: depth ``[V, Hs, Ws]`` fp32 or uint16 (then ``depth_scale`` fp32 ``[V, 2]``: (div, mul)), K fp32
    ``[V, 3, 3]``, c2w fp32 ``[V, 4, 4]``, ``transposed`` int32 ``[V]`` or ``None`` -> ``(pts3d fp32 [V, Hs, Ws, 3], valid u8 [V, Hs, Ws], sky u8, n_valid
    int32 [V])``, ``None`` where ``want`` / ``count`` say so."""
    _dev(depth, "gt_from_depth: depth")
    if depth.ndim != 3 or depth.numel() == 0 or depth.dtype not in (torch.float32, torch.uint16):
        raise ValueError(f"gt_from_depth: depth of shape {tuple(depth.shape)} and dtype {depth.dtype}, expected fp32 or uint16 [V, Hs, Ws]")
    V, Hs, Ws = (int(s) for s in depth.shape)
    dev, u16 = depth.device, depth.dtype == torch.uint16
    if not any(want) and not count:
        return None, None, None, None

    def f32(t, shape, what):
        _dev(t, f"gt_from_depth: {what}")
        if tuple(t.shape) != shape:
            raise ValueError(f"gt_from_depth: {what} of shape {tuple(t.shape)}, expected {shape}")
        return t.detach().to(torch.float32).contiguous()
    K, c2w = f32(K, (V, 3, 3), "K"), f32(c2w, (V, 4, 4), "c2w")
    if u16 != (depth_scale is not None):
        raise ValueError("gt_from_depth: depth_scale goes with uint16 depth, and with it alone")
    depth_scale = f32(depth_scale, (V, 2), "depth_scale") if u16 else None
    if transposed is not None:
        _dev(transposed, "gt_from_depth: transposed")
        if transposed.dtype != torch.int32 or tuple(transposed.shape) != (V,):
            raise ValueError(f"gt_from_depth: transposed of dtype {transposed.dtype} and shape {tuple(transposed.shape)}, expected int32 [{V}]")
        transposed = transposed.contiguous()
    depth = depth.detach().contiguous()
    pts3d = torch.empty((V, Hs, Ws, 3), dtype=torch.float32, device=dev) if want[0] else None
    valid = torch.empty((V, Hs, Ws), dtype=torch.uint8, device=dev) if want[1] else None
    sky = torch.empty((V, Hs, Ws), dtype=torch.uint8, device=dev) if want[2] else None
    n_valid = torch.empty((V,), dtype=torch.int32, device=dev) if count else None
    scratch = torch.empty((V * _lib.GT_VIEW_BLOCKS,), dtype=torch.int32, device=dev) if count else None
    a = _lib.GtArgs()
    for name, t in (("depth", depth), ("depth_scale", depth_scale), ("K", K), ("c2w", c2w), ("transposed", transposed), ("pts3d", pts3d), ("valid", valid),
                    ("sky", sky), ("n_valid", n_valid), ("scratch", scratch)):
        setattr(a, name, _ptr(t))
    a.scratch_bytes = 0 if scratch is None else scratch.numel() * 4
    a.V, a.Hs, a.Ws, a.depth_u16 = V, Hs, Ws, int(u16)
    a.stream = _stream(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().must3r_hip_gt_from_depth(C.byref(a)))
    return pts3d, valid, sky, n_valid


def portrait_flags(true_shape):
    """int32, the shape of ``true_shape`` without its last dimension, on its device: 1 where ``height > width`` (``train_encoder.patch_rows``' flags)."""
    return (true_shape[..., 0] > true_shape[..., 1]).to(torch.int32)


def _metric(is_metric_scale, B):
    """bool ``[B]`` on the host, where the criterion reads it"""
    if isinstance(is_metric_scale, torch.Tensor):
        return is_metric_scale.detach().to(torch.bool).cpu().reshape(-1).expand(B).clone() if is_metric_scale.numel() == 1 \
            else is_metric_scale.detach().to(torch.bool).cpu().reshape(B)
    return torch.full((B,), bool(is_metric_scale), dtype=torch.bool)


def ground_truth(depth, camera_intrinsics, camera_pose, true_shape, depth_scale=None, is_metric_scale=False, count=False):
    """The ground truth of a batch on the device: depth ``[B, n, Hs, Ws]`` (fp32; negative: sky, 0: invalid -- or uint16 with ``depth_scale`` (div, mul), any
    shape that expands to ``[B, n, 2]``), camera_intrinsics ``[B, n, 3, 3]`` of the true images, camera_pose ``[B, n, 4, 4]`` camera to world, true_shape
    ``[B, n, 2]`` (h, w) -> a dict of batched tensors: ``pts3d`` fp32 ``[B, n, Hs, Ws, 3]``, ``valid_mask`` and ``sky_mask`` bool ``[B, n, Hs, Ws]``,
    ``camera_pose``, ``true_shape`` (both on the device), ``is_metric_scale`` bool ``[B]`` ON THE HOST (the criterion branches on it there), and with
    ``count`` ``n_valid`` int32 ``[B, n]``, the pixels of positive depth (what the datasets' ``is_valid_check`` tests).  One launch; the portrait flags are
    computed from ``true_shape`` on the device and nothing is read back."""
    _dev(depth, "ground_truth: depth")
    if depth.ndim != 4:
        raise ValueError(f"ground_truth: depth of shape {tuple(depth.shape)}, expected [B, n, Hs, Ws]")
    B, n, Hs, Ws = (int(s) for s in depth.shape)
    dev, V = depth.device, B * n
    pose = camera_pose.to(dev, torch.float32)
    ts = true_shape.to(dev)
    if tuple(ts.shape) != (B, n, 2):
        raise ValueError(f"ground_truth: true_shape of shape {tuple(ts.shape)}, expected {(B, n, 2)}")
    if depth_scale is not None:
        depth_scale = torch.as_tensor(depth_scale, dtype=torch.float32).to(dev).expand(B, n, 2).reshape(V, 2)
    pts3d, valid, sky, n_valid = gt_from_depth(depth.reshape(V, Hs, Ws), camera_intrinsics.to(dev, torch.float32).reshape(V, 3, 3), pose.reshape(V, 4, 4),
                                               portrait_flags(ts).reshape(V), depth_scale, count=count)
    out = dict(pts3d=pts3d.view(B, n, Hs, Ws, 3), valid_mask=valid.view(torch.bool).view(B, n, Hs, Ws), sky_mask=sky.view(torch.bool).view(B, n, Hs, Ws),
               camera_pose=pose.reshape(B, n, 4, 4), true_shape=ts, is_metric_scale=_metric(is_metric_scale, B))
    if count:
        out["n_valid"] = n_valid.view(B, n)
    return out


def img_norm(img):
    """dust3r's ``ImgNorm`` on a uint8 tensor ``[..., 3, H, W]``: ``ToTensor`` then ``Normalize(0.5, 0.5)``, ``(x / 255 - 0.5) / 0.5`` in fp32"""
    return img.to(torch.float32).div(255.0).sub(0.5).div(0.5)


def collate_views(batch, device):
    """The reference's batch -- a list of ``n`` view dicts of ``[B, ...]`` tensors -- as the loop needs it: ``(imgs [B, n, 3, H, W] fp32, true_shape [B, n, 2],
    gt)``, both tensors on ``device``.  ``img`` may be uint8 ``[B, 3, H, W]`` (normalised on the device, ``img_norm``: a quarter of the upload) or fp32 as
    the reference's loaders give it.

    A batch whose views carry ``pts3d`` passes through: ``gt`` is ``batch``, unchanged.  A batch whose views carry ``depthmap`` (fp32, or uint16 with a
    ``depth_scale`` entry ``[B, 2]``) and ``camera_intrinsics`` in their place gets ``gt`` from ``ground_truth``: a list of ``n`` dicts with the keys
    ``GT_KEYS``, whose tensors are views of the batched ones (``is_metric_scale`` and ``memory_num_views`` are the loader's host tensors)."""
    if not isinstance(batch, (list, tuple)) or not batch:
        raise ValueError("collate_views: batch is a list of view dicts")
    imgs = torch.stack([b["img"] for b in batch], dim=1).to(device)
    if imgs.ndim != 5 or int(imgs.shape[2]) != 3:
        raise ValueError(f"collate_views: images of shape {tuple(imgs.shape)}, expected n views of [B, 3, H, W]")
    if imgs.dtype == torch.uint8:
        imgs = img_norm(imgs)
    elif imgs.dtype != torch.float32:
        raise ValueError(f"collate_views: images of dtype {imgs.dtype}, expected uint8 or float32")
    true_shape = torch.stack([b["true_shape"] for b in batch], dim=1).to(device)
    if "pts3d" in batch[0]:
        return imgs, true_shape, batch
    for key in ("depthmap", "camera_intrinsics", "camera_pose"):
        if any(key not in b for b in batch):
            raise KeyError(f"collate_views: a view without pts3d needs {key!r}")
    depth = torch.stack([b["depthmap"] for b in batch], dim=1).to(device)
    scale = torch.stack([b["depth_scale"] for b in batch], dim=1) if "depth_scale" in batch[0] else None
    G = ground_truth(depth, torch.stack([b["camera_intrinsics"] for b in batch], dim=1), torch.stack([b["camera_pose"] for b in batch], dim=1),
                     true_shape, depth_scale=scale, is_metric_scale=batch[0].get("is_metric_scale", False))
    B = int(imgs.shape[0])
    gt = []
    for i, b in enumerate(batch):
        gt.append(dict(pts3d=G["pts3d"][:, i], valid_mask=G["valid_mask"][:, i], sky_mask=G["sky_mask"][:, i], camera_pose=G["camera_pose"][:, i],
                       is_metric_scale=_metric(b["is_metric_scale"], B) if "is_metric_scale" in b else G["is_metric_scale"],
                       true_shape=true_shape[:, i], memory_num_views=b.get("memory_num_views", torch.full((B,), len(batch), dtype=torch.int64))))
    return imgs, true_shape, gt


class SyntheticDepthScenes:
    """The scenes of ``synthetic.SyntheticScenes(n_scenes, n_views, H, W, seed, invalid_frac, focal)`` -- the same draws of the same generator, hence the same
    images, poses, depths and masks -- shown through depth, intrinsics and pose.  ``dataset[i]`` is a list of ``n_views`` dicts: ``img`` fp32 ``[3, H, W]`` in
    [-1, 1] (``uint8_img``: uint8, the image ``img_norm`` maps back to within 1/255), ``true_shape`` int32 ``[2]``, ``camera_pose`` fp32 ``[4, 4]``,
    ``camera_intrinsics`` fp32 ``[3, 3]``, ``depthmap`` fp32 ``[H, W]`` (0 where invalid, -1 where sky), ``is_metric_scale`` and ``memory_num_views``.
    ``raw_depth``: ``depthmap`` is uint16, millimetres, with ``depth_scale`` = (1000, 1); that form has no sky (0 there as well).

    ``portrait_every = k > 0``: every k-th view (k - 1, 2 k - 1, ...) is a portrait image stored transposed: the stored arrays are those of the landscape
    view, ``true_shape`` is (W, H) and the intrinsics are those of the true image of height W and width H, whose pixel (row, col) is the stored (col, row)."""

    def __init__(self, n_scenes, n_views, H, W, seed=0, portrait_every=0, invalid_frac=0.15, focal=None, memory_num_views=None, metric=True,
                 uint8_img=False, raw_depth=False):
        self.n_scenes, self.n_views, self.H, self.W, self.seed = int(n_scenes), int(n_views), int(H), int(W), int(seed)
        self.portrait_every, self.invalid_frac = int(portrait_every), float(invalid_frac)
        self.focal = float(focal) if focal is not None else 0.9 * max(H, W)
        self.memory_num_views = int(memory_num_views) if memory_num_views is not None else self.n_views
        self.metric, self.uint8_img, self.raw_depth = bool(metric), bool(uint8_img), bool(raw_depth)

    def set_epoch(self, epoch):
        pass

    def __len__(self):
        return self.n_scenes

    def is_portrait(self, v):
        return self.portrait_every > 0 and (v + 1) % self.portrait_every == 0

    def __getitem__(self, idx):
        if not 0 <= idx < self.n_scenes:
            raise IndexError(idx)
        g = torch.Generator().manual_seed(self.seed * 100003 + idx)        # synthetic.SyntheticScenes.__getitem__, draw for draw
        H, W, f = self.H, self.W, self.focal
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        phase = torch.rand((3,), generator=g) * 6.2831853
        views = []
        for v in range(self.n_views):
            ang = 0.08 * v + 0.02 * float(torch.randn((), generator=g))
            c, s = math.cos(ang), math.sin(ang)
            pose = torch.eye(4)
            pose[:3, :3] = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
            pose[:3, 3] = torch.tensor([0.25 * v, 0.03 * v, 0.0]) + 0.02 * torch.randn((3,), generator=g)
            z = 3.0 + 0.5 * torch.sin(xs / W * 5.0 + phase[0] + 0.3 * v) + 0.3 * torch.cos(ys / H * 4.0 + phase[1]) \
                + 0.02 * torch.randn((H, W), generator=g)
            valid = torch.rand((H, W), generator=g) >= self.invalid_frac
            sky = ~valid & (ys < H / 4)
            shade = ((z - 2.2) / 1.6).clamp(0, 1) * 2 - 1
            img = torch.stack((shade, torch.sin(xs / 7.0 + phase[2]) * 0.5, torch.cos(ys / 5.0) * 0.5), dim=0).contiguous()
            depth = torch.where(valid, z, torch.where(sky, torch.full_like(z, -1.0), torch.zeros_like(z)))
            portrait = self.is_portrait(v)
            K = torch.tensor([[f, 0.0, (H if portrait else W) / 2], [0.0, f, (W if portrait else H) / 2], [0.0, 0.0, 1.0]])
            view = dict(img=img, true_shape=torch.tensor([W, H] if portrait else [H, W], dtype=torch.int32), camera_pose=pose, camera_intrinsics=K,
                        depthmap=depth.contiguous(), is_metric_scale=torch.tensor(self.metric), memory_num_views=torch.tensor(self.memory_num_views))
            if self.uint8_img:
                view["img"] = ((img + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8)
            if self.raw_depth:
                view["depthmap"] = (depth.clamp(min=0.0) * 1000.0).round().clamp(0, 65535).to(torch.int32).to(torch.uint16)
                view["depth_scale"] = torch.tensor([1000.0, 1.0])
            views.append(view)
        return views
