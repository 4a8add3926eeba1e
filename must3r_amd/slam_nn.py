"""SLAM keyframe test on the GPU -- drop-in for must3r/slam/nns.py and ``get_overlap_score`` (must3r/slam/model.py:62-91).

Same class / function names and call signatures as the reference (``get_searcher``, ``Base_NN.add_pts`` / ``.query``,
``QuandrantSearcher`` [sic], ``get_overlap_score``), torch CUDA tensors in, numpy distances / a float score out like the
reference.  Instead of rebuilding a scipy KD-tree over all keyframe points after every keyframe (nns.py:47-50) and
querying it on 4 host threads (nns.py:56), the points stay in HBM and a query is an exact brute-force scan
(``must3r_hip_nn_query``); quadrant ids (slam/tools.py:9-31) come from ``must3r_hip_quadrant_ids``.  ``BVH_hip`` /
``BVHQuadrant_hip`` (``get_searcher("bvh-hip[-quadrant_xN]")``) give the same distances bit for bit from an index rebuilt on the
GPU after each change of the map (``must3r_hip_nn_index_*``), so that a query no longer scans the whole map.
``forward_must3r`` is the SLAM agent's forward wrapper (slam/model.py:22-59).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _check_pts(pts):
    if not isinstance(pts, torch.Tensor) or not pts.is_cuda:
        raise RuntimeError("must3r_amd.slam_nn: points must be CUDA tensors; the HIP path has no CPU fallback")
    return pts.reshape(-1, 3).float().contiguous()


def nn_distances(db, q):
    """Exact 1-NN Euclidean distances of q [n,3] to db [m,3] (cuda fp32) -> cuda fp32 [n]; +inf if db is empty."""
    q = _check_pts(q)
    out = torch.empty((q.shape[0],), dtype=torch.float32, device=q.device)
    n_db = 0 if db is None else int(db.shape[0])
    with torch.cuda.device(q.device):
        _lib.check(_lib.load().must3r_hip_nn_query(db.data_ptr() if n_db else None, n_db, q.data_ptr(), q.shape[0], out.data_ptr(), _lib.stream_ptr(q.device)))
    return out


def quadrant_ids(pts, cam_center, quadrant_divider):
    """slam/tools.py:9-31 on rays pts - cam_center -> cuda int32 [n]."""
    pts = _check_pts(pts)
    out = torch.empty((pts.shape[0],), dtype=torch.int32, device=pts.device)
    cc = (C.c_float * 3)(*[float(v) for v in torch.as_tensor(cam_center).reshape(3).tolist()])
    with torch.cuda.device(pts.device):
        _lib.check(_lib.load().must3r_hip_quadrant_ids(pts.data_ptr(), pts.shape[0], cc, int(quadrant_divider), out.data_ptr(), _lib.stream_ptr(pts.device)))
    return out


class Base_NN:
    """nns.py:22-38."""

    def __init__(self, subsamp=None):
        self.subsamp = subsamp

    def add_pts(self, pts, **kw):
        raise NotImplementedError("Overload this function for your needs")

    def query(self, pts, **kw):
        raise NotImplementedError("Overload this function for your needs")


class BruteForce_hip(Base_NN):
    """Stands in for KDTree_scipy (nns.py:40-57): same results (exact 1-NN), the database lives in HBM."""

    def __init__(self):
        super().__init__()
        self.all_points = None      # cuda fp32 [capacity, 3]; rows [0, n) valid
        self.n = 0

    def add_pts(self, pts, **kw):
        pts = _check_pts(pts)
        need = self.n + pts.shape[0]
        if self.all_points is None or need > self.all_points.shape[0]:
            grown = torch.empty((max(need, 2 * (0 if self.all_points is None else self.all_points.shape[0])), 3), dtype=torch.float32,
                                device=pts.device)
            if self.n:
                grown[:self.n] = self.all_points[:self.n]
            self.all_points = grown
        self.all_points[self.n:need] = pts
        self.n = need

    def query_device(self, pts, **kw):
        return nn_distances(None if self.n == 0 else self.all_points[:self.n], pts)

    def query(self, pts, **kw):
        return self.query_device(pts).double().cpu().numpy()


KDTree_scipy = BruteForce_hip   # the reference's name, for callers that construct it directly


class QuandrantSearcher(Base_NN):
    """nns.py:60-92 (spelling as in the reference): one search structure per view-direction quadrant."""

    def __init__(self, method):
        super().__init__()
        self.quadrant_divider = int(method.split("quadrant_x")[-1].split("-")[0])
        self.search_structs = [BruteForce_hip() for _ in range(2 * self.quadrant_divider ** 2)]

    def add_pts(self, pts, cam_center, **kw):
        pts = _check_pts(pts)
        qid = quadrant_ids(pts, cam_center, self.quadrant_divider)
        for quad in torch.unique(qid).tolist():
            self.search_structs[quad].add_pts(pts[qid == quad])

    def query_device(self, pts, cam_center, **kw):
        pts = _check_pts(pts)
        qid = quadrant_ids(pts, cam_center, self.quadrant_divider)
        dists = torch.zeros((pts.shape[0],), dtype=torch.float32, device=pts.device)
        for quad in torch.unique(qid).tolist():
            idx = qid == quad
            dists[idx] = self.search_structs[quad].query_device(pts[idx])
        return dists

    def query(self, pts, cam_center, **kw):
        return self.query_device(pts, cam_center).double().cpu().numpy()


class BVH_hip(Base_NN):
    """Exact 1-NN over a growing map through the GPU index (include/must3r_hip.h ABI 12): the distances of ``BruteForce_hip``
    (``quadrant_divider`` 0) or of ``QuandrantSearcher`` (``quadrant_divider`` N), bit for bit.  ``add_pts`` appends the points and
    their quadrant ids (from the batch's ``cam_center``) to a device store that grows by doubling; the next query rebuilds the index
    once, then answers every query quadrant in one launch.  Host tensors and arrays are copied to the device first: the video
    driver hands the keyframe callbacks host results (``preserve_gpu_mem``), as the reference's does."""

    def __init__(self, quadrant_divider=0):
        super().__init__()
        self.quadrant_divider = int(quadrant_divider)
        self.all_points = None      # cuda fp32 [capacity, 3]; rows [0, n) valid
        self.quadrants = None       # cuda int32 [capacity] (quadrant_divider > 0)
        self.n = 0
        self.index = None           # cuda uint8, must3r_hip_nn_index_bytes(n, divider)
        self.dirty = False

    def _device_pts(self, pts):
        if not isinstance(pts, torch.Tensor):
            pts = torch.as_tensor(np.asarray(pts, dtype=np.float32))
        if not pts.is_cuda:
            pts = pts.to(self.all_points.device if self.all_points is not None else torch.device("cuda", torch.cuda.current_device()))
        return _check_pts(pts)

    def add_pts(self, pts, cam_center=None, **kw):
        pts = self._device_pts(pts)
        need = self.n + pts.shape[0]
        if self.all_points is None or need > self.all_points.shape[0]:
            cap = max(need, 2 * (0 if self.all_points is None else self.all_points.shape[0]))
            grown = torch.empty((cap, 3), dtype=torch.float32, device=pts.device)
            grown_q = torch.zeros((cap,), dtype=torch.int32, device=pts.device)
            if self.n:
                grown[:self.n] = self.all_points[:self.n]
                grown_q[:self.n] = self.quadrants[:self.n]
            self.all_points, self.quadrants = grown, grown_q
        self.all_points[self.n:need] = pts
        if self.quadrant_divider and need > self.n:
            self.quadrants[self.n:need] = quadrant_ids(pts, cam_center, self.quadrant_divider)
        self.n = need
        self.dirty = True

    def build(self):
        """(Re)build the index over the current map now (a query does it when the map changed)."""
        lib = _lib.load()
        dev = self.all_points.device if self.all_points is not None else torch.device("cuda", torch.cuda.current_device())
        self.index = torch.empty((lib.must3r_hip_nn_index_bytes(self.n, self.quadrant_divider),), dtype=torch.uint8, device=dev)
        scratch = torch.empty((max(1, lib.must3r_hip_nn_index_scratch_bytes(self.n)),), dtype=torch.uint8, device=dev)
        pts, qid = (self.all_points.data_ptr(), self.quadrants.data_ptr()) if self.n else (None, None)   # an empty map: an empty index
        with torch.cuda.device(dev):
            _lib.check(lib.must3r_hip_nn_index_build(pts, qid, self.n, self.quadrant_divider, self.index.data_ptr(), scratch.data_ptr(),
                                                     _lib.stream_ptr(dev)))
        self.dirty = False

    def query_device(self, pts, cam_center=None, **kw):
        pts = self._device_pts(pts)
        if self.n == 0:
            return torch.full((pts.shape[0],), float("inf"), dtype=torch.float32, device=pts.device)
        if self.dirty:
            self.build()
        out = torch.empty((pts.shape[0],), dtype=torch.float32, device=pts.device)
        cc = None
        if self.quadrant_divider:
            cc = (C.c_float * 3)(*[float(v) for v in torch.as_tensor(cam_center).reshape(3).tolist()])
        with torch.cuda.device(pts.device):
            _lib.check(_lib.load().must3r_hip_nn_index_query(self.index.data_ptr(), pts.data_ptr(), pts.shape[0], cc, self.quadrant_divider,
                                                             out.data_ptr(), _lib.stream_ptr(pts.device)))
        return out

    def query(self, pts, cam_center=None, **kw):
        return self.query_device(pts, cam_center=cam_center).double().cpu().numpy()


class BVHQuadrant_hip(BVH_hip):
    """The quadrant form of ``BVH_hip`` for a method string 'bvh-hip-quadrant_xN' (``QuandrantSearcher``'s distances, one index)."""

    def __init__(self, method):
        super().__init__(int(method.split("quadrant_x")[-1].split("-")[0]))


def get_searcher(method, isquadrant=False):
    """nns.py:9-19; the reference's method strings ('kdtree-scipy', 'kdtree-scipy-quadrant_x2', 'none') are accepted, and
    'bvh-hip' / 'bvh-hip-quadrant_xN' select the GPU index (``BVH_hip`` / ``BVHQuadrant_hip``)."""
    if method.startswith("bvh-hip"):
        return BVHQuadrant_hip(method) if "quadrant_x" in method and not isquadrant else BVH_hip()
    if "quadrant_x" in method and not isquadrant:
        return QuandrantSearcher(method)
    if "kdtree-scipy" in method or "bruteforce-hip" in method:
        return BruteForce_hip()
    if method == "none":
        return None
    raise ValueError(f"Unknown searcher method {method}")


def get_overlap_score(res, overlap_tree, cam_center, mode="nn", kf_x_subsamp=None, min_conf_keyframe=1.5, percentile=70, eps=1e-9):
    """slam/model.py:62-91.  ``res`` holds CUDA tensors (the dict ``postprocess`` returns, with the leading [1,1] dims)."""
    outscore = 0.0
    if mode == "meanconf":
        return res["conf"].mean()
    if mode == "medianconf":
        return res["conf"].median()
    if "nn" not in mode:
        raise ValueError(f"Unknown overlap score method {mode}")
    pts3d = res["pts3d"][0, 0, ::kf_x_subsamp, ::kf_x_subsamp] if kf_x_subsamp else res["pts3d"]
    msk = res["conf"][0, 0, ::kf_x_subsamp, ::kf_x_subsamp] if kf_x_subsamp else res["conf"]
    msk = msk > min_conf_keyframe
    if msk.sum() > 0:
        dists = np.array(overlap_tree.query(pts3d[msk], cam_center=cam_center), dtype=np.float64)
        if "norm" in mode:
            depths = res["pts3d_local"][0, 0, ::kf_x_subsamp, ::kf_x_subsamp, -1]
            dists /= depths[msk].cpu().numpy() + eps
        dists[np.isposinf(dists)] = np.finfo(dists.dtype).max   # unseen quadrant (slam/model.py:87-88)
        outscore = np.percentile(dists, percentile)
    return outscore


def choose_keyframe_from_overlap(overlap_score, thr, overlap_mode):
    """slam/model.py:123-128."""
    if "nn" in overlap_mode:
        return overlap_score > thr
    return overlap_score < thr


@torch.no_grad()
def forward_must3r(model, input_views, memory, render=False, device='cuda:0', postprocess=None):
    """slam/model.py:22-59: encode every view (dict with ``img`` [1,3,H,W] and ``true_shape`` [1,2], dust3r's view layout) on its own,
    ONE decoder call over the list (one group per view: views may differ in aspect ratio), activation per view.
    Returns ``(list of {pts3d, pts3d_local, conf} with a leading [1, 1] batch, new_memory)``.

    The (H, W) pairs stay on the host (both modules read them as host integers: no device round trip per view) and the
    allocator cache is left alone (the reference empties it after every frame, :50).  ``postprocess`` defaults to the
    fused native activation (``must3r_amd.engine.postprocess``)."""
    if postprocess is None:
        from .engine import postprocess
    from .model import get_pointmaps_activation
    encoder, decoder = model
    xs, poss, shapes = [], [], []
    for view in input_views:
        shape = view['true_shape']
        shape = (shape.cpu() if torch.is_tensor(shape) else torch.as_tensor(shape))[None]   # :31, kept on the host
        x, pos = encoder(view['img'].to(device), shape.view(-1, 2))
        xs.append(x[None])
        poss.append(pos[None])
        shapes.append(shape)
    new_memory, preds = decoder(xs, poss, shapes, memory, render=render)
    activation = get_pointmaps_activation(decoder, verbose=False)
    return [postprocess(pred, pointmaps_activation=activation) for pred in preds], new_memory
