"""The online SLAM agent -- must3r/slam/model.py (``SLAM_MUSt3R``, ``MUSt3R_Agent``, ``postproc_pred``, ``get_camera_pose``, ``mean_focal``,
``build_intr``, ``get_map``, ``prep_imgs``), slam/tools.py (the two smoothing functions) and the headless part of slam/slam.py -- with the per-frame
step between two decoder calls as device work.

Per frame: ``image.preproc_frame``, ``slam_nn.forward_must3r`` with the raw head output kept on the device, then ``must3r_hip_slam_pose`` (activation,
Weiszfeld focal, rectified registration, the agent's running focal sums) and ``must3r_hip_slam_keyframe`` (mask, compaction, index walk, percentile,
conf median and mean) are enqueued without a host read (csrc/slam.hip, include/must3r_hip.h), and ONE record of 32 doubles is copied into pinned memory
and waited for (``SLAM_MUSt3R.read_record``).  The keyframe decision is taken on the host from that record; on a keyframe the compacted points are
appended to the map with the camera centre of the record, which needs no further read.  The index is rebuilt after each keyframe, as ``BVH_hip`` does.

What differs from the reference, on purpose:
* the searcher is the GPU index: the reference's method strings select it too ('kdtree-scipy' -> ``BVH_hip``, 'kdtree-scipy-quadrant_xN' and
  'bvh-hip-quadrant_xN' -> ``BVHQuadrant_hip``; same distances, bit for bit, as the brute-force classes ``get_searcher`` gives for them);
* ``seq_focals`` is a ``FocalState``: the sums of ``mean_focal`` live on the device in fp64 (the reference: fp32 numpy), the per-frame (f, c) log is read
  back lazily, once, by ``get_true_focal`` / ``write_all_poses``;
* the returned ``focal`` is a Python float, ``cam_center`` a tuple of host floats, ``all_poses`` holds host 4 x 4 arrays (from the record);
* cv2 and open3d are not used: ``python -m must3r_amd.slam`` reads image folders and file lists with Pillow and refuses ``cam:N``, video files and ``--gui``.
"""
import argparse
import ctypes as C
import os
import pickle as pkl
import time

import numpy as np
import torch

from . import _lib
from .image import ImgNorm, preproc_frame
from .model import ActivationType, get_pointmaps_activation
from .slam_nn import BVH_hip, BVHQuadrant_hip, forward_must3r  # noqa: F401

REC = dict(n_sel=0, below=1, above=2, score=3, conf_median=4, conf_mean=5, focal=6, mean_focal=7, cam_center=slice(8, 11), c2w=slice(11, 27), virtual_index=27)


# -------------------------------------------------------------------------------------------------------------------------------------
# slam/tools.py:34-63
# -------------------------------------------------------------------------------------------------------------------------------------
def laplacian_smoothing(trajectory, alpha=0.5, iterations=10):
    smoothed_trajectory = trajectory.copy()
    N = len(trajectory)
    for _ in range(iterations):
        for i in range(1, N - 1):  # Exclude endpoints from smoothing
            smoothed_trajectory[i] = (1 - alpha) * smoothed_trajectory[i] + (alpha / 2) * (smoothed_trajectory[i - 1] + smoothed_trajectory[i + 1])
    return smoothed_trajectory


def laplacian_smoothing_with_confidence(trajectory, confidence, alpha=0.5, iterations=10):
    smoothed_trajectory = trajectory.copy()
    N = len(trajectory)
    for _ in range(iterations):
        for i in range(1, N - 1):  # Exclude endpoints from smoothing
            weight_self = (1 - alpha) * confidence[i]
            weight_previous = alpha * (1 - confidence[i - 1]) / 2
            weight_next = alpha * (1 - confidence[i + 1]) / 2
            sumw = weight_self + weight_previous + weight_next
            weight_self /= sumw
            weight_previous /= sumw
            weight_next /= sumw
            smoothed_trajectory[i] = (weight_self * smoothed_trajectory[i] + weight_previous * smoothed_trajectory[i - 1] +
                                      weight_next * smoothed_trajectory[i + 1])
    return smoothed_trajectory


# -------------------------------------------------------------------------------------------------------------------------------------
# the native calls
# -------------------------------------------------------------------------------------------------------------------------------------
def _dev(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"must3r_amd.slam: {what} must be a CUDA tensor; the HIP path has no CPU fallback")
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


class FocalState:
    """The agent's ``seq_focals`` on the device: fp64 (sum f c, sum c, n, sum f c / sum c) and the per-frame (f_i, c_i) log, which grows by doubling.
    ``to_orig`` stays a host list.  Nothing is allocated before the first frame."""

    def __init__(self):
        self.state = None       # cuda fp64 [4]
        self.log = None         # cuda fp64 [cap, 2]
        self.n = 0              # frames appended since the reset (the device's n, counted on the host as well)
        self.to_orig = []
        self._host = None       # (n, f, c) of the last read

    def reset(self):
        if self.state is not None:
            self.state.zero_()
        self.n = 0
        self.to_orig = []
        self._host = None

    def prepare(self, device):
        """buffers for one more frame; no host read"""
        if self.state is None:
            self.state = torch.zeros((_lib.SLAM_FOCAL_STATE_DOUBLES,), dtype=torch.float64, device=device)
        if self.log is None or self.n >= self.log.shape[0]:
            grown = torch.zeros((max(64, 2 * (0 if self.log is None else self.log.shape[0])), 2), dtype=torch.float64, device=device)
            if self.log is not None:
                grown[:self.log.shape[0]] = self.log
            self.log = grown

    def read(self):
        """-> (f [n], c [n]) fp64 numpy; one device read per change of n"""
        if self._host is None or self._host[0] != self.n:
            fc = self.log[:self.n].cpu().numpy() if self.n else np.zeros((0, 2))
            self._host = (self.n, fc[:, 0].copy(), fc[:, 1].copy())
        return self._host[1], self._host[2]

    def __len__(self):
        return self.n


def slam_pose(pointmaps, activation=ActivationType.NORM_EXP, seq_focals=None, is_first_frame=False, use_seq_focal=True, update_focal=False):
    """``must3r_hip_slam_pose``: raw head output [B, H, W, 7] (cuda fp32) -> dict(pts3d, pts3d_local (z rectified), conf, focal [B], c2w [B, 4, 4]).
    ``seq_focals``: a ``FocalState`` or None."""
    if isinstance(activation, str):
        activation = ActivationType(activation)
    pm = _dev(pointmaps, "pointmaps").float().contiguous()
    if pm.dim() != 4 or pm.shape[-1] != 7:
        raise ValueError(f"must3r_amd.slam.slam_pose: expected raw head output [B, H, W, 7], got {tuple(pm.shape)}")
    B, H, W = (int(s) for s in pm.shape[:3])
    dev = pm.device
    lib = _lib.load()
    out = {"pts3d": torch.empty((B, H, W, 3), dtype=torch.float32, device=dev), "pts3d_local": torch.empty((B, H, W, 3), dtype=torch.float32, device=dev),
           "conf": torch.empty((B, H, W), dtype=torch.float32, device=dev), "focal": torch.empty((B,), dtype=torch.float32, device=dev),
           "c2w": torch.empty((B, 4, 4), dtype=torch.float32, device=dev)}
    a = _lib.SlamPoseArgs()
    a.pm, a.pts3d, a.pts3d_local, a.conf, a.focal, a.c2w = (t.data_ptr() for t in (pm, out["pts3d"], out["pts3d_local"], out["conf"], out["focal"], out["c2w"]))
    if seq_focals is not None:
        if update_focal:
            seq_focals.prepare(dev)
        a.focal_state = _ptr(seq_focals.state)
        a.focal_log = _ptr(seq_focals.log)
        a.focal_log_cap = 0 if seq_focals.log is None else int(seq_focals.log.shape[0])
    a.B, a.H, a.W = B, H, W
    a.activation = _lib.ACT_LINEAR if activation == ActivationType.LINEAR else _lib.ACT_NORM_EXP
    a.is_first, a.use_seq_focal, a.update_focal = int(bool(is_first_frame)), int(bool(use_seq_focal)), int(bool(update_focal))
    with torch.cuda.device(dev):
        a.scratch_bytes = lib.must3r_hip_slam_pose_scratch_bytes(B, H, W)
        scratch = torch.empty((max(1, a.scratch_bytes),), dtype=torch.uint8, device=dev)
        a.scratch = scratch.data_ptr()
        a.stream = _lib.stream_ptr(dev)
        _lib.check(lib.must3r_hip_slam_pose(C.byref(a)))
    if update_focal:
        seq_focals.n += 1
    return out


def mode_bits(overlap_mode):
    """the reference's ``overlap_mode`` strings (slam/model.py:72-90) -> MUST3R_SLAM_MODE_*"""
    if overlap_mode == "meanconf":
        return _lib.SLAM_MODE_MEANCONF
    if overlap_mode == "medianconf":
        return _lib.SLAM_MODE_MEDIANCONF
    if "nn" in overlap_mode:
        return _lib.SLAM_MODE_NN | (_lib.SLAM_MODE_NORM if "norm" in overlap_mode else 0)
    raise ValueError(f"Unknown overlap score method {overlap_mode}")


def candidates(H, W, subsamp):
    s = subsamp if subsamp and subsamp > 1 else 1
    return ((H + s - 1) // s) * ((W + s - 1) // s)


def slam_keyframe(pts3d, pts3d_local, conf, c2w, overlap_tree=None, mode="nn-norm", kf_x_subsamp=None, min_conf_keyframe=1.5, percentile=70.0,
                  focal=None, seq_focals=None, want_dist=False):
    """``must3r_hip_slam_keyframe`` on one frame's [H, W, 3] / [H, W] maps and its c2w [4, 4] on the device -> (sel [candidates, 3], record (cuda fp64 [32]),
    dist [candidates] or None).  ``overlap_tree``: a ``BVH_hip`` (rebuilt here when the map changed) or None.  Nothing is read back."""
    p3, pl, cf = (_dev(t, n).float().contiguous() for t, n in ((pts3d, "pts3d"), (pts3d_local, "pts3d_local"), (conf, "conf")))
    H, W = (int(s) for s in cf.shape[-2:])
    dev = cf.device
    lib = _lib.load()
    sub = int(kf_x_subsamp) if kf_x_subsamp else 0
    n_cand = candidates(H, W, sub)
    sel = torch.empty((n_cand, 3), dtype=torch.float32, device=dev)
    dist = torch.empty((n_cand,), dtype=torch.float32, device=dev) if want_dist else None
    record = torch.empty((_lib.SLAM_RECORD_DOUBLES,), dtype=torch.float64, device=dev)
    a = _lib.SlamKeyframeArgs()
    a.pts3d, a.pts3d_local, a.conf, a.c2w = p3.data_ptr(), pl.data_ptr(), cf.data_ptr(), _dev(c2w, "c2w").float().contiguous().data_ptr()
    a.focal = _ptr(focal)
    a.focal_state = None if seq_focals is None else _ptr(seq_focals.state)
    a.divider = 0
    if overlap_tree is not None:
        if not isinstance(overlap_tree, BVH_hip):
            raise TypeError("must3r_amd.slam: the device keyframe test walks the GPU index; the searcher must be a BVH_hip / BVHQuadrant_hip")
        a.divider = overlap_tree.quadrant_divider
        if overlap_tree.n:
            if overlap_tree.dirty:
                overlap_tree.build()
            a.index = overlap_tree.index.data_ptr()
    a.sel, a.dist, a.record = sel.data_ptr(), _ptr(dist), record.data_ptr()
    a.quantile, a.min_conf = float(percentile) / 100.0, float(min_conf_keyframe)
    a.H, a.W, a.subsamp, a.mode = H, W, sub, mode_bits(mode) if isinstance(mode, str) else int(mode)
    with torch.cuda.device(dev):
        a.scratch_bytes = lib.must3r_hip_slam_keyframe_scratch_bytes(H, W, sub)
        scratch = torch.empty((max(1, a.scratch_bytes),), dtype=torch.uint8, device=dev)
        a.scratch = scratch.data_ptr()
        a.stream = _lib.stream_ptr(dev)
        _lib.check(lib.must3r_hip_slam_keyframe(C.byref(a)))
    return sel, record, dist


def read_record(record):
    """The one host read of a frame: the record into pinned memory on the current stream, one wait -> fp64 numpy [32]."""
    host = torch.empty(record.shape, dtype=record.dtype, pin_memory=True)
    host.copy_(record, non_blocking=True)
    torch.cuda.current_stream(record.device).synchronize()
    return host.numpy().copy()


def rigid_inverse(c2w):
    """w2c of a rigid c2w [..., 4, 4] in closed form (R^T, -R^T T), on c2w's device."""
    Rt, T = c2w[..., :3, :3].transpose(-1, -2), c2w[..., :3, 3:]
    # the last row of a rigid transform is its own inverse's; concatenation, because assigning a Python scalar into an element synchronises
    return torch.cat((torch.cat((Rt, -(Rt @ T)), -1), c2w[..., 3:, :]), -2)


# -------------------------------------------------------------------------------------------------------------------------------------
# slam/model.py
# -------------------------------------------------------------------------------------------------------------------------------------
def prep_imgs(cimg, img_mean, img_std):
    """slam/model.py:94-96.  Equal means and equal stds (ImgNorm) are applied as scalars: no upload per frame."""
    cimg = cimg.permute(0, 2, 3, 1)  # [B, H, W, 3] color is float3 \\in [0,1]
    if len(set(img_std)) == 1 and len(set(img_mean)) == 1:
        return cimg * float(img_std[0]) + float(img_mean[0])
    return (cimg * torch.tensor(img_std, device=cimg.device)) + torch.tensor(img_mean, device=cimg.device)


def choose_keyframe_from_overlap(overlap_score, thr, overlap_mode):
    """slam/model.py:123-128."""
    if 'nn' in overlap_mode:
        return overlap_score > thr
    return overlap_score < thr


def mean_focal(seq_focals):
    """slam/model.py:131-137: the conf-weighted mean of the sequence's focals, or None.  ``seq_focals``: the reference's dict of lists, or a
    ``FocalState`` (its log is read from the device, once per change)."""
    if isinstance(seq_focals, FocalState):
        f, c = seq_focals.read()
    else:
        f, c = np.array(seq_focals['f'], dtype=np.float64), np.array(seq_focals['conf'], dtype=np.float64)
    out = None
    if len(f):
        out = (f * c / c.sum()).sum()
    return out


def build_intr(focal, W, H, device, dtype):
    """slam/model.py:140-144."""
    out = torch.eye(3, device=device, dtype=dtype)
    out[0, 0] = out[1, 1] = float(focal)
    out[:2, -1] = torch.tensor([W / 2, H / 2], device=device, dtype=dtype)
    return out


def get_camera_pose(res, seq_focal, HW, is_first_frame=False, rectify=True):
    """slam/model.py:147-172 through ``must3r_hip_slam_pose``.  ``res['pointmaps']`` is the raw head output [1, B, H, W, 7] (the native call activates,
    estimates and registers in one pass); ``seq_focal`` is a ``FocalState``, a number, or None.  As in the reference, ``res['pts3d_local']`` holds the
    RECTIFIED depths afterwards (``pts3d``, ``pts3d_local`` and ``conf`` of ``res`` are set from the same call).  -> (c2w [B, 4, 4], focal [B])"""
    if 'pointmaps' not in res:
        raise RuntimeError("must3r_amd.slam.get_camera_pose: res['pointmaps'] (the raw head output) is needed; there is no path from activated maps")
    pm = res['pointmaps']
    H, W = (int(v) for v in HW)
    if tuple(pm.shape[-3:]) != (H, W, 7):
        raise ValueError(f"must3r_amd.slam.get_camera_pose: pointmaps {tuple(pm.shape)} against HW {(H, W)}")
    state = seq_focal
    if seq_focal is not None and not isinstance(seq_focal, FocalState):
        state = FocalState()
        state.state = torch.tensor([float(seq_focal), 1.0, 1.0, float(seq_focal)], dtype=torch.float64, device=pm.device)
    out = slam_pose(pm.reshape(-1, H, W, 7), res.get('activation', ActivationType.NORM_EXP), state, is_first_frame, use_seq_focal=rectify and state is not None)
    lead = tuple(pm.shape[:-3])
    for k in ('pts3d', 'pts3d_local', 'conf'):
        res[k] = out[k].reshape(*lead, *out[k].shape[1:])
    return out['c2w'], out['focal']


def get_map(ptscolsconfs, confthr):
    """slam/model.py:175-182."""
    allpts = []
    allcols = []
    for pts, cols, confs in ptscolsconfs:
        msk = confs > confthr
        allpts.append(pts[msk])
        allcols.append(cols[0, 0, msk])
    return torch.cat(allpts), torch.cat(allcols)


def postproc_pred(img, res, is_first_frame, seq_focals, fixed_focal=True, overlap_mode='nn-norm', overlap_tree=None, kf_x_subsamp=None,
                  keyframe_overlap_thr=.15, min_conf_keyframe=1.5, overlap_percentile=70, img_mean=[0.5, 0.5, 0.5], img_std=[0.5, 0.5, 0.5],
                  read=read_record):
    """slam/model.py:185-248 for one frame: ``res['pointmaps']`` is its raw head output [1, 1, H, W, 7], ``seq_focals`` the agent's ``FocalState``, which
    this call also advances (the reference's ``MUSt3R_Agent.update`` appends after the call; the sums are read before they are advanced either way).
    Everything is enqueued, then ``read`` is called once.  The returned depth is the RECTIFIED one, as in the reference.  ``res['record']`` keeps the
    frame's record (fp64 numpy, ``REC`` names its fields) and ``res['overlap_score']`` the score."""
    pm = res['pointmaps']
    assert pm.shape[0] == 1 and pm.shape[1] == 1, "Need to implement batching if ever needed, frames should come 1 by 1 here."
    H, W = (int(v) for v in img['true_shape'][0])
    out = slam_pose(pm.reshape(1, H, W, 7), res.get('activation', ActivationType.NORM_EXP), seq_focals, is_first_frame, use_seq_focal=fixed_focal,
                    update_focal=True)
    for k in ('pts3d', 'pts3d_local', 'conf'):
        res[k] = out[k][None]
    c2w = out['c2w'][0]
    sel, record, _ = slam_keyframe(out['pts3d'][0], out['pts3d_local'][0], out['conf'][0], c2w, overlap_tree, overlap_mode, kf_x_subsamp,
                                   min_conf_keyframe, overlap_percentile, out['focal'], seq_focals)
    cols = prep_imgs(img['img'], img_mean=img_mean, img_std=img_std)[None]
    w2c = rigid_inverse(c2w)
    rec = read(record)
    score, n_sel = float(rec[REC['score']]), int(rec[REC['n_sel']])
    res['record'], res['overlap_score'] = rec, score
    # the median comparison in fp32, as torch makes it
    iskeyframe = bool(is_first_frame or (choose_keyframe_from_overlap(score, keyframe_overlap_thr, overlap_mode)
                                         and np.float32(rec[REC['conf_median']]) > np.float32(min_conf_keyframe)))
    cam_center = tuple(float(v) for v in rec[REC['cam_center']])
    return (sel[:n_sel], out['pts3d'][0], cols.to(torch.float32), out['pts3d_local'][0, ..., -1], out['conf'][0], out['focal'], w2c, cam_center, iskeyframe)


class MUSt3R_Agent():
    """
    Manage focal length, and smoothing operations for each agent independently
    """

    def __init__(self, fixed_focal=True, smooth_focal_changes=False, img_mean=[0.5, 0.5, 0.5], img_std=[0.5, 0.5, 0.5]):
        assert fixed_focal or not smooth_focal_changes, "TODO maybe: online focal smoothing when varying focals"
        self.fixed_focal = fixed_focal
        self.smooth_focal_changes = smooth_focal_changes
        self.img_mean = img_mean
        self.img_std = img_std
        self.seq_focals = FocalState()
        self.reset()

    def reset(self):
        self.seq_focals.reset()

    def get_true_focal(self):
        out = None
        if len(self.seq_focals) != 0:
            to_orig = self.seq_focals.to_orig
            if self.fixed_focal:
                assert np.all(np.array(to_orig) == to_orig[0]), "To orig should be constant for a single true focal"
                out = mean_focal(self.seq_focals) * to_orig[0]
            else:
                out = [ff * tt for ff, tt in zip(self.seq_focals.read()[0], to_orig)]
        return out

    @torch.no_grad()
    def update(self, inp, pred, is_first_frame, overlap_mode, overlap_tree, kf_x_subsamp, keyframe_overlap_thr, min_conf_keyframe, overlap_percentile,
               to_orig_focal, read=read_record):
        selpts3d, pts3d, colors, depth, conf, focal, w2c, cam_center, iskeyframe = postproc_pred(
            img=inp, res=pred, is_first_frame=is_first_frame, seq_focals=self.seq_focals, fixed_focal=self.fixed_focal, overlap_mode=overlap_mode,
            overlap_tree=overlap_tree, kf_x_subsamp=kf_x_subsamp, keyframe_overlap_thr=keyframe_overlap_thr, min_conf_keyframe=min_conf_keyframe,
            overlap_percentile=overlap_percentile, img_mean=self.img_mean, img_std=self.img_std, read=read)
        self.seq_focals.to_orig.append(to_orig_focal)
        rec = pred['record']
        outfocal = float(rec[REC['mean_focal']] if self.fixed_focal else rec[REC['focal']])
        return selpts3d, pts3d, colors, depth, conf, outfocal, w2c, cam_center, iskeyframe


def _raw_pred(pred, pointmaps_activation=ActivationType.NORM_EXP):
    """``forward_must3r``'s postprocess hook: keep the raw head output on the device (the pose call activates it)"""
    return {'pointmaps': pred, 'activation': pointmaps_activation}


def slam_searcher(method):
    """The searcher behind a method string: the GPU index for the reference's strings and for 'bvh-hip[-quadrant_xN]'; 'none' -> None."""
    if method == "none":
        return None
    if not (method.startswith("bvh-hip") or "kdtree-scipy" in method or "bruteforce-hip" in method):
        raise ValueError(f"Unknown searcher method {method}")
    return BVHQuadrant_hip(method) if "quadrant_x" in method else BVH_hip()


class SLAM_MUSt3R():
    """
    Main memory manager, will take care of redistributing input images to respective agent, will gather agent's response and update memory accordingly
    You can save/load memory for/from other runs
    """

    def __init__(self, chkpt, res=512, searcher='bvh-hip-quadrant_x2', overlap_mode='nn-norm', kf_x_subsamp=4, keyframe_overlap_thr=.15,
                 min_conf_keyframe=1.5, overlap_percentile=70., rerender=False, fixed_focal=True, keep_memory=False, load_memory=None, num_agents=1,
                 device='cuda:0', num_init_frames=2):
        self.agents = [MUSt3R_Agent(fixed_focal) for _ in range(num_agents)]
        self.num_init_frames = num_init_frames
        self.res = res
        self.device = device
        self.transform = ImgNorm
        if isinstance(chkpt, (tuple, list)):
            self.model = tuple(chkpt)          # an (encoder, decoder) pair in place of a path
        else:
            from .model import load_model
            self.model = load_model(chkpt, device=device)
        self.searcher = searcher
        self.kf_x_subsamp = kf_x_subsamp
        self.keyframe_overlap_thr = keyframe_overlap_thr
        self.min_conf_keyframe = min_conf_keyframe
        self.overlap_percentile = overlap_percentile
        self.overlap_mode = overlap_mode
        self.rerender = rerender  # once sequence is processed, repredict everything from full memory
        self.keep_memory = keep_memory  # save latent_kf+pointmaps for export
        self.memory_memory = None
        self.memory_map = None
        self.memory_data = []
        self.memory_overlap_tree = None
        if load_memory is not None:
            self.load_memory(load_memory)
        self.reset()

    def reset(self):
        self.all_poses = []
        self.all_confs = []
        self.all_timestamps = []
        self.memory = self.memory_memory
        self.keyframe_pointmaps = self.memory_data
        self.keyframes = []
        if self.memory_overlap_tree is None:
            self.overlap_tree = slam_searcher(self.searcher if 'nn' in self.overlap_mode else 'none')
        else:
            self.overlap_tree = self.memory_overlap_tree
        self.all_images = []
        self.all_pts3d = None
        self.mem_was_loaded = self.memory_memory is not None  # reset to loaded memory
        for i in range(len(self.agents)):
            self.agents[i].reset()

    @property
    def num_mem_frames(self):
        return len(self.keyframes)

    def get_true_focals(self):
        return {agid: agent.get_true_focal() for agid, agent in enumerate(self.agents)}

    def write_all_poses(self, path, filtering_mode=None, filtering_steps=5, filtering_alpha=.5, **tolog):
        print(f"Writing full trajectory in {path}")
        all_poses = np.stack([p.cpu().numpy() if torch.is_tensor(p) else np.asarray(p) for p in self.all_poses]).astype(np.float32)
        timestamps = np.stack(self.all_timestamps).astype(int)
        conf = np.asarray([float(c) for c in self.all_confs], dtype=np.float32)
        focals = self.get_true_focals()
        if filtering_mode is not None:
            if 'laplacian' in filtering_mode:
                trajectory = all_poses[:, :3, -1]
                if 'conf' in filtering_mode:
                    conf_remap = (conf - conf.min()) / (conf.max() - conf.min())  # remap [1,inf] in between [0,1]
                    smoothed_trajectory = laplacian_smoothing_with_confidence(trajectory, conf_remap, alpha=filtering_alpha, iterations=filtering_steps)
                else:
                    smoothed_trajectory = laplacian_smoothing(trajectory, alpha=filtering_alpha, iterations=filtering_steps)
                all_poses[:, :3, -1] = smoothed_trajectory
            else:
                raise ValueError(f"Unknown filtering mode {filtering_mode}")
        np.savez(path, poses=all_poses, timestamps=timestamps, confs=conf, focal=focals, **tolog)

    def save_memory(self, output):
        """Pickles (memory, keyframe_pointmaps, overlap_tree) as the reference does.  The file holds this package's searcher (a ``BVH_hip``) and
        device tensors: it is read by ``load_memory`` here and is not readable by the reference."""
        mem = (self.memory, self.keyframe_pointmaps, self.overlap_tree)
        with open(output, 'wb') as f:
            pkl.dump(mem, f)

    def load_memory(self, mem_file):
        with open(mem_file, 'rb') as f:
            self.memory_memory, self.memory_data, self.memory_overlap_tree = pkl.load(f)
        self.memory = self.memory_memory
        self.keyframe_pointmaps = self.memory_data
        self.overlap_tree = self.memory_overlap_tree
        self.mem_was_loaded = True

    def fetch_memory_map(self, conf_thr):
        if self.mem_was_loaded:
            self.memory_map = get_map(self.memory_data, conf_thr)
            self.mem_was_loaded = False
        return self.memory_map

    # the three steps of a frame that touch the device: a test replaces them to drive the bookkeeping alone
    def preproc(self, img, frame_id):
        return preproc_frame(img, frame_id, res=self.res, transform=self.transform)

    def forward(self, views, memory, render=False):
        return forward_must3r(self.model, views, memory, render=render, device=self.device, postprocess=_raw_pred)

    def read_record(self, record):
        """every host read of the per-frame loop goes through here: one call per frame"""
        return read_record(record)

    def frame_step(self, agent, view, pred, is_first_frame, to_orig_focal):
        return agent.update(view, pred, is_first_frame, overlap_mode=self.overlap_mode, overlap_tree=self.overlap_tree, kf_x_subsamp=self.kf_x_subsamp,
                            keyframe_overlap_thr=self.keyframe_overlap_thr, min_conf_keyframe=self.min_conf_keyframe,
                            overlap_percentile=self.overlap_percentile, to_orig_focal=to_orig_focal, read=self.read_record) + (pred['record'],)

    @torch.no_grad()
    def rerender_all_frames(self, maxbs=64):
        assert len(self.agents) == 1, "Multiagent rerender to be managed (different focal lengths)"
        if self.rerender:
            B = len(self.all_images)
            all_pts3d, all_c2w = [], []
            for i in range(B // maxbs + 1):
                sel = self.all_images[slice(i * maxbs, (i + 1) * maxbs)]
                if sel == []:
                    continue
                all_imgs = {'img': torch.cat([im['img'] for im in sel]), 'true_shape': np.concatenate([im['true_shape'] for im in sel])}
                pred, _ = self.forward([all_imgs], self.memory, render=True)
                c2w, _ = get_camera_pose(pred[0], self.agents[0].seq_focals, HW=all_imgs['true_shape'][0], is_first_frame=False)
                all_pts3d.append(pred[0]['pts3d'].cpu())
                all_c2w.append(c2w)
            self.all_pts3d = torch.cat(all_pts3d, dim=1)
            self.all_poses = [cc for cc in torch.cat(all_c2w)]

    @torch.no_grad()
    def __call__(self, img, frame_id, cam_id, device_outputs=False):
        """slam/model.py:481-528.  -> (pts3d, colors, depth, conf, focal, w2c, HW, iskeyframe) of the LAST frame processed, pts3d and colors as numpy
        arrays, or, with ``device_outputs``, as the device tensors (no copy)."""
        query_view_prep, to_orig_focal = self.preproc(img, frame_id)

        if self.memory is not None and len(self.all_images) < self.num_init_frames:
            # we have not reached the correct initialization, reset memory
            other_init_images = self.all_images
            frame_ids = self.all_timestamps
            self.reset()
            self.all_images = other_init_images.copy()
        else:
            other_init_images = []
            frame_ids = []

        if self.rerender or (len(self.all_images) < self.num_init_frames):
            self.all_images.append(query_view_prep)

        query_images = other_init_images + [query_view_prep]
        frame_ids += [frame_id]
        preds, newmem = self.forward(query_images, self.memory)

        for query_view_prep, pred, frame_id in zip(query_images, preds, frame_ids):
            HW = query_view_prep['true_shape'][0]
            selpts3d, pts3d, colors, depth, conf, focal, w2c, cam_center, iskeyframe, rec = self.frame_step(
                self.agents[cam_id], query_view_prep, pred, self.memory is None, to_orig_focal)
            self.all_timestamps.append(frame_id)
            self.all_poses.append(np.asarray(rec[REC['c2w']], dtype=np.float32).reshape(4, 4))
            self.all_confs.append(np.float32(rec[REC['conf_mean']]))

            if iskeyframe:
                self.memory = newmem
                self.keyframes.append(frame_id)
                if self.overlap_tree is not None:
                    self.overlap_tree.add_pts(selpts3d, cam_center=cam_center)
                if self.keep_memory:
                    self.keyframe_pointmaps.append([pts3d.cpu(), colors.cpu(), conf.cpu()])

        if device_outputs:
            return pts3d, colors, depth, conf, focal, w2c, HW, iskeyframe
        return pts3d.cpu().numpy(), colors.cpu().numpy(), depth, conf, focal, w2c, HW, iskeyframe


# -------------------------------------------------------------------------------------------------------------------------------------
# headless slam/slam.py
# -------------------------------------------------------------------------------------------------------------------------------------
IMAGE_FORMATS = ['jpg', 'jpeg', 'jpe', 'png', 'tiff', 'tif', 'bmp', 'dib', 'jp2', 'webp', 'pbm', 'pgm', 'ppm', 'pxm', 'pnm']


class ImageCollection:
    """slam/data.py:83-125 without cv2: the image files of a folder in sorted order (``image_string`` selects by substring), or a list of files, read
    with Pillow as RGB."""

    def __init__(self, inp, image_string=None):
        def sel_file(ff):
            return ff.split('.')[-1].lower() in IMAGE_FORMATS and (image_string is None or image_string in ff)
        if isinstance(inp, str) and os.path.isdir(inp):
            self.frames = [os.path.join(inp, ff) for ff in sorted(os.listdir(inp)) if sel_file(ff)]
        else:
            self.frames = [ff for ff in ([inp] if isinstance(inp, str) else list(inp)) if sel_file(os.path.basename(ff))]
        assert len(self.frames) != 0, f"no image file in {inp}"
        print(f"Found {len(self)} frames")
        self.current_frame = 0

    def __len__(self):
        return len(self.frames)

    def grab(self):
        self.current_frame += 1

    def read(self):
        import PIL.Image
        im = None
        if self.current_frame < len(self):
            im = np.asarray(PIL.Image.open(self.frames[self.current_frame]).convert('RGB'))
            self.current_frame += 1
        return im


def open_input(inputs, image_string=None):
    """--input: one folder of images, or a list of image files.  Camera streams and video files need cv2, which this package does not use."""
    inputs = [inputs] if isinstance(inputs, str) else list(inputs)
    for inp in inputs:
        if inp.startswith('cam:'):
            raise SystemExit(f"must3r_amd.slam: input {inp}: camera capture needs cv2 (OpenCV), which is not available here; give a folder or a list of images")
    if len(inputs) == 1 and os.path.isdir(inputs[0]):
        return ImageCollection(inputs[0], image_string)
    for inp in inputs:
        if os.path.isdir(inp):
            raise SystemExit("must3r_amd.slam: several folders mean several agents, whose frames the reference interleaves through cv2 loaders; give one folder")
        if not os.path.isfile(inp):
            raise SystemExit(f"must3r_amd.slam: incorrect input {inp}")
        if inp.split('.')[-1].lower() not in IMAGE_FORMATS:
            raise SystemExit(f"must3r_amd.slam: input {inp}: video files need cv2 (OpenCV), which is not available here; give a folder or a list of images")
    return ImageCollection(inputs, image_string)


def get_parser():
    """slam/slam.py:570-611"""
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--chkpt', required=True, help='Path to checkpoint.')
    parser.add_argument('--device', default='cuda:0', help='Device to run on (e.g. "cuda:0").')
    parser.add_argument('--input', default='cam:0', nargs='+', help="A folder of images or a list of image files.")
    parser.add_argument('--image_string', default=None, type=str, help="In the case of an image collection, string to identify image files.")
    parser.add_argument('--load_memory', default=None, type=str, help="Load memory from another run.")
    parser.add_argument('--output', default=None, type=str, help="Output directory to write predictions")
    parser.add_argument('--res', default=224, choices=[224, 512], type=int, help="Image resolution that works for the model used.")
    parser.add_argument('--skip_every', default=1, type=int, help="Subsample input by skipping frames.")
    parser.add_argument('--rerender', action='store_true', default=False, help="Rerender all frames at the end.")
    parser.add_argument('--rerender_bs', default=64, type=int, help="Re-rendering batch size")
    parser.add_argument('--filter', action='store_true', default=False, help="Minimal Laplacian filtering after rerender.")
    parser.add_argument('--searcher', default="bvh-hip-quadrant_x2", type=str, help="Method for overlap prediction")
    parser.add_argument('--overlap_mode', default="nn-norm", type=str, help="How to estimate overlap")
    parser.add_argument('--subsamp', default=2, type=int)
    parser.add_argument('--keyframe_overlap_thr', default=.1, type=float, help="At least this overlap to add incoming image in memory")
    parser.add_argument('--min_conf_keyframe', default=1.2, type=float, help="Ignore 3D points below this confidence.")
    parser.add_argument('--overlap_percentile', default=85., type=float, help="Percentile of image distances to compute overlap")
    parser.add_argument('--varying_focals', action='store_true', default=False, help="Focals may vary along sequence (e.g. zoom-in/out).")
    parser.add_argument('--force_first_keyframes', default=None, type=int)
    parser.add_argument('--num_init_frames', default=2, type=int)
    parser.add_argument('--viz_conf', default=4., type=float, help="Conf threshold for pts3d vizu")
    parser.add_argument('--gui', action='store_true', default=False, help="Refused: the GUI needs open3d")
    parser.add_argument('--hide_cameras', action='store_true', default=False)
    parser.add_argument('--render_dir', default=None, type=str,
                        help="Headless stand-in for the GUI: after the run, write a fly-through there, one PNG frame per pose (must3r_amd.render).")
    return parser


def flythrough_points(model, viz_conf):
    """-> (conf [1, N], pts [1, N, 3], rgb [1, N, 3]), one 1 x N view: the re-rendered pointmaps of all frames when there are any
    (``all_pts3d``, every point, coloured by its frame), else the keyframe map at ``viz_conf`` (``fetch_memory_map``)."""
    if model.all_pts3d is not None:
        pts = model.all_pts3d.reshape(-1, 3)
        cols = torch.cat([prep_imgs(im['img'], [0.5] * 3, [0.5] * 3).reshape(-1, 3) for im in model.all_images]).to(torch.float32)
    else:
        memory_map = model.fetch_memory_map(viz_conf)
        if memory_map is None:
            memory_map = get_map(model.keyframe_pointmaps, viz_conf)
        pts, cols = memory_map
    n = pts.shape[0]
    return torch.ones((1, n)), pts.reshape(1, n, 3), cols.reshape(1, n, 3)


def render_flythrough(model, outdir, viz_conf=4., W=512, H=384, point_size=2, batch=32):
    """One ``render.follow_camera`` frame (the reference's ``reset_view``) per pose of ``all_poses`` over ``flythrough_points``, ``batch`` cameras
    per render call -> the list of paths."""
    from . import render as _render
    view = flythrough_points(model, viz_conf)
    cams = [_render.follow_camera(p.cpu().numpy() if torch.is_tensor(p) else p, W, H) for p in model.all_poses]
    return _render.render_views(outdir, [view], None, cams, thr=0.5, point_size=point_size, batch=batch)


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.gui:
        raise SystemExit("must3r_amd.slam: --gui needs open3d, which is not available here; run headless with --output, and with --render_dir for a "
                         "rendered fly-through of the map")
    camera = open_input(args.input, args.image_string)
    assert args.output is not None, "You should define an output folder"
    model = SLAM_MUSt3R(chkpt=args.chkpt, res=args.res, kf_x_subsamp=args.subsamp, searcher=args.searcher, overlap_mode=args.overlap_mode,
                        keyframe_overlap_thr=args.keyframe_overlap_thr, min_conf_keyframe=args.min_conf_keyframe,
                        overlap_percentile=args.overlap_percentile, rerender=args.rerender, keep_memory=True, load_memory=args.load_memory,
                        fixed_focal=not args.varying_focals, num_agents=1, device=args.device, num_init_frames=args.num_init_frames)
    os.makedirs(args.output, exist_ok=True)

    def grab_frame():
        frame = camera.read()
        for _ in range(args.skip_every - 1):
            camera.grab()
        return frame

    print(f"Start processing sequence of {len(camera)} frames")
    frame = grab_frame()
    start = time.time()
    imgHWs = [frame.shape[:2]]
    for frame_id in range(len(camera) // args.skip_every):
        model(frame, frame_id * args.skip_every, 0, device_outputs=True)
        frame = grab_frame()
        if frame is not None:
            imgHWs.append(frame.shape[:2])
    if args.rerender:
        model.rerender_all_frames(maxbs=args.rerender_bs)
    wallclock_time = time.time() - start
    fps = (len(camera) // args.skip_every) / wallclock_time
    gpumem = torch.cuda.max_memory_allocated() / 1024. ** 2
    print(f"Done @{fps}fps on average using {gpumem}MB GPU Memory")
    tolog = {'fps': fps, 'gpumem': gpumem, 'imgHWs': imgHWs}
    if not args.filter:
        model.write_all_poses(os.path.join(args.output, 'all_poses.npz'), **tolog)
    else:
        filtering_mode, filtering_alpha, filtering_steps = 'laplacian', .1, 256
        outfile = os.path.join(args.output, f"all_poses{filtering_mode}_{filtering_steps}-steps_{filtering_alpha}-alpha.npz")
        model.write_all_poses(outfile, filtering_mode=filtering_mode, filtering_steps=filtering_steps, filtering_alpha=filtering_alpha, **tolog)
    outname = os.path.join(args.output, "memory.pkl")
    count = 0
    while args.load_memory == outname:  # make sure you do not overwrite loaded memory file
        outname = os.path.join(args.output, f"memory_{count}.pkl")
        count += 1
    print(f"Dumping memory as {outname}")
    model.save_memory(outname)
    if args.render_dir is not None:
        frames = render_flythrough(model, args.render_dir, args.viz_conf)
        print(f"Wrote {len(frames)} fly-through frames to {args.render_dir}")


if __name__ == "__main__":
    main()
