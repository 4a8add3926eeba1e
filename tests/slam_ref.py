"""The yardstick of the SLAM agent's per-frame step (must3r_amd/slam.py, csrc/slam.hip): must3r/slam/model.py's get_camera_pose, postproc_pred,
get_overlap_score and mean_focal and slam/tools.py's two smoothing functions restated on the CPU, in the dtype of the tensors they are given (fp64 inputs:
an fp64 evaluation).  tests/test_slam_host.py holds it to the reference's own functions at rtol 1e-10.

What the restatement keeps from the reference on purpose:
* get_camera_pose rectifies the local depth IN PLACE (the reference multiplies through a view of res['pts3d_local']), so the depth postproc_pred returns
  and the depths that normalise the 'nn-norm' score are the rectified ones; the first frame is the identity and is not rectified;
* the ratio is formed in the tensors' dtype from the scalar seq_focal, as torch forms ``scalar / tensor``;
* get_overlap_score forms ``depth + eps`` in the depth's dtype (numpy keeps fp32 for ``fp32 array + python float``), divides in fp64, replaces +inf by
  the largest fp64 and calls numpy's percentile."""
import numpy as np
import torch

from oracle import cam_ref


def mean_focal(seq_focals, dtype=np.float64):
    """slam/model.py:131-137; ``dtype=np.float32`` gives the reference's own arithmetic (its lists hold fp32 values)"""
    out = None
    if len(seq_focals['f']):
        focals = np.array(seq_focals['f'], dtype=dtype)
        confs = np.array(seq_focals['conf'], dtype=dtype)
        out = (focals * confs / confs.sum()).sum()
    return out


def get_camera_pose(res, seq_focal, HW, is_first_frame=False, rectify=True, c2w_dtype=torch.float32):
    """slam/model.py:147-172.  res['pts3d_local'] is rectified in place.  The reference assembles c2w in fp32 whatever the dtype of the maps
    (``torch.eye(4)``); ``c2w_dtype=torch.float64`` keeps the fp64 solution."""
    B = res['pts3d'].shape[1]
    dtype = c2w_dtype
    H, W = HW
    pp = torch.tensor((W / 2, H / 2))
    focal = cam_ref.estimate_focal_knowing_depth(res['pts3d_local'][0], pp, focal_mode='weiszfeld')
    focal_ratio = 1.
    if seq_focal is not None and rectify:
        focal_ratio = torch.tensor(float(seq_focal), dtype=focal.dtype) / focal[:, None]
    if is_first_frame:
        R = torch.eye(3, dtype=dtype).repeat(B, 1, 1)
        T = torch.zeros(3, dtype=dtype).repeat(B, 1)
    else:
        pts3d_local = res['pts3d_local'][0].view(B, -1, 3)
        pts3d_local[..., -1] *= focal_ratio
        R, T = cam_ref.rigid_points_registration(pts3d_local, res['pts3d'][0].view(B, -1, 3), weights=res['conf'][0].view(B, -1) - 1.,
                                                 compute_scaling=False)
    c2w = torch.eye(4, dtype=dtype).repeat(B, 1, 1)
    c2w[:, :3, :3] = R
    c2w[:, :3, 3] = T
    return c2w, focal


def overlap_values(dists, depths=None, eps=1e-9):
    """the fp64 array np.percentile sees (slam/model.py:82-87): ``dists`` fp64 numpy, ``depths`` the selected depths in their own dtype, or None"""
    dists = np.array(dists, dtype=np.float64)
    if depths is not None:
        dists /= depths + eps
    dists[np.isposinf(dists)] = np.finfo(dists.dtype).max
    return dists


def get_overlap_score(res, overlap_tree, cam_center, mode='nn', kf_x_subsamp=None, min_conf_keyframe=1.5, percentile=70, eps=1e-9):
    """slam/model.py:62-91"""
    outscore = 0.
    if mode == 'meanconf':
        outscore = res['conf'].mean()
    elif mode == 'medianconf':
        outscore = res['conf'].median()
    elif 'nn' in mode:
        pts3d = res['pts3d'][0, 0, ::kf_x_subsamp, ::kf_x_subsamp] if kf_x_subsamp else res['pts3d']
        msk = res['conf'][0, 0, ::kf_x_subsamp, ::kf_x_subsamp] if kf_x_subsamp else res['conf']
        msk = msk > min_conf_keyframe
        if msk.sum() > 0:
            dists = overlap_tree.query(pts3d[msk], cam_center=cam_center)
            depths = None
            if 'norm' in mode:
                depths = res['pts3d_local'][0, 0, ::kf_x_subsamp, ::kf_x_subsamp, -1][msk].cpu().numpy()
            outscore = np.percentile(overlap_values(dists, depths, eps), percentile)
    else:
        raise ValueError(f"Unknown overlap score method {mode}")
    return outscore


def prep_imgs(cimg, img_mean, img_std):
    cimg = cimg.permute(0, 2, 3, 1)
    return (cimg * torch.tensor(img_std)) + torch.tensor(img_mean)


def postproc_pred(img, res, is_first_frame, seq_focals, fixed_focal=True, overlap_mode='nn-norm', overlap_tree=None, kf_x_subsamp=None,
                  keyframe_overlap_thr=.15, min_conf_keyframe=1.5, overlap_percentile=70, img_mean=[0.5, 0.5, 0.5], img_std=[0.5, 0.5, 0.5],
                  focal_dtype=np.float64):
    """slam/model.py:185-248; ``depth`` is a view of res['pts3d_local'] and so holds the rectified values after get_camera_pose"""
    assert res['pts3d'].shape[0] == 1 and res['pts3d'].shape[1] == 1
    depth = res['pts3d_local'][0, 0, ..., -1]
    conf = res['conf'][0, 0]
    msk = res['conf'] > min_conf_keyframe
    if kf_x_subsamp:
        msk = msk[0, 0, ::kf_x_subsamp, ::kf_x_subsamp]
        pts = res['pts3d'][0, 0, ::kf_x_subsamp, ::kf_x_subsamp][msk]
    else:
        pts = res['pts3d'][msk]
    cols = prep_imgs(img['img'], img_mean=img_mean, img_std=img_std)[None]
    seq_focal = mean_focal(seq_focals, focal_dtype) if fixed_focal else None
    c2w, focal = get_camera_pose(res, seq_focal, HW=img['true_shape'][0], is_first_frame=is_first_frame)
    c2w = c2w[0]
    cam_center = c2w[:3, -1]
    res['overlap_score'] = get_overlap_score(res, overlap_tree, cam_center=cam_center, mode=overlap_mode, kf_x_subsamp=kf_x_subsamp,
                                             min_conf_keyframe=min_conf_keyframe, percentile=overlap_percentile)
    choice = res['overlap_score'] > keyframe_overlap_thr if 'nn' in overlap_mode else res['overlap_score'] < keyframe_overlap_thr
    iskeyframe = is_first_frame or (choice and conf.median() > min_conf_keyframe)
    return (pts, res['pts3d'][0, 0], cols.to(torch.float32), depth, conf, focal, torch.inverse(c2w), cam_center, iskeyframe)


def laplacian_smoothing(trajectory, alpha=0.5, iterations=10):
    """slam/tools.py:34-41"""
    out = trajectory.copy()
    for _ in range(iterations):
        for i in range(1, len(trajectory) - 1):
            out[i] = (1 - alpha) * out[i] + (alpha / 2) * (out[i - 1] + out[i + 1])
    return out


def laplacian_smoothing_with_confidence(trajectory, confidence, alpha=0.5, iterations=10):
    """slam/tools.py:44-63"""
    out = trajectory.copy()
    for _ in range(iterations):
        for i in range(1, len(trajectory) - 1):
            ws = (1 - alpha) * confidence[i]
            wp = alpha * (1 - confidence[i - 1]) / 2
            wn = alpha * (1 - confidence[i + 1]) / 2
            sumw = ws + wp + wn
            ws, wp, wn = ws / sumw, wp / sumw, wn / sumw
            out[i] = ws * out[i] + wp * out[i - 1] + wn * out[i + 1]
    return out
