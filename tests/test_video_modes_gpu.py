"""GPU (-m gpu): the video modes end to end (must3r_amd.demo.must3r_inference_video, get_reconstructed_scene) on PNG files and the
synthetic 224 models: vidseq equals a direct inference_video_multi_ar call with the same schedule; vidslam on the GPU index equals
vidslam on the brute-force quadrant searcher (same keyframes, bit-equal pointmaps, focals and poses); all four modes run."""
import functools

import numpy as np
import pytest
import torch

from must3r_amd import demo as Dm
from must3r_amd.slam_nn import QuandrantSearcher, get_overlap_score, get_searcher
from test_asmk_gpu import _models, _pngs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_vidseq_equals_direct_call(tmp_path):
    from must3r_amd.engine import postprocess
    from must3r_amd.image import load_images
    from must3r_amd.inference import inference_video_multi_ar
    from must3r_amd.model import get_pointmaps_activation
    _, enc, dec = _models()
    act = get_pointmaps_activation(dec, verbose=False)
    files = _pngs(tmp_path, 7)
    key = lambda id, res, scene_state: id % 3 == 0   # noqa: E731
    scene = Dm.must3r_inference_video((enc, dec), DEV, 224, False, files, 0, 2, 1, local_context_size=3, is_keyframe_function=key,
                                      verbose=False)
    views = load_images(files, 224, verbose=False)
    out = inference_video_multi_ar(enc, dec, [v["img"].to(DEV) for v in views], [torch.from_numpy(v["true_shape"]).to(DEV) for v in views],
                                   [2, 1, 1, 1, 1, 1], device=DEV, preserve_gpu_mem=True, local_context_size=3, is_keyframe_function=key,
                                   post_process_function=lambda x: postprocess(x, pointmaps_activation=act, compute_cam=True))
    assert scene.image_list == files and len(scene.x_out) == 7
    for i in range(7):
        for k in ("pts3d", "pts3d_local", "conf", "focal", "c2w"):
            assert torch.equal(scene.x_out[i][k], out[i][k].cpu()), (i, k)
        assert scene.focals[i] == float(out[i]["focal"].cpu())
        assert torch.equal(scene.cams2world[i], out[i]["c2w"].cpu())


class _QuadrantOnDevice(QuandrantSearcher):
    """the brute-force quadrant searcher fed the driver's host results on the device (BVH_hip copies host points itself)"""

    def add_pts(self, pts, cam_center, **kw):
        super().add_pts(pts.to(DEV), cam_center)

    def query(self, pts, cam_center, **kw):
        return super().query(pts.to(DEV), cam_center)


def _vidslam(enc, dec, files, method, thr, scores=None):
    flags = {}

    def is_key(id, res, scene_state):
        if scores is not None:
            r = {k: v.unsqueeze(0).unsqueeze(0) for k, v in res.items()}
            scores.append(float(get_overlap_score(r, scene_state, res["c2w"][:3, -1], mode="nn-norm", kf_x_subsamp=2, percentile=70)))
        flags[id] = bool(Dm.slam_is_keyframe(2, 1.5, thr, 70, "nn-norm", id, res, scene_state))
        return flags[id]
    tree = get_searcher(method) if method.startswith("bvh") else _QuadrantOnDevice(method)
    scene = Dm.must3r_inference_video((enc, dec), DEV, 224, False, files, 0, 2, 1, local_context_size=3, is_keyframe_function=is_key,
                                      scene_state=tree, scene_state_update_function=functools.partial(Dm.slam_update_scene_state, 2, 1.5),
                                      verbose=False)
    return scene, flags, tree


def test_vidslam_index_equals_brute_force(tmp_path):
    _, enc, dec = _models()
    files = _pngs(tmp_path, 8)
    scores = []
    _vidslam(enc, dec, files, "kdtree-scipy-quadrant_x2", float("inf"), scores)     # every later frame scored against the first two
    thr = float(np.median(scores))
    sa, fa, ta = _vidslam(enc, dec, files, "bvh-hip-quadrant_x2", thr)
    sb, fb, tb = _vidslam(enc, dec, files, "kdtree-scipy-quadrant_x2", thr)
    assert fa == fb and any(fa.values()) and not all(fa.values()), (fa, scores, thr)
    assert ta.n > 0 and isinstance(tb, QuandrantSearcher)
    assert sa.focals == sb.focals
    for a, b in zip(sa.x_out, sb.x_out):
        assert all(torch.equal(a[k], b[k]) for k in ("pts3d", "pts3d_local", "conf", "focal", "c2w"))
    assert all(torch.equal(a, b) for a, b in zip(sa.cams2world, sb.cams2world))


@pytest.mark.parametrize("mode", ["vidseq", "vidslam", "linseq", "retrieval"])
def test_get_reconstructed_scene_runs(tmp_path, mode):
    from test_asmk_gpu import _retrieval_files
    cfg, enc, dec = _models()
    files = _pngs(tmp_path, 6)
    retrieval = _retrieval_files(tmp_path, cfg.enc_dim)[0] if mode == "retrieval" else None
    np.random.seed(0)
    scene, outfile = Dm.get_reconstructed_scene(
        str(tmp_path), None, False, (enc, dec), retrieval, DEV, False, 224, False, files, 0, 0, mode, 4, False, 3, 2, 3, 2, 1.5, 0.05, 70,
        3.0, True, False, False, 0.05)
    assert outfile is None and len(scene.x_out) == 6 and sorted(scene.image_list) == sorted(files)
    assert all(np.isfinite(f) for f in scene.focals)
    assert all(torch.isfinite(x["pts3d"]).all() for x in scene.x_out)
