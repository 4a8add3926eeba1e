"""Host side of the video modes (must3r_amd.demo: must3r_inference_video, slam_is_keyframe, slam_update_scene_state,
get_reconstructed_scene), no GPU needed: the reference's own demo/inference.py and the execution-mode dispatch of demo/gradio.py:160-217
run against the native functions with the same recorders standing in for the loaders, the video driver, must3r_inference and the
searcher.  The memory batches, local_context_size, keyframe decisions, map updates and SceneState fields must be equal."""
import ast
import datetime
import functools
import os

import numpy as np
import pytest
import torch

from must3r_amd import demo as Dm
from test_asmk_host import _Decoder, _Encoder, _fake_views, ref_demo  # noqa: F401  (ref_demo: the reference's demo/inference.py)

from oracle.ref_shims import REFERENCE_ROOT

REF_GRADIO = os.path.join(REFERENCE_ROOT, "must3r", "demo", "gradio.py")


def _frame(i, H=12, W=16):
    """a deterministic fake post-processed result of frame i (postprocess(compute_cam=True) keys, no batch dims)"""
    g = torch.Generator().manual_seed(100 + i)
    local = torch.randn((H, W, 3), generator=g) * 0.3
    local[..., 2] = local[..., 2].abs() + 1.0 + 0.1 * i
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.2 * i, 0.05 * i * i % 0.7, -0.1 * i])
    conf = 1.0 + torch.rand((H, W), generator=g) * (1.0 + 0.2 * (i % 4))
    return dict(pts3d=local + c2w[:3, 3], pts3d_local=local, conf=conf, focal=torch.tensor(10.0 + i), c2w=c2w)


class _Searcher:
    """records add_pts / query; a query returns the distance of each point to the nearest point added so far (host, float64)"""

    def __init__(self, method="recording"):
        self.method, self.calls, self.pts = method, [], []

    def add_pts(self, pts, cam_center=None, **kw):
        self.calls.append(("add", np.asarray(pts, np.float64).copy(), np.asarray(cam_center, np.float64).copy()))
        self.pts.append(np.asarray(pts, np.float64))

    def query(self, pts, cam_center=None, **kw):
        q = np.asarray(pts, np.float64)
        self.calls.append(("query", q.copy(), np.asarray(cam_center, np.float64).copy()))
        if not self.pts:
            return np.full(q.shape[0], np.inf)
        db = np.concatenate(self.pts)
        return np.sqrt(((q[:, None, :] - db[None, :, :]) ** 2).sum(-1)).min(1)


def _same_calls(a, b):
    assert len(a) == len(b)
    for (ka, pa, ca), (kb, pb, cb) in zip(a, b):
        assert ka == kb and np.array_equal(pa, pb) and np.array_equal(ca, cb)


class _VideoRecord:
    """load_images + inference_video_multi_ar: records the schedule, then runs the callbacks the way the driver does (the first batch
    is all keyframes, every later frame asks is_keyframe_function) on the fake results"""

    def __init__(self):
        self.calls = []

    def load_images(self, filelist, size, patch_size=16, verbose=True, **kw):
        return _fake_views(len(filelist))

    def inference_video_multi_ar(self, encoder, decoder, imgs, true_shape, mem_batches, local_context_size=25,
                                 is_keyframe_function=None, scene_state=None, scene_state_update_function=None, **kw):
        flags = []
        n0 = mem_batches[0]
        out = []
        for i in range(len(imgs)):
            res = _frame(i)
            key = True if i < n0 else bool(is_keyframe_function(i, res, scene_state))
            if key:
                scene_state = scene_state_update_function(res, scene_state)
            flags.append(key)
            out.append(res)
        self.calls.append(dict(mem_batches=list(mem_batches), local_context_size=local_context_size, flags=flags, n=len(imgs),
                               shapes=[tuple(int(v) for v in t) for t in true_shape],
                               rest={k: kw[k] for k in ("max_bs", "preserve_gpu_mem", "num_refinements_iterations")}))
        return out


def _drive_video(module, monkeypatch, rec, files, **kw):
    monkeypatch.setattr(module, "load_images", rec.load_images)
    monkeypatch.setattr(module, "inference_video_multi_ar", rec.inference_video_multi_ar)
    return module.must3r_inference_video((_Encoder(), _Decoder()), "cpu", 224, False, files, verbose=False, **kw)


@pytest.mark.parametrize("n,init,bnv,lcs,interval", [(1, 2, 1, 25, 3), (2, 2, 1, 4, 2), (7, 2, 1, 3, 3), (12, 3, 2, 5, 4),
                                                      (17, 1, 4, 25, 5), (9, 4, 3, 2, 1)])
def test_inference_video_equals_reference(ref_demo, monkeypatch, n, init, bnv, lcs, interval):   # noqa: F811
    files = [f"frame{i:04d}.png" for i in range(n)]
    rec_ref, rec_nat = _VideoRecord(), _VideoRecord()
    kw = dict(max_bs=0, init_num_images=init, batch_num_views=bnv, local_context_size=lcs,
              is_keyframe_function=lambda id, res, scene_state: id % interval == 0)
    s_ref = _drive_video(ref_demo, monkeypatch, rec_ref, files, **kw)
    s_nat = _drive_video(Dm, monkeypatch, rec_nat, files, **kw)
    assert rec_ref.calls == rec_nat.calls and len(rec_nat.calls) == 1
    assert s_ref.image_list == s_nat.image_list == files
    assert s_ref.focals == s_nat.focals
    assert all(torch.equal(a, b) for a, b in zip(s_ref.cams2world, s_nat.cams2world))
    assert [tuple(int(v) for v in t) for t in s_ref.true_shape] == [tuple(int(v) for v in t) for t in s_nat.true_shape]
    assert len(s_ref.x_out) == len(s_nat.x_out) == n
    for a, b in zip(s_ref.x_out, s_nat.x_out):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert len(s_nat.imgs) == n


@pytest.mark.parametrize("mode,subsample,thr", [("nn", None, 0.17), ("nn", 2, 0.28), ("nn", 3, 0.29), ("nn-norm", 2, 0.15),
                                               ("nn-norm", 3, 0.17)])   # thresholds inside the fake frames' score range
def test_slam_callbacks_equal_reference(ref_demo, mode, subsample, thr):   # noqa: F811
    ref_tree, nat_tree = _Searcher(), _Searcher()
    decisions = {"ref": [], "nat": []}
    for tag, mod, tree in (("ref", ref_demo, ref_tree), ("nat", Dm, nat_tree)):
        for i in range(10):
            res = _frame(i)
            if i < 2:
                assert mod.slam_update_scene_state(subsample, 1.5, res, tree) is tree
                continue
            key = mod.slam_is_keyframe(subsample, 1.5, thr, 70, mode, i, res, tree)
            decisions[tag].append(bool(key))
            if key:
                mod.slam_update_scene_state(subsample, 1.5, res, tree)
    assert decisions["ref"] == decisions["nat"]
    assert any(decisions["nat"]) and not all(decisions["nat"])        # both branches of the decision occur
    _same_calls(ref_tree.calls, nat_tree.calls)


def test_slam_is_keyframe_refuses_nan(ref_demo):   # noqa: F811
    class NanTree(_Searcher):
        def query(self, pts, cam_center=None, **kw):
            return np.full(np.asarray(pts).shape[0], np.nan)
    for mod in (ref_demo, Dm):
        with pytest.raises(AssertionError):
            mod.slam_is_keyframe(2, 1.5, 0.1, 70, "nn", 3, _frame(3), NanTree())


# ---------------------------------------------------------------------------------------------------------------------------------
# get_reconstructed_scene: the reference's function compiled alone from gradio.py (its module needs gradio, trimesh, viser)
# ---------------------------------------------------------------------------------------------------------------------------------
class _DispatchRecord:
    def __init__(self):
        self.calls, self.searchers = [], []

    def get_searcher(self, method):
        s = _Searcher(method)
        self.searchers.append(s)
        return s

    def must3r_inference_video(self, model, device, image_size, amp, filelist, max_bs, init_num_images, batch_num_views, viser_server=None,
                               num_refinements_iterations=0, local_context_size=25, is_keyframe_function=None, scene_state=None,
                               scene_state_update_function=None, verbose=True):
        flags = []
        for i in range(len(filelist)):
            res = _frame(i)
            key = True if i < init_num_images else bool(is_keyframe_function(i, res, scene_state))
            if key:
                scene_state = scene_state_update_function(res, scene_state)
            flags.append(key)
        self.calls.append(dict(fn="video", args=(model, device, image_size, amp, tuple(filelist), max_bs, init_num_images,
                                                 batch_num_views, viser_server, num_refinements_iterations, local_context_size, verbose),
                               flags=flags, state=None if scene_state is None else scene_state.method))
        return "scene"

    def must3r_inference(self, model, retrieval, device, image_size, amp, filelist, num_mem_images, max_bs, init_num_images, batch_num_views,
                         render_once, is_sequence, viser_server=None, num_refinements_iterations=0, verbose=True):
        self.calls.append(dict(fn="images", args=(model, retrieval, device, image_size, amp, tuple(filelist), num_mem_images, max_bs,
                                                  init_num_images, batch_num_views, render_once, is_sequence, viser_server,
                                                  num_refinements_iterations, verbose)))
        return "scene"


def _ref_get_reconstructed_scene(ref_demo, rec):   # noqa: F811
    src = open(REF_GRADIO).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_reconstructed_scene")
    node.decorator_list = []
    ns = dict(functools=functools, datetime=datetime, torch=torch, slam_is_keyframe=ref_demo.slam_is_keyframe,
              slam_update_scene_state=ref_demo.slam_update_scene_state, get_searcher=rec.get_searcher,
              must3r_inference_video=rec.must3r_inference_video, must3r_inference=rec.must3r_inference,
              get_3D_model_from_scene=None)
    exec(compile(ast.Module(body=[node], type_ignores=[]), REF_GRADIO, "exec"), ns)
    return ns["get_reconstructed_scene"]


def _scene_args(mode, files, loaded=""):
    return dict(outdir="/tmp/out", viser_server=None, should_save_glb=False, model=("enc", "dec"), retrieval="ret.pth", device="cpu",
                verbose=False, image_size=512, amp=False, filelist=files, max_bs=3, num_refinements_iterations=1, execution_mode=mode,
                num_mem_images=4, render_once=True, vidseq_local_context_size=5, keyframe_interval=3, slam_local_context_size=7,
                subsample=2, min_conf_keyframe=1.5, keyframe_overlap_thr=0.15, overlap_percentile=70, min_conf_thr=3.0,
                as_pointcloud=True, transparent_cams=False, local_pointmaps=False, cam_size=0.05, loaded_files=loaded)


@pytest.mark.parametrize("mode", ["vidseq", "vidslam", "linseq", "retrieval"])
def test_get_reconstructed_scene_equals_reference(ref_demo, monkeypatch, mode):   # noqa: F811
    files = [f"f{i}.png" for i in range(11)]
    rec_ref, rec_nat = _DispatchRecord(), _DispatchRecord()
    ref_fn = _ref_get_reconstructed_scene(ref_demo, rec_ref)
    for name in ("get_searcher", "must3r_inference_video", "must3r_inference"):
        monkeypatch.setattr(Dm, name, getattr(rec_nat, name))
    for files_arg, loaded in ((files, ""), (None, "\n".join(files))):
        out_ref = ref_fn(**_scene_args(mode, files_arg, loaded))
        out_nat = Dm.get_reconstructed_scene(**_scene_args(mode, files_arg, loaded))
        assert out_ref == out_nat == ("scene", None)
    assert [{k: v for k, v in c.items() if k != "state"} for c in rec_ref.calls] == \
        [{k: v for k, v in c.items() if k != "state"} for c in rec_nat.calls]
    if mode == "vidslam":
        assert [s.method for s in rec_ref.searchers] == ["kdtree-scipy-quadrant_x2"] * 2
        assert [s.method for s in rec_nat.searchers] == ["bvh-hip-quadrant_x2"] * 2
        flags = rec_nat.calls[0]["flags"]
        assert any(flags[2:]) and not all(flags[2:])
        for a, b in zip(rec_ref.searchers, rec_nat.searchers):
            _same_calls(a.calls, b.calls)
    else:
        assert not rec_nat.searchers
    if mode == "vidseq":
        assert rec_nat.calls[0]["flags"] == [i < 2 or i % 3 == 0 for i in range(11)]
    assert ref_fn(**_scene_args(mode, None, "")) == Dm.get_reconstructed_scene(**_scene_args(mode, None, "")) == (None, None)


def test_get_reconstructed_scene_refuses_glb_export():
    args = _scene_args("vidseq", ["a.png"])
    args["should_save_glb"] = True
    with pytest.raises(NotImplementedError, match="GLB"):
        Dm.get_reconstructed_scene(**args)


def test_gradio_partials_bind_unchanged():
    """demo/gradio.py binds the callbacks with functools.partial over the leading parameters; the native signatures take them in order"""
    f = functools.partial(Dm.slam_is_keyframe, 2, 1.5, 0.1, 70, "nn-norm")
    u = functools.partial(Dm.slam_update_scene_state, 2, 1.5)
    tree = _Searcher()
    assert u(_frame(0), tree) is tree
    assert isinstance(bool(f(5, _frame(5), tree)), bool)
