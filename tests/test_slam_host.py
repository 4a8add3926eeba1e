"""No GPU: the SLAM agent (must3r_amd/slam.py, csrc/slam.hip).  The yardstick tests/slam_ref.py against the reference's own functions (compiled out of
must3r/slam/model.py and slam/tools.py, rtol 1e-10; skipped where the reference tree does not exist), the bookkeeping of SLAM_MUSt3R.__call__ against the
reference's class over the same recorded per-frame results, and the library's surface: symbols, descriptor offsets, every refusal, ABI 21."""
import ast
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import slam_ref as SR
from conftest import HAS_REFERENCE, ROOT
from must3r_amd import _lib
from must3r_amd import synthetic as S

needs_reference = pytest.mark.skipif(not HAS_REFERENCE, reason="runs the reference's code live; its tree is not present")
RTOL = 1e-10


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference's side
# ---------------------------------------------------------------------------------------------------------------------------------------
def _reference_functions(path, names, namespace):
    """the named functions of one reference file, each executed verbatim from the reference tree into ``namespace`` (nothing is copied into the repo)"""
    from oracle import ref_shims
    path = os.path.join(ref_shims.REFERENCE_ROOT, path)
    body = ast.parse(open(path).read()).body
    for name in names:
        node = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)
        exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
    return namespace


def _model_functions():
    from oracle import cam_ref
    roma = types.SimpleNamespace(rigid_points_registration=cam_ref.rigid_points_registration)
    ns = {"np": np, "torch": torch, "roma": roma, "estimate_focal_knowing_depth": cam_ref.estimate_focal_knowing_depth}
    return _reference_functions("must3r/slam/model.py", ["get_overlap_score", "prep_imgs", "choose_keyframe_from_overlap", "mean_focal", "build_intr",
                                                         "get_camera_pose", "get_map", "postproc_pred"], ns)


def _reference_slam_module():
    """must3r.slam.model itself, imported on the leaf shims plus the dust3r leaves they lack (registered here, not in oracle/)"""
    import importlib
    from oracle import ref_shims
    ref_shims.install()
    for name in ("dust3r.datasets", "dust3r.datasets.utils", "dust3r.datasets.utils.transforms", "must3r.tools.path_to_dust3r"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    sys.modules["dust3r.datasets.utils.transforms"].ImgNorm = "ImgNorm"
    if not hasattr(sys.modules["dust3r.utils.image"], "_resize_pil_image"):
        sys.modules["dust3r.utils.image"]._resize_pil_image = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError())
    return importlib.import_module("must3r.slam.model")


def _frame(seed, H=24, W=32, dtype=torch.float64):
    """one frame's activated maps with the leading [1, 1], from a noisy pinhole scene"""
    from oracle import must3r_ref as R
    act = R.postprocess(S.make_cam_pointmaps(1, H, W, focal=0.9 * W, noise=0.02, seed=seed))
    return {k: act[k].to(dtype)[None].clone() for k in ("pts3d", "pts3d_local", "conf")}


def _close(a, b):
    a, b = (torch.as_tensor(np.asarray(x.detach() if torch.is_tensor(x) else x), dtype=torch.float64) for x in (a, b))
    assert a.shape == b.shape
    assert torch.allclose(a, b, rtol=RTOL, atol=0), float(((a - b).abs() / b.abs().clip(min=1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the yardstick against the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("case", ["first", "none", "seq0.8", "seq1.3"])
def test_get_camera_pose_equals_reference(case):
    ref = _model_functions()["get_camera_pose"]
    a, b = _frame(3), _frame(3)
    local0 = a["pts3d_local"].clone()
    f0 = float(SR.get_camera_pose(_frame(3), None, (24, 32))[1][0])
    seq = None if case in ("first", "none") else float(case[3:]) * f0
    ca, fa = ref(a, seq, (24, 32), is_first_frame=case == "first")
    cb, fb = SR.get_camera_pose(b, seq, (24, 32), is_first_frame=case == "first")
    _close(cb, ca)
    _close(fb, fa)
    _close(b["pts3d_local"], a["pts3d_local"])
    if seq is None or case == "first":
        assert torch.equal(b["pts3d_local"], local0)
    else:   # rectified in place, z alone
        assert torch.equal(b["pts3d_local"][..., :2], local0[..., :2])
        assert torch.equal(b["pts3d_local"][..., 2], local0[..., 2] * (torch.tensor(seq, dtype=torch.float64) / fb[0]))
    if case == "first":
        assert torch.equal(cb[0], torch.eye(4, dtype=torch.float64))


class _Tree:
    """stands in for a searcher: distances that depend on the points alone, some of them +inf"""

    def query(self, pts, cam_center=None):
        d = np.abs(pts.cpu().numpy().astype(np.float64)).sum(-1) * 0.01
        d[::7] = np.inf
        return d


@needs_reference
@pytest.mark.parametrize("mode,subsamp", [("nn-norm", 2), ("nn", 2), ("nn", None), ("meanconf", 2), ("medianconf", 2)])
@pytest.mark.parametrize("first", [False, True])
def test_postproc_pred_equals_reference_and_returns_the_rectified_depth(mode, subsamp, first):
    ref = _model_functions()["postproc_pred"]
    a, b = _frame(5), _frame(5)
    z0 = a["pts3d_local"][0, 0, ..., -1].clone()
    img = {"img": torch.rand(1, 3, 24, 32, dtype=torch.float64), "true_shape": np.int32([[24, 32]])}
    f0 = float(SR.get_camera_pose(_frame(5), None, (24, 32))[1][0])
    seq = {"f": [0.8 * f0, 0.9 * f0], "conf": [1.5, 0.5]}
    kw = dict(overlap_mode=mode, overlap_tree=_Tree(), kf_x_subsamp=subsamp, keyframe_overlap_thr=0.05, min_conf_keyframe=1.2, overlap_percentile=85)
    ra, rb = ref(img, a, first, seq, **kw), SR.postproc_pred(img, b, first, seq, **kw)
    for x, y in zip(ra[:8], rb[:8]):
        _close(y, x)
    assert bool(ra[8]) == bool(rb[8])
    _close(b["overlap_score"], a["overlap_score"])
    depth = rb[3]
    if first:
        assert torch.equal(depth, z0)
    else:   # the depth the agent returns is the rectified one
        ratio = torch.tensor(float(SR.mean_focal(seq)), dtype=torch.float64) / rb[5][0]
        assert torch.equal(depth, z0 * ratio) and not torch.equal(depth, z0)
        assert depth.data_ptr() == b["pts3d_local"][0, 0, ..., -1].data_ptr()


@needs_reference
@pytest.mark.parametrize("mode", ["nn", "nn-norm"])
def test_get_overlap_score_equals_reference_on_the_scipy_searcher(mode):
    """slam/nns.py runs verbatim (scipy KD-tree per quadrant); fp32 frames, as the agent's are"""
    import importlib
    from oracle import ref_shims
    ref_shims.install()
    nns = importlib.import_module("must3r.slam.nns")
    ref = _model_functions()["get_overlap_score"]
    tree = nns.get_searcher("kdtree-scipy-quadrant_x2")
    for i, f in enumerate(S.make_overlap_frames(2)):
        res = {k: torch.from_numpy(f[k]) for k in ("pts3d", "pts3d_local", "conf")}
        cam = torch.from_numpy(f["cam"])
        for q in (0, 70, 85, 100):
            sa = ref(res, tree, cam, mode=mode, kf_x_subsamp=2, percentile=q)
            sb = SR.get_overlap_score(res, tree, cam, mode=mode, kf_x_subsamp=2, percentile=q)
            assert float(sa) == float(sb), (i, q, sa, sb)
        tree.add_pts(torch.from_numpy(f["pts3d"][0, 0][f["conf"][0, 0] > 1.5]), cam_center=cam)


@needs_reference
def test_mean_focal_and_smoothing_equal_reference():
    from must3r_amd import slam
    ns = _model_functions()
    tools = _reference_functions("must3r/slam/tools.py", ["laplacian_smoothing", "laplacian_smoothing_with_confidence"], {"np": np})
    rng = np.random.default_rng(0)
    seq = {"f": list(40 + rng.random(7)), "conf": list(0.5 + rng.random(7))}
    for fn in (SR.mean_focal, slam.mean_focal):
        _close(fn(seq), ns["mean_focal"](seq))
        assert fn({"f": [], "conf": []}) is None
    traj, conf = rng.standard_normal((12, 3)), rng.random(12)
    for mod in (SR, slam):
        _close(mod.laplacian_smoothing(traj, alpha=0.1, iterations=7), tools["laplacian_smoothing"](traj, alpha=0.1, iterations=7))
        _close(mod.laplacian_smoothing_with_confidence(traj, conf, alpha=0.3, iterations=5),
               tools["laplacian_smoothing_with_confidence"](traj, conf, alpha=0.3, iterations=5))
    for name in ("build_intr", "get_map", "prep_imgs"):
        assert callable(getattr(slam, name))
    _close(slam.build_intr(37.5, 32, 24, "cpu", torch.float64), ns["build_intr"](37.5, 32, 24, "cpu", torch.float64))
    img = torch.rand(2, 3, 4, 5)
    _close(slam.prep_imgs(img, [0.5] * 3, [0.5] * 3), ns["prep_imgs"](img, [0.5] * 3, [0.5] * 3))
    _close(slam.prep_imgs(img, [0.4, 0.5, 0.6], [0.2, 0.3, 0.4]), ns["prep_imgs"](img, [0.4, 0.5, 0.6], [0.2, 0.3, 0.4]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the agent's bookkeeping against the reference's class
# ---------------------------------------------------------------------------------------------------------------------------------------
N_FRAMES = 10
SCRIPT = [False, True, False, False, True, True, False, True, False, False, True, False, True, False, False, True]   # one decision per update call


class _Recorder:
    """a searcher that records what is appended to it"""

    def __init__(self, log):
        self.log = log
        log.append(("new",))

    def add_pts(self, pts, cam_center=None, **kw):
        self.log.append(("add", int(pts.shape[0]), float(pts.reshape(-1)[0]), tuple(float(v) for v in cam_center)))


class _Replay:
    """the recorded per-frame results: what the stub forward and the stub keyframe step hand out, identically on both sides"""

    def __init__(self):
        self.calls = 0          # update calls
        self.forwards = 0
        self.mems = []

    def view(self, frame_id):
        return {"img": torch.full((1, 3, 2, 2), float(frame_id)), "true_shape": np.int32([[2, 2]]), "idx": frame_id}

    def forward(self, views, memory):
        self.forwards += 1
        newmem = ("mem", self.forwards, tuple(int(v["idx"]) for v in views))
        return [{"frame": int(v["idx"])} for v in views], newmem

    def result(self, pred, is_first):
        k, f = self.calls, pred["frame"]
        self.calls += 1
        iskf = bool(is_first or SCRIPT[k % len(SCRIPT)])
        sel = torch.full((3 + f, 3), 100.0 * f + k)
        cam = (0.5 * f, 0.25 * k, 1.0)
        return dict(sel=sel, pts3d=torch.full((2, 2, 3), float(f)), colors=torch.zeros(1, 1, 2, 2, 3), depth=torch.ones(2, 2), conf=torch.full((2, 2), 1.0 + f),
                    focal=30.0 + f, w2c=torch.eye(4), cam=cam, iskf=iskf)


def _drive_reference(num_init, rerender):
    mod = _reference_slam_module()
    rp, log, trace = _Replay(), [], []
    saved = {k: getattr(mod, k) for k in ("load_model", "get_searcher", "preproc_frame", "forward_must3r")}
    try:
        mod.load_model = lambda chkpt, device=None: ("encoder", "decoder")
        mod.get_searcher = lambda method: _Recorder(log)
        mod.preproc_frame = lambda img, idx, res=512, transform=None: (rp.view(idx), 1.0)
        mod.forward_must3r = lambda model, views, memory, device=None: rp.forward(views, memory)
        agent = mod.SLAM_MUSt3R("none", num_init_frames=num_init, rerender=rerender, keep_memory=True, device="cpu")

        def update(inp, pred, is_first_frame, **kw):
            r = rp.result(pred, is_first_frame)
            return r["sel"], r["pts3d"], r["colors"], r["depth"], r["conf"], r["focal"], r["w2c"], torch.tensor(r["cam"]), r["iskf"]
        agent.agents[0].update = update
        for t in range(N_FRAMES):
            out = agent(None, t, 0)
            trace.append((agent.memory, list(agent.keyframes), list(agent.all_timestamps), len(agent.all_images), len(agent.keyframe_pointmaps), bool(out[-1])))
    finally:
        for k, v in saved.items():
            setattr(mod, k, v)
    return trace, log


def _drive_native(num_init, rerender, monkeypatch):
    from must3r_amd import slam
    rp, log, trace = _Replay(), [], []
    monkeypatch.setattr(slam, "slam_searcher", lambda method: _Recorder(log))
    agent = slam.SLAM_MUSt3R(("encoder", "decoder"), num_init_frames=num_init, rerender=rerender, keep_memory=True, device="cpu")
    agent.preproc = lambda img, idx: (rp.view(idx), 1.0)
    agent.forward = lambda views, memory, render=False: rp.forward(views, memory)

    def frame_step(ag, view, pred, is_first_frame, to_orig_focal):
        r = rp.result(pred, is_first_frame)
        rec = np.zeros(_lib.SLAM_RECORD_DOUBLES)
        rec[slam.REC["c2w"]] = np.eye(4).reshape(-1)
        rec[slam.REC["conf_mean"]] = float(r["conf"].mean())
        return r["sel"], r["pts3d"], r["colors"], r["depth"], r["conf"], r["focal"], r["w2c"], r["cam"], r["iskf"], rec
    agent.frame_step = frame_step
    for t in range(N_FRAMES):
        out = agent(None, t, 0)
        trace.append((agent.memory, list(agent.keyframes), list(agent.all_timestamps), len(agent.all_images), len(agent.keyframe_pointmaps), bool(out[-1])))
        assert isinstance(out[0], np.ndarray) and isinstance(out[1], np.ndarray) and len(agent.all_poses) == len(agent.all_timestamps) == len(agent.all_confs)
    return trace, log


@needs_reference
@pytest.mark.parametrize("rerender", [False, True])
@pytest.mark.parametrize("num_init", [1, 2, 3])
def test_call_bookkeeping_equals_reference(num_init, rerender, monkeypatch):
    """keyframes, all_timestamps, len(all_images), which memory object is held after each frame and what is appended to the tree, frame by frame"""
    ref_trace, ref_log = _drive_reference(num_init, rerender)
    trace, log = _drive_native(num_init, rerender, monkeypatch)
    assert len(trace) == len(ref_trace) == N_FRAMES
    for t, (a, b) in enumerate(zip(trace, ref_trace)):
        assert a == b, (t, a, b)
    assert log == ref_log
    assert any(kf for *_, kf in trace[num_init:]) and not all(kf for *_, kf in trace[num_init:])
    assert sum(1 for e in log if e[0] == "new") == (num_init if num_init > 1 else 1)   # the re-initialisation resets the tree


def test_call_bookkeeping_without_the_reference(monkeypatch):
    """the same drive against the values the reference's class gives (recorded by hand from the run above): runs where the reference tree does not exist"""
    trace, log = _drive_native(2, False, monkeypatch)
    # frame 0: first frame -> keyframe.  frame 1: fewer than 2 init frames seen -> reset, frames 0 and 1 again in one forward, frame 0 first again
    assert trace[0][1] == [0] and trace[0][3] == 1 and trace[0][0] == ("mem", 1, (0,))
    assert trace[1][2] == [0, 1] and trace[1][3] == 2 and trace[1][0][2] == (0, 1) and trace[1][1][0] == 0
    assert [e[0] for e in log].count("new") == 2
    assert trace[-1][2] == list(range(N_FRAMES)) and trace[-1][3] == 2
    kfs = trace[-1][1]
    assert kfs == sorted(set(kfs)) and 0 < len(kfs) < N_FRAMES
    last_new = [i for i, e in enumerate(log) if e[0] == "new"][-1]
    assert len([e for e in log[last_new:] if e[0] == "add"]) == len(kfs)
    # reset() hands keyframe_pointmaps the loaded-memory list itself, as the reference does: the entry of the discarded first attempt stays in it
    assert trace[-1][4] == len([e for e in log if e[0] == "add"]) == len(kfs) + 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# host pieces of must3r_amd.slam
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_host_pieces():
    from must3r_amd import slam
    assert slam.mode_bits("nn") == 1 and slam.mode_bits("nn-norm") == 3 and slam.mode_bits("meanconf") == 4 and slam.mode_bits("medianconf") == 8
    with pytest.raises(ValueError):
        slam.mode_bits("retrieval")
    assert slam.candidates(384, 512, 2) == 49152 and slam.candidates(384, 512, 4) == 12288 and slam.candidates(384, 512, None) == 196608
    assert slam.candidates(33, 47, 4) == 9 * 12
    assert slam.slam_searcher("none") is None
    for m, div in (("bvh-hip-quadrant_x2", 2), ("kdtree-scipy-quadrant_x2", 2), ("kdtree-scipy", 0), ("bvh-hip", 0)):
        assert isinstance(slam.slam_searcher(m), slam.BVH_hip) and slam.slam_searcher(m).quadrant_divider == div
    with pytest.raises(ValueError):
        slam.slam_searcher("faiss")
    import inspect
    assert inspect.signature(slam.SLAM_MUSt3R.__init__).parameters["searcher"].default == "bvh-hip-quadrant_x2"
    g = torch.Generator().manual_seed(0)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, 3, generator=g, dtype=torch.float64))
    c2w = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    c2w[:, :3, :3], c2w[:, :3, 3] = Q, torch.randn(3, 3, generator=g, dtype=torch.float64)
    assert torch.allclose(slam.rigid_inverse(c2w), torch.inverse(c2w), rtol=1e-12, atol=1e-12)
    for name in ("SLAM_MUSt3R", "MUSt3R_Agent", "postproc_pred", "get_camera_pose", "mean_focal", "build_intr", "get_map", "prep_imgs",
                 "laplacian_smoothing", "laplacian_smoothing_with_confidence"):
        assert hasattr(slam, name), name
    for name in ("__call__", "reset", "num_mem_frames", "get_true_focals", "write_all_poses", "save_memory", "load_memory", "fetch_memory_map",
                 "rerender_all_frames"):
        assert hasattr(slam.SLAM_MUSt3R, name), name
    assert "not readable by the reference" in slam.SLAM_MUSt3R.save_memory.__doc__


def test_headless_entry_refuses_what_needs_cv2_or_open3d(tmp_path):
    from must3r_amd import slam
    with pytest.raises(SystemExit, match="cv2"):
        slam.open_input(["cam:0"])
    video = tmp_path / "clip.mp4"
    video.write_bytes(b"0")
    with pytest.raises(SystemExit, match="cv2"):
        slam.open_input([str(video)])
    with pytest.raises(SystemExit, match="open3d"):
        slam.main(["--chkpt", "x", "--input", str(tmp_path), "--gui"])
    import PIL.Image
    for i in (2, 0, 1):
        PIL.Image.fromarray(np.full((4, 6, 3), 10 * i, np.uint8)).save(tmp_path / f"f{i}_rgb.png")
    PIL.Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(tmp_path / "other.png")
    cam = slam.open_input([str(tmp_path)], "rgb")
    assert len(cam) == 3 and [int(cam.read()[0, 0, 0]) for _ in range(3)] == [0, 10, 20] and cam.read() is None
    a = slam.get_parser().parse_args(["--chkpt", "x"])
    assert (a.subsamp, a.keyframe_overlap_thr, a.min_conf_keyframe, a.overlap_percentile, a.num_init_frames, a.res, a.skip_every) == (2, .1, 1.2, 85., 2, 224, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        return f.read()


_CTYPE = {"int32_t": (4, 4), "float": (4, 4), "double": (8, 8), "size_t": (8, 8)}


def _struct_layout(name):
    """(field, offset) of a descriptor as the header declares it, by the C rules for the x86-64 / gfx ABI"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, out = 0, []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl, flags=re.S)
        size, align = (8, 8) if m.group(3) or "*" in m.group(4).split(",")[0] else _CTYPE[m.group(2)]
        for field in (f.strip().lstrip("*").strip() for f in m.group(4).split(",")):
            off = (off + align - 1) // align * align
            out.append((field, off))
            off += size
    return out, (off + 7) // 8 * 8


@pytest.mark.parametrize("cname,cls", [("must3r_hip_slam_pose_args", "SlamPoseArgs"), ("must3r_hip_slam_keyframe_args", "SlamKeyframeArgs")])
def test_descriptor_offsets_match_the_header(cname, cls):
    st = getattr(_lib, cls)
    layout, size = _struct_layout(cname)
    assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == layout
    assert C.sizeof(st) == size


def test_abi_surface():
    h = _header()
    assert _lib.ABI_VERSION == 21 and re.search(r"#define\s+MUST3R_HIP_ABI_VERSION\s+21\b", h)
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == 21
    sz, i32 = C.c_size_t, C.c_int
    for name, proto in (("must3r_hip_slam_pose_scratch_bytes", (sz, [i32] * 3)), ("must3r_hip_slam_pose", (i32, [C.POINTER(_lib.SlamPoseArgs)])),
                        ("must3r_hip_slam_keyframe_scratch_bytes", (sz, [i32] * 3)), ("must3r_hip_slam_keyframe", (i32, [C.POINTER(_lib.SlamKeyframeArgs)]))):
        assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == proto and hasattr(lib, name)
    assert re.search(r"\bint\s+must3r_hip_slam_pose\s*\(\s*const\s+must3r_hip_slam_pose_args\s*\*\s*a\s*\)\s*;", h)
    assert re.search(r"\bint\s+must3r_hip_slam_keyframe\s*\(\s*const\s+must3r_hip_slam_keyframe_args\s*\*\s*a\s*\)\s*;", h)
    # no new entry point whose last parameter is a stream: the stream travels in the descriptor
    decl = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert not re.findall(r"\bint\s+(must3r_hip_slam\w+)\s*\([^;{}]*?void\*\s*stream\s*\)\s*;", decl)
    for macro, value in (("MUST3R_SLAM_RECORD_DOUBLES", _lib.SLAM_RECORD_DOUBLES), ("MUST3R_SLAM_FOCAL_STATE_DOUBLES", _lib.SLAM_FOCAL_STATE_DOUBLES),
                         ("MUST3R_SLAM_MODE_NN", _lib.SLAM_MODE_NN), ("MUST3R_SLAM_MODE_NORM", _lib.SLAM_MODE_NORM),
                         ("MUST3R_SLAM_MODE_MEANCONF", _lib.SLAM_MODE_MEANCONF), ("MUST3R_SLAM_MODE_MEDIANCONF", _lib.SLAM_MODE_MEDIANCONF)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, h).group(1)) == value
    with open(os.path.join(ROOT, "must3r_amd", "csrc", "slam.hip")) as f:
        src = f.read()
    assert 'extern "C" int must3r_hip_slam_pose(' in src and 'extern "C" int must3r_hip_slam_keyframe(' in src
    # scratch sizes: the camera pass's + one ratio per view; 12 bytes per candidate + the statistics head
    assert lib.must3r_hip_slam_pose_scratch_bytes(0, 4, 4) == 0 and lib.must3r_hip_slam_keyframe_scratch_bytes(4, 4, -1) == 0
    assert lib.must3r_hip_slam_pose_scratch_bytes(3, 32, 48) >= lib.must3r_hip_postprocess_cam_scratch_bytes(3, 32, 48) + 12
    for H, W, s, cand in ((384, 512, 2, 49152), (384, 512, 4, 12288), (384, 512, 0, 196608), (33, 47, 4, 108)):
        assert cand * 12 + 256 <= lib.must3r_hip_slam_keyframe_scratch_bytes(H, W, s) <= cand * 12 + 256 + 512


def _refused(fn, a, word):
    lib = _lib.load()
    assert fn(C.byref(a)) != 0
    msg = lib.must3r_hip_last_error().decode()
    assert word in msg, (word, msg)


def test_pose_refusals_before_any_launch():
    """every refusal the header lists for must3r_hip_slam_pose; the pointers are never read (host addresses here)"""
    lib = _lib.load()
    fn = lib.must3r_hip_slam_pose
    assert fn(None) != 0 and "null" in lib.must3r_hip_last_error().decode()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)

    def good():
        a = _lib.SlamPoseArgs()
        a.pm = a.pts3d = a.pts3d_local = a.conf = a.focal = a.c2w = a.scratch = p
        a.B, a.H, a.W, a.activation = 1, 32, 48, _lib.ACT_NORM_EXP
        a.scratch_bytes = lib.must3r_hip_slam_pose_scratch_bytes(1, 32, 48)
        return a
    for field in ("pm", "pts3d", "pts3d_local", "conf", "focal", "c2w", "scratch"):
        a = good()
        setattr(a, field, None)
        _refused(fn, a, "null argument")
    for field, v in (("B", 0), ("H", 0), ("W", -1)):
        a = good()
        setattr(a, field, v)
        _refused(fn, a, "B must be at least 1")
    a = good(); a.activation = 7; _refused(fn, a, "activation")
    a = good(); a.update_focal, a.focal_state, a.B = 1, p, 2; a.scratch_bytes = 1 << 30; _refused(fn, a, "one view")
    a = good(); a.update_focal = 1; _refused(fn, a, "needs focal_state")
    a = good(); a.focal_log_cap = -1; _refused(fn, a, "focal_log_cap")
    a = good(); a.focal_log_cap = 4; _refused(fn, a, "focal_log_cap")
    a = good(); a.scratch_bytes -= 1; _refused(fn, a, "scratch too small")


def test_keyframe_refusals_before_any_launch():
    """every refusal the header lists for must3r_hip_slam_keyframe"""
    lib = _lib.load()
    fn = lib.must3r_hip_slam_keyframe
    assert fn(None) != 0 and "null" in lib.must3r_hip_last_error().decode()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)

    def good():
        a = _lib.SlamKeyframeArgs()
        a.pts3d = a.pts3d_local = a.conf = a.c2w = a.sel = a.record = a.scratch = p
        a.H, a.W, a.subsamp, a.divider, a.mode = 32, 48, 4, 2, _lib.SLAM_MODE_NN | _lib.SLAM_MODE_NORM
        a.quantile, a.min_conf = 0.7, 1.5
        a.scratch_bytes = lib.must3r_hip_slam_keyframe_scratch_bytes(32, 48, 4)
        return a
    for field in ("pts3d", "pts3d_local", "conf", "c2w", "sel", "record", "scratch"):
        a = good()
        setattr(a, field, None)
        _refused(fn, a, "null argument")
    for field, v in (("H", 0), ("W", -3)):
        a = good()
        setattr(a, field, v)
        _refused(fn, a, "positive")
    a = good(); a.H, a.W = 8192, 4096; _refused(fn, a, "2^24")
    a = good(); a.subsamp = -1; _refused(fn, a, "subsamp")
    for v in (-1, 9):
        a = good(); a.divider = v; _refused(fn, a, "divider")
    for v in (-0.01, 1.01, float("nan")):
        a = good(); a.quantile = v; _refused(fn, a, "quantile")
    for v, word in ((0, "no bit"), (16, "unknown bit"), (_lib.SLAM_MODE_NORM, "NORM goes with NN"), (_lib.SLAM_MODE_NN | _lib.SLAM_MODE_MEANCONF, "exclude"),
                    (_lib.SLAM_MODE_MEANCONF | _lib.SLAM_MODE_MEDIANCONF, "exclude")):
        a = good(); a.mode = v; _refused(fn, a, word)
    a = good(); a.scratch_bytes -= 1; _refused(fn, a, "scratch too small")
    for field in ("sel", "record", "scratch"):
        a = good()
        setattr(a, field, p + 4)
        _refused(fn, a, "8-byte aligned")
