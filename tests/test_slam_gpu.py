"""GPU (-m gpu): the SLAM agent's per-frame step (csrc/slam.hip: must3r_hip_slam_pose, must3r_hip_slam_keyframe) and must3r_amd/slam.py against the yardstick
tests/slam_ref.py (itself held to the reference by tests/test_slam_host.py) and against the already tested pieces of the package: the camera pass of
must3r_hip_postprocess_cam (same launches, so the unrectified outputs and the focal are its bits), the index walk of BVH_hip.query_device, numpy's sort and
percentile on the fp64 values, torch.median on the CPU.

Tolerances.  Focal and pose: F_RTOL and C_ATOL of tests/test_cam_gpu.py, nothing new.  The rectified z against fp64: the ratio seq_focal / focal inherits the
focal's relative error (F_RTOL) and z the activation's (rtol 2e-6, atol 1e-6 in test_cam_gpu._check), so |z - z64| <= (F_RTOL + 2e-6) |z64| + 1e-6; against
the device's own focal it is bit-equal.  Order statistics, n_sel, compaction, distances, conf median: bit-equal.  Score: 1 ulp (fp64) of np.percentile.
Conf mean: H W 2^-24 relative (torch's fp32 mean against the fp64 sum)."""
import time

import numpy as np
import pytest
import torch

import slam_ref as SR
from must3r_amd import slam
from must3r_amd import synthetic as S
from must3r_amd.slam_nn import BVH_hip, get_overlap_score
from oracle import must3r_ref as R
from test_cam_gpu import C_ATOL, F_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
DBL_MAX = np.finfo(np.float64).max


# ---------------------------------------------------------------------------------------------------------------------------------------
# pose
# ---------------------------------------------------------------------------------------------------------------------------------------
def _state(seq):
    st = slam.FocalState()
    st.state = torch.tensor([seq, 1.0, 1.0, seq], dtype=torch.float64, device=DEV)
    return st


@pytest.mark.parametrize("case", ["first", "none", "seq0.8", "seq1.3"])
@pytest.mark.parametrize("H,W", [(32, 48), (48, 32)])
@pytest.mark.parametrize("B", [1, 3])
def test_pose(B, H, W, case):
    from must3r_amd.engine import postprocess
    true_focal = 0.9 * max(H, W)
    pm = S.make_cam_pointmaps(B, H, W, focal=true_focal, noise=0.02, seed=B * 1000 + H)
    first = case == "first"
    seq = float(case[3:]) * true_focal if case.startswith("seq") else None
    base = postprocess(pm.to(DEV), compute_cam=True)            # the camera pass alone: unrectified maps, focal
    out = slam.slam_pose(pm.to(DEV), seq_focals=None if seq is None else _state(seq), is_first_frame=first)
    # the yardstick in fp64 on the CPU activation
    act = R.postprocess(pm)
    res = {k: act[k].double()[None].clone() for k in ("pts3d", "pts3d_local", "conf")}
    c2w64, f64 = SR.get_camera_pose(res, seq, (H, W), is_first_frame=first, c2w_dtype=torch.float64)
    f, c = out["focal"].cpu(), out["c2w"].cpu()
    assert torch.equal(f, base["focal"].cpu()), "the focal is the camera pass's, on the unrectified points"
    ef = float(((f.double() - f64) / f64).abs().max())
    scale = max(1.0, float(c2w64.abs().max()))
    ec = float((c.double() - c2w64).abs().max()) / scale
    print(f"pose B={B} {H}x{W} {case}: focal rel {ef:.2e}, c2w {ec:.2e}")
    assert ef < F_RTOL and ec < C_ATOL, (ef, ec)
    if first:
        assert torch.equal(c, torch.eye(4).expand(B, 4, 4))
    else:
        assert torch.allclose(torch.det(c[:, :3, :3].double()), torch.ones(B, dtype=torch.float64), atol=1e-5)
        assert torch.equal(c[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 4))
    # the maps: the camera pass's bits, z alone rectified
    assert torch.equal(out["pts3d"], base["pts3d"]) and torch.equal(out["conf"], base["conf"])
    assert torch.equal(out["pts3d_local"][..., :2], base["pts3d_local"][..., :2])
    z, z0 = out["pts3d_local"][..., 2].cpu(), base["pts3d_local"][..., 2].cpu()
    if seq is None or first:
        assert torch.equal(z, z0)
    else:
        ratio = torch.tensor(seq, dtype=torch.float64).float() / f          # fp32(fp32(seq_focal) / focal), torch's scalar / tensor
        assert torch.equal(z, z0 * ratio[:, None, None]) and not torch.equal(z, z0)
    z64 = res["pts3d_local"][0, ..., 2]
    assert bool(((z.double() - z64).abs() <= (F_RTOL + 2e-6) * z64.abs() + 1e-6).all())


def test_pose_focal_update_keeps_fp64_sums_and_a_log():
    st = slam.FocalState()
    fs, cs = [], []
    for i in range(3):
        pm = S.make_cam_pointmaps(1, 32, 48, focal=40.0 + 3 * i, noise=0.02, seed=70 + i).to(DEV)
        before = None if st.state is None else st.state.clone()
        out = slam.slam_pose(pm, seq_focals=st, is_first_frame=i == 0, update_focal=True)
        f = out["focal"].cpu().double()[0]
        if i:   # the ratio was formed from the sums BEFORE this frame was added
            from must3r_amd.engine import postprocess
            z0 = postprocess(pm, compute_cam=True)["pts3d_local"][..., 2]
            ratio = (before[0] / before[1]).float().cpu() / out["focal"].cpu()
            assert torch.equal(out["pts3d_local"][..., 2].cpu(), z0.cpu() * ratio)
        fs.append(float(f))
        cs.append(float((out["conf"] - 1.0).double().mean()))
        s = st.state.cpu().numpy()
        fa, ca = np.array(fs), np.array(cs)
        assert s[2] == i + 1 == st.n
        assert np.allclose(s[0], (fa * ca).sum(), rtol=1e-12) and np.allclose(s[1], ca.sum(), rtol=1e-12) and np.allclose(s[3], (fa * ca).sum() / ca.sum(), rtol=1e-12)
    lf, lc = st.read()
    assert np.array_equal(lf, np.array(fs)) and np.allclose(lc, cs, rtol=1e-12)
    assert np.allclose(slam.mean_focal(st), SR.mean_focal({"f": fs, "conf": cs}), rtol=1e-12)
    st.reset()
    assert float(st.state.abs().sum()) == 0 and st.n == 0 and slam.mean_focal(st) is None


# ---------------------------------------------------------------------------------------------------------------------------------------
# keyframe step
# ---------------------------------------------------------------------------------------------------------------------------------------
def _frame(H, W, seed, dups=False):
    """points on rays in EVERY direction around the camera centre (so that some fall in quadrants a one-sided map has no points in), depths in (0.5, 2.5)"""
    g = torch.Generator().manual_seed(seed)
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.3, -0.2, 0.1])
    rays = torch.randn(H, W, 3, generator=g)
    rays = rays / rays.norm(dim=-1, keepdim=True)
    depth = 0.5 + 2 * torch.rand(H, W, generator=g)
    p3 = c2w[:3, 3] + rays * depth[..., None]
    if dups:    # coordinates on a grid of 1/4: equal points, equal distances
        p3 = torch.round(p3 * 4) / 4
    pl = torch.stack((rays[..., 0] * depth, rays[..., 1] * depth, depth), -1)
    cf = 1 + torch.exp(torch.randn(H, W, generator=g))
    return p3.contiguous(), pl.contiguous(), cf.contiguous(), c2w


def _map(n, divider, centre, dups=False):
    """a BVH_hip of n points in the half space x > centre.x (quadrants with phi beyond +-90 degrees stay empty)"""
    tree = BVH_hip(divider)
    if n:
        g = torch.Generator().manual_seed(n)
        pts = torch.randn(n, 3, generator=g)
        pts[:, 0] = pts[:, 0].abs() + 0.05
        pts = pts + centre
        if dups:
            pts = torch.round(pts * 4) / 4 + torch.tensor([0.125, 0.0, 0.0])
        tree.add_pts(pts.to(DEV), cam_center=centre)
    return tree


def _min_conf(cf, s, mask):
    grid = cf[::s, ::s].reshape(-1).sort().values
    if mask == "none":
        return float(grid[-1])                     # conf > max: nothing
    if mask == "one":
        return float(grid[-2])                     # the largest alone
    if mask == "all":
        return float(grid[0]) - 0.5
    return float(grid[len(grid) // 2])


def _keyframe(p3, pl, cf, c2w, tree, mode, sub, min_conf, q):
    sel, record, dist = slam.slam_keyframe(p3.to(DEV), pl.to(DEV), cf.to(DEV), c2w.to(DEV), tree, mode, sub, min_conf, q, want_dist=True)
    return sel, slam.read_record(record), dist


def _check_keyframe(p3, pl, cf, c2w, tree, mode, sub, min_conf, q):
    s = sub if sub else 1
    sel, rec, dist = _keyframe(p3, pl, cf, c2w, tree, mode, sub, min_conf, q)
    msk = cf[::s, ::s] > min_conf
    pts = p3[::s, ::s][msk]
    n = int(msk.sum())
    assert rec[slam.REC["n_sel"]] == n
    assert torch.equal(sel[:n].cpu(), pts), "the compacted points in row-major grid order"
    # conf statistics of the FULL map
    assert np.float32(rec[slam.REC["conf_median"]]) == np.float32(cf.median()) and rec[slam.REC["conf_median"]] == float(cf.median())
    mean64 = float(cf.double().mean())
    assert abs(rec[slam.REC["conf_mean"]] - mean64) <= cf.numel() * 2.0 ** -24 * abs(mean64)
    assert abs(rec[slam.REC["conf_mean"]] - float(cf.mean())) <= cf.numel() * 2.0 ** -24 * abs(mean64)
    assert np.array_equal(rec[slam.REC["c2w"]], c2w.double().reshape(-1).numpy()) and np.array_equal(rec[slam.REC["cam_center"]], c2w[:3, 3].double().numpy())
    if n == 0:
        assert rec[slam.REC["score"]] == 0 and rec[slam.REC["below"]] == 0 and rec[slam.REC["above"]] == 0
        return rec, np.zeros(0)
    # the distances: the tested query on the same points and the same camera centre
    want = tree.query_device(pts.to(DEV), cam_center=c2w[:3, 3])
    assert torch.equal(dist[:n], want)
    depths = pl[::s, ::s, 2][msk].numpy() if "norm" in mode else None
    vals = SR.overlap_values(want.double().cpu().numpy(), depths)
    srt = np.sort(vals)
    vi = (n - 1) * (q / 100.0)
    lo, hi = (n - 1, n - 1) if vi >= n - 1 else (int(np.floor(vi)), int(np.floor(vi)) + 1)
    assert rec[slam.REC["virtual_index"]] == vi
    assert rec[slam.REC["below"]].tobytes() == srt[lo].tobytes() and rec[slam.REC["above"]].tobytes() == srt[hi].tobytes(), (rec[1:3], srt[lo], srt[hi])
    score = float(np.percentile(vals, q))
    assert abs(rec[slam.REC["score"]] - score) <= np.spacing(abs(score)), (rec[slam.REC["score"]], score)
    return rec, vals


@pytest.mark.parametrize("mask", ["none", "one", "all", "half"])
@pytest.mark.parametrize("n_map,divider", [(0, 2), (1, 0), (1, 2), (5000, 0), (5000, 2)])
@pytest.mark.parametrize("H,W,sub", [(32, 48, 4), (32, 48, 2), (48, 64, 0)])
def test_keyframe_step(H, W, sub, n_map, divider, mask):
    dups = mask == "half"
    p3, pl, cf, c2w = _frame(H, W, seed=H + (sub or 0), dups=dups)
    tree = _map(n_map, divider, c2w[:3, 3], dups=dups)
    min_conf = _min_conf(cf, sub if sub else 1, mask)
    for mode in ("nn-norm", "nn"):
        for q in (0, 70, 85, 100):
            rec, vals = _check_keyframe(p3, pl, cf, c2w, tree, mode, sub, min_conf, q)
    n = int(rec[slam.REC["n_sel"]])
    assert n == {"none": 0, "one": 1, "all": slam.candidates(H, W, sub)}.get(mask, n) and (mask != "half" or 0 < n < slam.candidates(H, W, sub))
    if n > 1:
        if n_map == 0:
            assert bool((vals == DBL_MAX).all()), "an empty map: every distance is the largest fp64"
        elif divider == 2 and n_map > 1:
            assert bool((vals == DBL_MAX).any()) and bool((vals < DBL_MAX).any()), "rays in quadrants the map has no points in"
        if dups and n_map > 1:
            fin = vals[vals < DBL_MAX]
            assert len(np.unique(fin)) < len(fin), "duplicate distances"


@pytest.mark.parametrize("mode", ["meanconf", "medianconf"])
def test_keyframe_conf_modes(mode):
    p3, pl, cf, c2w = _frame(32, 48, seed=9)
    sel, rec, _ = _keyframe(p3, pl, cf, c2w, None, mode, 4, 1.5, 70)
    msk = cf[::4, ::4] > 1.5
    assert rec[slam.REC["n_sel"]] == int(msk.sum()) and torch.equal(sel[:int(msk.sum())].cpu(), p3[::4, ::4][msk])
    assert rec[slam.REC["score"]] == rec[slam.REC["conf_mean" if mode == "meanconf" else "conf_median"]]
    assert rec[slam.REC["conf_median"]] == float(cf.median())
    ref = {k: v[None, None] for k, v in (("pts3d", p3), ("pts3d_local", pl), ("conf", cf))}
    assert abs(rec[slam.REC["score"]] - float(SR.get_overlap_score(ref, None, None, mode=mode))) <= cf.numel() * 2.0 ** -24 * rec[slam.REC["score"]]


def test_keyframe_bits_do_not_depend_on_the_frame_before():
    """a frame alone, after another frame, and again: the same record, points and distances, bit for bit"""
    A, B = _frame(32, 48, seed=1), _frame(32, 48, seed=2)
    tree = _map(5000, 2, A[3][:3, 3])

    def run(f, sub, q):
        sel, rec, dist = _keyframe(*f, tree, "nn-norm", sub, 1.8, q)
        n = int(rec[0])
        return rec.tobytes(), sel[:n].cpu().numpy().tobytes(), dist[:n].cpu().numpy().tobytes()
    alone = run(A, 2, 85)
    other = run(B, 2, 70)
    assert other != alone
    run(B, 0, 100)
    assert run(A, 2, 85) == alone and run(A, 2, 85) == alone and run(B, 2, 70) == other


# ---------------------------------------------------------------------------------------------------------------------------------------
# stream order
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stream_inputs(seed):
    return {"pm": S.make_cam_pointmaps(1, 32, 48, focal=40.0 + seed, noise=0.02, seed=seed).to(DEV),
            "state": torch.tensor([41.0 + seed, 1.0, 1.0, 41.0 + seed], dtype=torch.float64, device=DEV)}


def _stream_call(bufs, tree):
    st = slam.FocalState()
    st.state, st.log, st.n = bufs["state"], bufs["log"], 1
    out = slam.slam_pose(bufs["pm"], seq_focals=st, update_focal=True)
    sel, record, dist = slam.slam_keyframe(out["pts3d"][0], out["pts3d_local"][0], out["conf"][0], out["c2w"][0], tree, "nn-norm", 2, 1.5, 85.0,
                                           out["focal"], st, want_dist=True)
    return [out["pts3d"], out["pts3d_local"], out["conf"], out["focal"], out["c2w"], record, bufs["state"], bufs["log"][:2]]


def test_entry_points_run_on_the_descriptors_stream():
    """the protocol of tests/test_train_data_gpu.py::test_ground_truth_runs_on_the_descriptors_stream for must3r_hip_slam_pose (with its focal update) and
    must3r_hip_slam_keyframe: enqueued behind a delay on a side stream they return while the delay is running and give the default-stream bits"""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay, null_stream
    delay = Delay()
    src = {"A": _stream_inputs(31), "B": _stream_inputs(32)}
    bufs = {k: torch.empty_like(v) for k, v in src["A"].items()}
    bufs["log"] = torch.zeros((64, 2), dtype=torch.float64, device=DEV)
    tree = _map(5000, 2, torch.zeros(3))
    tree.build()
    torch.cuda.synchronize()

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = _stream_call(bufs, tree)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        ref[which] = [t.clone() for t in outs]
    assert all(not torch.equal(a, b) for a, b in zip(ref["A"], ref["B"]))
    ms = min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)
    assert ms < DELAY_CAP_MS or host_ms < DELAY_CAP_MS / 10
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")
        t0 = time.perf_counter()
        outs = _stream_call(bufs, tree)
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in outs]
        load("B")
    s.synchronize()
    print(f"slam step: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the calls took {side_ms:.3f} ms on the host)"
    for i, (g, r) in enumerate(zip(got, ref["A"])):
        assert torch.equal(g, r), f"output {i}: on a side stream the bits differ from the default-stream bits (equal to the decoy's: {torch.equal(g, ref['B'][i])})"
    # control: with the null stream in the descriptors the calls run on the null stream and see the decoy
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")                         # queued behind the delay: the inputs still hold the decoy
        with torch.cuda.stream(torch.cuda.default_stream()), null_stream():
            outs = _stream_call(bufs, tree)
            torch.cuda.default_stream().synchronize()
            got = [t.clone() for t in outs]
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"the delay ({ms:.1f} ms) ended before the null stream was idle"
    for i, (g, r) in enumerate(zip(got, ref["B"])):
        assert torch.equal(g, r), f"output {i}: with the null stream the call did not run on the null stream"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the agent end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
# The camera of e2e_scene moves 0.3 a frame over a surface 3 away: in the comparison form a frame one step from the last keyframe scores about 0.07, one two
# steps away about 0.15 (85th percentile of distance / depth at subsample 2).  The threshold lies between the two; the test asserts the margin.
E2E = dict(seed=3, n_frames=8, kf_x_subsamp=2, overlap_percentile=85.0, min_conf_keyframe=1.2, keyframe_overlap_thr=0.1, num_init_frames=2)


def e2e_frames(seed, n):
    """n uint8 RGB frames of 48 x 64: a smooth pattern drifting with the frame index, plus noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:48, 0:64].astype(np.float32)
    out = []
    for t in range(n):
        base = 127 + 90 * np.stack([np.sin(0.2 * xx + 0.7 * t), np.cos(0.15 * yy - 0.5 * t), np.sin(0.1 * (xx + yy) + 1.3 * t)], -1)
        out.append(np.clip(base + 25 * rng.standard_normal((48, 64, 3)), 0, 255).astype(np.uint8))
    return out


def e2e_scene(seed, n):
    """raw head outputs [1, 1, 48, 64, 7] of n frames of synthetic.make_overlap_frames: a wavy surface seen from a camera that moves 0.3 a frame"""
    def inv_norm_exp(p):   # raw v with v / |v| * expm1(|v|) = p
        d = p.norm(dim=-1, keepdim=True)
        return p / d.clip(min=1e-8) * torch.log1p(d)
    out = []
    for f in S.make_overlap_frames(seed, n_kf=n - 1, H=48, W=64):
        p3, pl, cf = (torch.from_numpy(f[k])[0, 0] for k in ("pts3d", "pts3d_local", "conf"))
        out.append(torch.cat((inv_norm_exp(p3), inv_norm_exp(pl), torch.log(cf - 1)[..., None]), -1)[None, None])
    return out


def run_e2e(cfg, sync_debug=False):
    """Drives SLAM_MUSt3R over the frames with the tiny modules (preprocessing, encoder, decoder and memory run as they are).  With their random weights the
    head output is noise: the focal is then a cancellation near zero and seq_focal / focal amplifies its last bits, so no pose tolerance could hold.  The
    prediction a frame step sees is therefore a synthetic pinhole sequence (``e2e_scene``) plus 1 % of the model's own head output, which keeps the
    dependence on the adopted memory.  Beside every native frame step the COMPARISON FORM is evaluated on the same raw prediction, from existing package
    functions: engine.postprocess (activation), the yardstick's get_camera_pose in fp64 on the CPU with its own running focal lists (pose, rectified depth),
    slam_nn.get_overlap_score on its own BVH_hip map with the DEVICE's camera centre (so that a quadrant boundary cannot flip a decision through a 1e-6
    pose difference), the reference's decision rule.  -> (agent, rows), a row per frame step."""
    from must3r_amd.engine import postprocess
    from stream_forms import tiny_modules
    agent = slam.SLAM_MUSt3R(tiny_modules(), res=64, kf_x_subsamp=cfg["kf_x_subsamp"], keyframe_overlap_thr=cfg["keyframe_overlap_thr"],
                             min_conf_keyframe=cfg["min_conf_keyframe"], overlap_percentile=cfg["overlap_percentile"], num_init_frames=cfg["num_init_frames"],
                             device=DEV)
    cmp_state = {"tree": None, "seq": {"f": [], "conf": []}}
    scene = [r.to(DEV) for r in e2e_scene(cfg["seed"], cfg["n_frames"])]
    rows, reads = [], [0]
    native_reset, native_step, native_read, native_forward = agent.reset, agent.frame_step, agent.read_record, agent.forward

    def reset():
        native_reset()
        cmp_state["tree"] = slam.slam_searcher(agent.searcher)
        cmp_state["seq"] = {"f": [], "conf": []}
    cmp_state["tree"] = slam.slam_searcher(agent.searcher)

    def read_record(record):
        reads[0] += 1
        if sync_debug:
            torch.cuda.set_sync_debug_mode("default")
        try:
            return native_read(record)
        finally:
            if sync_debug:
                torch.cuda.set_sync_debug_mode("error")

    def forward(views, memory, render=False):
        if sync_debug:
            torch.cuda.set_sync_debug_mode("default")
        try:
            preds, newmem = native_forward(views, memory, render)
            for v, p in zip(views, preds):
                p["pointmaps"] = scene[int(v["idx"])] + 0.01 * p["pointmaps"]
            return preds, newmem
        finally:
            if sync_debug:
                torch.cuda.set_sync_debug_mode("error")   # everything between the decoder call and the end of __call__, the one read excepted

    def frame_step(ag, view, pred, is_first, to_orig):
        out = native_step(ag, view, pred, is_first, to_orig)
        if sync_debug:
            rows.append(dict(iskf=bool(out[8])))
            return out
        rec = out[9]
        H, W = (int(v) for v in view["true_shape"][0])
        act = postprocess(pred["pointmaps"].reshape(1, 1, H, W, 7))
        res64 = {k: act[k].double().cpu().clone() for k in ("pts3d", "pts3d_local", "conf")}
        seq = cmp_state["seq"]
        c2w64, f64 = SR.get_camera_pose(res64, SR.mean_focal(seq), (H, W), is_first_frame=is_first, c2w_dtype=torch.float64)
        res = {"pts3d": act["pts3d"], "conf": act["conf"], "pts3d_local": res64["pts3d_local"].float().to(DEV)}
        dev_centre = torch.tensor(rec[slam.REC["cam_center"]], dtype=torch.float32)
        score = float(get_overlap_score(res, cmp_state["tree"], dev_centre, mode="nn-norm", kf_x_subsamp=cfg["kf_x_subsamp"],
                                        min_conf_keyframe=cfg["min_conf_keyframe"], percentile=cfg["overlap_percentile"]))
        median_ok = bool(act["conf"].median() > cfg["min_conf_keyframe"])
        iskf = bool(is_first or (score > cfg["keyframe_overlap_thr"] and median_ok))
        seq["f"].append(float(f64[0]))
        seq["conf"].append(float(act["conf"].double().mean()) - 1.0)
        if iskf:
            s = cfg["kf_x_subsamp"]
            msk = act["conf"][0, 0, ::s, ::s] > cfg["min_conf_keyframe"]
            cmp_state["tree"].add_pts(act["pts3d"][0, 0, ::s, ::s][msk], cam_center=dev_centre)
        rows.append(dict(frame=int(view["idx"]), first=bool(is_first), score=score, native_score=float(rec[slam.REC["score"]]), iskf=iskf, native_iskf=bool(out[8]),
                         median_ok=median_ok, c2w64=c2w64[0], native_c2w=torch.from_numpy(rec[slam.REC["c2w"]].reshape(4, 4).copy()),
                         f64=float(f64[0]), native_f=float(rec[slam.REC["focal"]]), map=cmp_state["tree"].n, native_map=None))
        return out
    agent.reset, agent.frame_step, agent.read_record, agent.forward = reset, frame_step, read_record, forward
    steps = []
    try:
        for t, img in enumerate(e2e_frames(cfg["seed"], cfg["n_frames"])):
            before = len(rows)
            agent(img, t, 0, device_outputs=True)
            steps.append(len(rows) - before)
            if rows and "map" in rows[-1]:
                rows[-1]["native_map"] = agent.overlap_tree.n
    finally:
        if sync_debug:
            torch.cuda.set_sync_debug_mode("default")
    return agent, rows, reads[0], steps, cmp_state


def test_agent_end_to_end_equals_the_comparison_form():
    cfg = E2E
    agent, rows, reads, steps, cmp_state = run_e2e(cfg)
    thr = cfg["keyframe_overlap_thr"]
    for r in rows:
        print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items() if k not in ("c2w64", "native_c2w")})
    # the condition on the inputs, in the comparison form alone
    assert all(r["first"] or abs(r["score"] - thr) > 1e-6 * max(1.0, abs(r["score"])) for r in rows)
    later = [r for r in rows if not r["first"]]
    assert any(r["iskf"] for r in later) and any(not r["iskf"] for r in later), "the list must hold keyframes and non-keyframes"
    assert all(r["median_ok"] for r in rows), "the decisions of this test rest on the score"
    # the agent
    assert [r["native_iskf"] for r in rows] == [r["iskf"] for r in rows]
    assert agent.overlap_tree.n == cmp_state["tree"].n > 0
    for r in rows:
        scale = max(1.0, float(r["c2w64"].abs().max()))
        assert float((r["native_c2w"] - r["c2w64"]).abs().max()) / scale < C_ATOL, r["frame"]
        assert abs(r["native_f"] - r["f64"]) / r["f64"] < F_RTOL
    assert reads == len(rows) == sum(steps) and steps == [1, 2] + [1] * (cfg["n_frames"] - 2), "one read per frame step; frame 1 re-runs frame 0 (num_init_frames = 2)"
    assert agent.all_timestamps == list(range(cfg["n_frames"])) and len(agent.all_poses) == cfg["n_frames"]
    assert agent.keyframes == sorted({r["frame"] for r in rows[1:] if r["iskf"]})
    focals = agent.get_true_focals()[0]
    assert abs(focals - SR.mean_focal(cmp_state["seq"])) / focals < F_RTOL


def sync_debug_detects_item():
    """does this torch build flag a plain .item() under set_sync_debug_mode("error")?"""
    x = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_one_read_per_frame_and_no_other_synchronisation():
    """all host reads of the loop go through SLAM_MUSt3R.read_record: one call per frame step.  Where this torch build flags synchronising calls, everything
    between the decoder call and the end of __call__ (the frame steps, the map update, the index rebuild) also runs under
    torch.cuda.set_sync_debug_mode("error"), the one read excepted."""
    detects = sync_debug_detects_item()
    print(f"set_sync_debug_mode('error') flags .item(): {detects}")
    agent, rows, reads, steps, _ = run_e2e(E2E, sync_debug=detects)
    assert reads == len(rows) == sum(steps) == E2E["n_frames"] + 1
