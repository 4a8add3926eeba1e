"""GPU (-m gpu): the exact 1-NN index of the keyframe map (csrc/nn_index.hip, include/must3r_hip.h ABI 12; must3r_amd.slam_nn.BVH_hip /
BVHQuadrant_hip) against the brute force it replaces.  Every distance is compared with torch.equal: the index's contract is the brute
force's fp32 result bit for bit (nn_distances over the map, or QuandrantSearcher over the query's quadrant), +inf for an empty segment
and for a non-finite query."""
import ctypes as C

import numpy as np
import pytest
import torch

from must3r_amd import _lib
from must3r_amd import synthetic as S
from must3r_amd.slam_nn import (BVH_hip, BVHQuadrant_hip, BruteForce_hip, QuandrantSearcher, get_overlap_score, get_searcher,
                                nn_distances)
from test_ops_gpu import record
from util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _plain(db, q):
    tree = BVH_hip()
    if db.shape[0]:
        tree.add_pts(db)
    got = tree.query_device(q)
    ref = nn_distances(db if db.shape[0] else None, q)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert torch.equal(got, ref), (got - ref).abs().max()
    return got


def _quadrant(batches, queries, div):
    """batches / queries: lists of (pts, cam) on the device; the index and QuandrantSearcher fed the same adds, compared per query batch"""
    tree, ref = BVHQuadrant_hip(f"bvh-hip-quadrant_x{div}"), QuandrantSearcher(f"kdtree-scipy-quadrant_x{div}")
    for p, c in batches:
        tree.add_pts(p, cam_center=c)
        ref.add_pts(p, cam_center=c)
    for q, c in queries:
        a, b = tree.query_device(q, cam_center=c), ref.query_device(q, cam_center=c)
        assert torch.equal(a, b), (div, (a - b).abs().max())
    return tree


@pytest.mark.parametrize("shape", [(1, 1), (1000, 1), (1, 1000), (5000, 777), (2049, 4097), (33, 100), (300000, 12288)])
def test_index_equals_brute_force(shape):
    nd, nq = shape
    g = torch.Generator().manual_seed(nd + nq)
    db = (torch.randn((nd, 3), generator=g) * 2.0).to(DEV)
    q = (torch.randn((nq, 3), generator=g) * 2.0).to(DEV)
    if nq > 10:
        q[3] = db[min(5, nd - 1)]                      # exact hit -> distance 0
    d = _plain(db, q)
    if nq > 10:
        assert float(d[3]) == 0.0
    record("nn_index_plain", shape=shape)


def test_index_twenty_million_points():
    g = torch.Generator(device=DEV).manual_seed(7)
    db = torch.rand((20_000_000, 3), generator=g, device=DEV) * 10.0
    q = torch.rand((4096, 3), generator=g, device=DEV) * 12.0 - 1.0
    q[:16] = db[:16 * 997:997]
    d = _plain(db, q)
    assert (d[:16] == 0).all()


def test_index_empty_and_single_point():
    q = torch.randn((17, 3), device=DEV)
    assert torch.isinf(BVH_hip().query_device(q)).all()
    assert np.isposinf(BVH_hip().query(q)).all()
    assert np.isposinf(get_searcher("bvh-hip-quadrant_x2").query(q, cam_center=torch.zeros(3))).all()
    _plain(torch.tensor([[0.5, -1.0, 2.0]], device=DEV), q)
    # through the ABI: a build of zero points, then a query
    lib = _lib.load()
    for div in (0, 2):
        index = torch.empty((lib.must3r_hip_nn_index_bytes(0, div),), dtype=torch.uint8, device=DEV)
        _lib.check(lib.must3r_hip_nn_index_build(None, None, 0, div, index.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
        out = torch.empty((17,), device=DEV)
        cc = (C.c_float * 3)(0.0, 0.0, 0.0)
        _lib.check(lib.must3r_hip_nn_index_query(index.data_ptr(), q.data_ptr(), 17, cc, div, out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream))
        assert torch.isinf(out).all() and (out > 0).all()


@pytest.mark.parametrize("n", [15, 16, 17, 31, 32, 33, 63, 64, 65, 1000, 4097])
def test_index_sizes_not_multiple_of_leaf(n):
    g = torch.Generator().manual_seed(n)
    _plain(torch.randn((n, 3), generator=g).to(DEV), torch.randn((999, 3), generator=g).to(DEV))


def test_index_degenerate_maps():
    g = torch.Generator().manual_seed(3)
    q = torch.randn((3000, 3), generator=g).to(DEV)
    same = torch.tensor([[0.25, -0.5, 1.0]]).repeat(5000, 1).to(DEV)                       # all points identical
    _plain(same, q)
    t = torch.linspace(-3, 3, 7000)
    line = torch.stack([t, 0.5 * t + 1.0, torch.full_like(t, 2.0)], 1).to(DEV)             # zero-extent z axis, points on a line
    _plain(line, q)
    u, v = torch.rand((2, 9000), generator=g) * 4 - 2
    plane = torch.stack([u, v, torch.zeros_like(u)], 1).to(DEV)                             # a plane
    _plain(plane, q)
    axis = torch.stack([torch.zeros_like(t), torch.zeros_like(t), t], 1).to(DEV)            # two zero-extent axes
    _plain(axis, q)


@pytest.mark.parametrize("scale", [1e-6, 1e6])
def test_index_scales(scale):
    g = torch.Generator().manual_seed(int(scale > 1))
    db = torch.randn((20000, 3), generator=g) * scale
    q = torch.randn((5000, 3), generator=g) * scale
    q[:50] = db[:50]
    d = _plain(db.to(DEV), q.to(DEV))
    assert (d[:50] == 0).all()


def test_index_non_finite_entries():
    g = torch.Generator().manual_seed(11)
    db = torch.randn((10000, 3), generator=g)
    db[::7, 0] = float("nan")
    db[3::11, 1] = float("inf")
    db[5::13, 2] = -float("inf")
    q = torch.randn((4000, 3), generator=g)
    q[::5, 1] = float("nan")
    q[1::9, 2] = float("inf")
    q[2::17, 0] = -float("inf")
    d = _plain(db.to(DEV), q.to(DEV))
    assert torch.isinf(d[::5]).all()
    allbad = torch.full((100, 3), float("nan"), device=DEV)                                 # a map of non-finite points only
    _plain(allbad, q.to(DEV))
    for div in (1, 2):
        cam = torch.tensor([0.1, 0.2, -0.3])
        _quadrant([(db.to(DEV), cam)], [(q.to(DEV), cam)], div)


@pytest.mark.parametrize("div", [1, 2, 4])
def test_index_quadrants(div):
    g = torch.Generator().manual_seed(div)
    cam0, cam1 = torch.tensor([0.0, 0.0, 0.0]), torch.tensor([0.5, -0.2, 0.1])
    a = torch.randn((30000, 3), generator=g) * 3.0
    b = torch.rand((8000, 3), generator=g) + torch.tensor([0.5, 0.5, 2.0])                   # one cone of directions: most quadrants empty
    q = torch.randn((12000, 3), generator=g) * 3.0
    q[:100] = a[:100]
    _quadrant([(b.to(DEV), cam1)], [(q.to(DEV), cam0), (q.to(DEV), cam1)], div)              # empty quadrant segments
    _quadrant([(a.to(DEV), cam0), (b.to(DEV), cam1)], [(q.to(DEV), cam0), (q.to(DEV), cam1)], div)


def test_index_divider_zero_is_plain_searcher():
    assert isinstance(get_searcher("bvh-hip"), BVH_hip) and get_searcher("bvh-hip").quadrant_divider == 0
    s = get_searcher("bvh-hip-quadrant_x4")
    assert isinstance(s, BVHQuadrant_hip) and s.quadrant_divider == 4
    assert type(get_searcher("bvh-hip-quadrant_x2", isquadrant=True)) is BVH_hip
    assert isinstance(get_searcher("kdtree-scipy-quadrant_x2"), QuandrantSearcher)                  # unchanged strings
    assert type(get_searcher("kdtree-scipy")) is BruteForce_hip and get_searcher("none") is None


@pytest.mark.parametrize("leaf_log2", [4, 6])
def test_index_leaf_sizes(leaf_log2):
    g = torch.Generator().manual_seed(leaf_log2)
    db, q = torch.randn((50000, 3), generator=g).to(DEV), torch.randn((7000, 3), generator=g).to(DEV)
    try:
        _lib.set_option("NN_LEAF_LOG2", leaf_log2)
        _plain(db, q)
        _quadrant([(db, torch.zeros(3))], [(q, torch.tensor([0.1, 0.0, 0.0]))], 2)
    finally:
        _lib.set_option("NN_LEAF_LOG2", 5)
    with pytest.raises(_lib.HipError):
        _lib.set_option("NN_LEAF_LOG2", 7)


def test_index_rounds_on_overlap_frames():
    """20 interleaved add / query rounds at 384 x 512 (49 152 queries per frame), both forms, against the brute force."""
    frames = S.make_overlap_frames(5, n_kf=19, H=384, W=512)
    for div in (0, 2):
        tree = BVHQuadrant_hip(f"bvh-hip-quadrant_x{div}") if div else BVH_hip()
        ref = QuandrantSearcher(f"kdtree-scipy-quadrant_x{div}") if div else BruteForce_hip()
        for f in frames:
            cam = torch.from_numpy(f["cam"])
            q = torch.from_numpy(f["pts3d"][0, 0, ::2, ::2].reshape(-1, 3)).to(DEV)
            assert torch.equal(tree.query_device(q, cam_center=cam), ref.query_device(q, cam_center=cam))
            sel = torch.from_numpy(f["pts3d"][0, 0][f["conf"][0, 0] > 1.5]).to(DEV)
            tree.add_pts(sel, cam_center=cam)
            ref.add_pts(sel, cam_center=cam)
        record("nn_index_rounds", div=div, map_points=tree.n)


def test_index_build_is_deterministic():
    g = torch.Generator().manual_seed(2)
    db = (torch.randn((300001, 3), generator=g) * 5).to(DEV)
    db[::97, 1] = float("nan")
    cam = torch.tensor([0.3, 0.1, -0.2])
    for div in (0, 2):
        a, b = BVH_hip(div), BVH_hip(div)
        a.add_pts(db, cam_center=cam)
        b.add_pts(db, cam_center=cam)
        a.build()
        torch.cuda.synchronize()
        junk = torch.empty_like(a.index).fill_(0xA5)     # the allocator hands b a buffer holding other bytes
        del junk
        b.build()
        assert a.index.shape == b.index.shape and torch.equal(a.index, b.index)


def test_index_reference_fixture():
    """tests/golden/nn_overlap.npz (the reference's own searchers), at the tolerance of test_nn_gpu.test_overlap_score_reference_fixture."""
    from test_nn_gpu import RTOL, _close
    gold = load_golden("nn_overlap")
    frames = S.make_overlap_frames(7, n_kf=4, H=48, W=64)
    for method, mine in (("kdtree-scipy", "bvh-hip"), ("kdtree-scipy-quadrant_x2", "bvh-hip-quadrant_x2")):
        tree = get_searcher(mine)
        worst_s = worst_d = 0.0
        for i, f in enumerate(frames):
            res = {k: torch.from_numpy(f[k]).to(DEV) for k in ("pts3d", "pts3d_local", "conf")}
            cam = torch.from_numpy(f["cam"])
            for j, m in enumerate(("nn", "nn-norm")):
                sc = float(get_overlap_score(res, tree, cam, mode=m, kf_x_subsamp=2, percentile=70))
                ref = float(gold[method + "/scores"][i][j])
                worst_s = max(worst_s, abs(sc - ref) / max(abs(ref), 1e-30) if np.isfinite(ref) and ref < 1e300 else float(sc != ref))
            d = tree.query(res["pts3d"][0, 0, ::2, ::2].reshape(-1, 3), cam_center=cam)
            worst_d = max(worst_d, _close(d, gold[method + "/dists"][i]))
            tree.add_pts(res["pts3d"][0, 0][res["conf"][0, 0] > 1.5], cam_center=cam)
        record("nn_index_fixture", method=mine, score_rel=worst_s, dist_rel=worst_d)
        assert worst_d < RTOL and worst_s < 1e-5, (mine, worst_s, worst_d)


def test_overlap_score_equal_with_both_searchers():
    frames = S.make_overlap_frames(9, n_kf=8, H=96, W=128)
    for mode in ("nn", "nn-norm"):
        a, b = get_searcher("bvh-hip-quadrant_x2"), get_searcher("kdtree-scipy-quadrant_x2")
        for f in frames:
            res = {k: torch.from_numpy(f[k]).to(DEV) for k in ("pts3d", "pts3d_local", "conf")}
            cam = torch.from_numpy(f["cam"])
            sa = get_overlap_score(res, a, cam, mode=mode, kf_x_subsamp=2)
            sb = get_overlap_score(res, b, cam, mode=mode, kf_x_subsamp=2)
            assert sa == sb, (mode, sa, sb)
            sel = res["pts3d"][0, 0, ::2, ::2][res["conf"][0, 0, ::2, ::2] > 1.5]
            a.add_pts(sel, cam_center=cam)
            b.add_pts(sel, cam_center=cam)


@pytest.mark.parametrize("lanes_log2", [0, 1, 2, 4])
def test_index_query_lanes(lanes_log2):
    """the lanes that walk one query together split the leaves' points; the distances must not depend on how many there are"""
    g = torch.Generator().manual_seed(20 + lanes_log2)
    db, q = torch.randn((60000, 3), generator=g).to(DEV), torch.randn((5001, 3), generator=g).to(DEV)
    q[::11, 2] = float("nan")
    try:
        _lib.set_option("NN_QUERY_LANES_LOG2", lanes_log2)
        _plain(db, q)
        _quadrant([(db, torch.zeros(3))], [(q, torch.tensor([0.2, -0.1, 0.0]))], 4)
    finally:
        _lib.set_option("NN_QUERY_LANES_LOG2", 3)


def test_index_query_with_another_divider_gives_nan():
    lib = _lib.load()
    db, q = torch.randn((5000, 3), device=DEV), torch.randn((300, 3), device=DEV)
    cc = (C.c_float * 3)(0.0, 0.0, 0.0)
    stream = torch.cuda.current_stream().cuda_stream
    for built, asked in ((2, 0), (0, 2), (2, 4)):
        tree = BVH_hip(built)
        tree.add_pts(db, cam_center=torch.zeros(3))
        tree.build()
        out = torch.empty((300,), device=DEV)
        _lib.check(lib.must3r_hip_nn_index_query(tree.index.data_ptr(), q.data_ptr(), 300, cc, asked, out.data_ptr(), stream))
        assert torch.isnan(out).all(), (built, asked)


def test_build_of_an_empty_searcher():
    for tree in (BVH_hip(), get_searcher("bvh-hip-quadrant_x2")):
        tree.build()
        assert not tree.dirty
        assert torch.isinf(tree.query_device(torch.randn((9, 3), device=DEV), cam_center=torch.zeros(3))).all()
