"""CPU: the yardstick of the ground-truth kernel (tests/train_data_ref.py) against its own fp64 form and against synthetic.SyntheticScenes, the meaning of the
orientation flag, the ABI surface of must3r_hip_gt_from_depth, and the host side of must3r_amd/train_data.py (collate_views, SyntheticDepthScenes)."""
import ctypes as C
import os
import re

import pytest
import torch
from torch.utils.data import DataLoader

import train_data_ref as DR
from conftest import ROOT
from must3r_amd import _lib, synthetic as S, train_data as TD


def _stack(ds, idx, key):
    return torch.stack([v[key] for v in ds[idx]])


def _scene(ds, idx):
    return _stack(ds, idx, "depthmap"), _stack(ds, idx, "camera_intrinsics"), _stack(ds, idx, "camera_pose")


def test_fp32_yardstick_is_within_the_rounding_bound_of_the_fp64_one():
    ds = TD.SyntheticDepthScenes(2, 4, 48, 80, seed=3, portrait_every=2)
    worst = 0.0
    for idx in range(2):
        depth, K, pose = _scene(ds, idx)
        flags = torch.tensor([ds.is_portrait(v) for v in range(4)])
        p32, v32, s32, n32, cam = DR.gt_from_depth(depth, K, pose, flags)
        p64, v64, s64, n64, _ = DR.gt_from_depth(depth, K, pose, flags, dtype=torch.float64)
        assert p32.dtype == torch.float32 and p64.dtype == torch.float64
        assert torch.equal(v32, v64) and torch.equal(s32, s64) and torch.equal(n32, n64)
        ratio = (p32.double() - p64).abs() / DR.bound(pose, cam)
        worst = max(worst, float(ratio.max()))
    print(f"fp32 yardstick against fp64: worst error {worst:.3f} of the bound")
    assert worst <= 1.0


def test_the_two_synthetic_classes_show_the_same_scenes():
    a = S.SyntheticScenes(2, 3, 32, 48, seed=5)
    b = TD.SyntheticDepthScenes(2, 3, 32, 48, seed=5)
    worst = 0.0
    for idx in range(2):
        depth, K, pose = _scene(b, idx)
        pts, valid, sky, n_valid, cam = DR.gt_from_depth(depth, K, pose)
        lim = DR.bound(pose, cam)
        for v, (va, vb) in enumerate(zip(a[idx], b[idx])):
            for key in ("img", "true_shape", "camera_pose", "is_metric_scale"):
                assert torch.equal(va[key], vb[key]), key
            assert torch.equal(va["valid_mask"], valid[v]) and torch.equal(va["sky_mask"], sky[v])
            assert int(n_valid[v]) == int(va["valid_mask"].sum())
            m = va["valid_mask"]
            ratio = (pts[v][m].double() - va["pts3d"][m].double()).abs() / lim[v][m]
            worst = max(worst, float(ratio.max()))
    print(f"yardstick on SyntheticDepthScenes against SyntheticScenes' pts3d: worst difference {worst:.3f} of the bound")
    assert worst <= 1.0


def test_a_flagged_view_is_the_unflagged_call_on_the_transposed_depth_swapped_back():
    ds = TD.SyntheticDepthScenes(1, 3, 32, 48, seed=7, portrait_every=3)
    depth, K, pose = _scene(ds, 0)
    assert [ds.is_portrait(v) for v in range(3)] == [False, False, True] and ds[0][2]["true_shape"].tolist() == [48, 32]
    assert float(K[2, 0, 2]) == 16.0 and float(K[2, 1, 2]) == 24.0            # the true image is 48 high and 32 wide
    pts, valid, sky, n_valid, _ = DR.gt_from_depth(depth, K, pose, torch.tensor([0, 0, 1]))
    ptsT, validT, skyT, n_validT, _ = DR.gt_from_depth(depth[2:].swapaxes(1, 2).contiguous(), K[2:], pose[2:])
    assert torch.equal(pts[2], ptsT[0].swapaxes(0, 1)) and torch.equal(valid[2], validT[0].T) and torch.equal(sky[2], skyT[0].T)
    assert torch.equal(n_valid[2:], n_validT)
    plain = DR.gt_from_depth(depth, K, pose)[0]
    assert torch.equal(plain[:2], pts[:2]) and not torch.equal(plain[2], pts[2])


def test_uint16_form_of_the_yardstick():
    raw = torch.tensor([[[0, 1, 1000, 65535]]], dtype=torch.uint16)
    z = DR.depth_values(raw, torch.tensor([[1000.0, 1.0]]))
    assert z.dtype == torch.float32 and z.flatten().tolist() == [0.0, float(torch.tensor(1.0) / 1000.0), 1.0, float(torch.tensor(65535.0) / 1000.0)]
    z = DR.depth_values(raw, torch.tensor([[65535.0, 20.0]]))
    assert float(z[0, 0, 3]) == 20.0
    ds = TD.SyntheticDepthScenes(1, 2, 16, 32, seed=1, raw_depth=True)
    v = ds[0][0]
    assert v["depthmap"].dtype == torch.uint16 and v["depth_scale"].tolist() == [1000.0, 1.0]
    assert not bool(DR.gt_from_depth(v["depthmap"][None], v["camera_intrinsics"][None], v["camera_pose"][None], None, v["depth_scale"][None])[2].any())


# ---------------------------------------------------------------------------------------------------------------------------------
# the ABI surface
# ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        return f.read()


def test_abi_surface_of_gt_from_depth():
    name = "must3r_hip_gt_from_depth"
    assert _lib.ABI_VERSION == 21 and re.search(r"#define\s+MUST3R_HIP_ABI_VERSION\s+21\b", _header())
    assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == (C.c_int, [C.POINTER(_lib.GtArgs)])
    fn = getattr(_lib.load(), name)
    assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == C.c_int
    h = _header()
    assert re.search(r"\bint\s+must3r_hip_gt_from_depth\s*\(\s*const\s+must3r_hip_gt_args\s*\*\s*a\s*\)\s*;", h)
    body = re.search(r"typedef struct must3r_hip_gt_args \{(.*?)\} must3r_hip_gt_args;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [first.split()[-1].lstrip("*")] + [r.strip() for r in rest]
    assert fields == [n for n, _ in _lib.GtArgs._fields_]
    assert int(re.search(r"#define\s+MUST3R_GT_VIEW_BLOCKS\s+(\d+)", h).group(1)) == _lib.GT_VIEW_BLOCKS
    assert C.sizeof(_lib.GtArgs) == 10 * 8 + 8 + 4 * 4 + 8
    with open(os.path.join(ROOT, "must3r_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS\s*=.*\btrain_data\.hip\b", mk, flags=re.M) and re.search(r"^build/train_data\.o: FLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    with open(os.path.join(ROOT, "must3r_amd", "csrc", "train_data.hip")) as f:
        assert 'extern "C" int must3r_hip_gt_from_depth(' in f.read()


def test_gt_from_depth_refuses_before_touching_anything():
    lib = _lib.load()
    assert lib.must3r_hip_gt_from_depth(None) != 0 and "null" in lib.must3r_hip_last_error().decode()
    buf = (C.c_float * 64)()
    a = _lib.GtArgs()
    a.depth = a.K = a.c2w = a.pts3d = C.addressof(buf)
    a.V, a.Hs, a.Ws = 1, 4, 6
    assert lib.must3r_hip_gt_from_depth(C.byref(a)) != 0 and "multiple of 4" in lib.must3r_hip_last_error().decode()
    a.Ws = 4
    a.depth_u16 = 1
    assert lib.must3r_hip_gt_from_depth(C.byref(a)) != 0 and "depth_scale" in lib.must3r_hip_last_error().decode()
    a.depth_u16 = 0
    a.pts3d = None
    assert lib.must3r_hip_gt_from_depth(C.byref(a)) != 0 and "one output" in lib.must3r_hip_last_error().decode()
    a.n_valid = C.addressof(buf)
    a.scratch, a.scratch_bytes = C.addressof(buf), 4 * _lib.GT_VIEW_BLOCKS - 4
    assert lib.must3r_hip_gt_from_depth(C.byref(a)) != 0 and "scratch" in lib.must3r_hip_last_error().decode()
    a.n_valid, a.pts3d = None, C.addressof(buf) + 4
    assert lib.must3r_hip_gt_from_depth(C.byref(a)) != 0 and "aligned" in lib.must3r_hip_last_error().decode()
    with pytest.raises(RuntimeError, match="no CPU path"):
        TD.ground_truth(torch.zeros(1, 1, 16, 16), torch.eye(3).view(1, 1, 3, 3), torch.eye(4).view(1, 1, 4, 4), torch.tensor([[[16, 16]]]))


# ---------------------------------------------------------------------------------------------------------------------------------
# collate_views
# ---------------------------------------------------------------------------------------------------------------------------------
def _cpu_kernel(depth, K, c2w, transposed=None, depth_scale=None, want=(True, True, True), count=False):
    pts, valid, sky, n_valid, _ = DR.gt_from_depth(depth, K, c2w, transposed, depth_scale)
    return pts, valid.to(torch.uint8), sky.to(torch.uint8), n_valid.to(torch.int32) if count else None


@pytest.fixture
def on_cpu(monkeypatch):
    """must3r_amd.train_data with the yardstick in the kernel's place, so that the host side runs here"""
    monkeypatch.setattr(TD, "gt_from_depth", _cpu_kernel)
    monkeypatch.setattr(TD, "_dev", lambda t, what: t)


def _batch(ds, B):
    return next(iter(DataLoader(ds, batch_size=B)))


def test_collate_views_of_a_depth_batch(on_cpu):
    ds = TD.SyntheticDepthScenes(2, 4, 32, 48, seed=9, portrait_every=3, uint8_img=True, memory_num_views=2)
    batch = _batch(ds, 2)
    assert len(batch) == 4 and batch[0]["img"].shape == (2, 3, 32, 48) and batch[0]["img"].dtype == torch.uint8 and "pts3d" not in batch[0]
    imgs, ts, gt = TD.collate_views(batch, "cpu")
    assert imgs.shape == (2, 4, 3, 32, 48) and imgs.dtype == torch.float32 and ts.shape == (2, 4, 2)
    assert ts[:, 2].tolist() == [[48, 32]] * 2 and ts[:, 0].tolist() == [[32, 48]] * 2
    assert torch.equal(imgs, (torch.stack([b["img"] for b in batch], dim=1).float() / 255 - 0.5) / 0.5) and float(imgs.min()) >= -1 and float(imgs.max()) <= 1
    exact = TD.collate_views(_batch(TD.SyntheticDepthScenes(2, 4, 32, 48, seed=9, portrait_every=3), 2), "cpu")[0]
    assert float((imgs - exact).abs().max()) <= 1 / 255 + 1e-6
    depth = torch.stack([b["depthmap"] for b in batch], dim=1)
    K, pose = (torch.stack([b[k] for b in batch], dim=1) for k in ("camera_intrinsics", "camera_pose"))
    pts, valid, sky, _ = DR.batched(depth, K, pose, ts)
    assert len(gt) == 4
    for i, g in enumerate(gt):
        assert set(g) == set(TD.GT_KEYS)
        assert g["pts3d"].shape == (2, 32, 48, 3) and g["valid_mask"].shape == g["sky_mask"].shape == (2, 32, 48)
        assert g["valid_mask"].dtype == g["sky_mask"].dtype == torch.bool and g["camera_pose"].shape == (2, 4, 4) and g["true_shape"].shape == (2, 2)
        assert torch.equal(g["pts3d"], pts[:, i]) and torch.equal(g["valid_mask"], valid[:, i]) and torch.equal(g["sky_mask"], sky[:, i])
        assert torch.equal(g["camera_pose"], pose[:, i]) and g["is_metric_scale"].tolist() == [True, True] and g["memory_num_views"].tolist() == [2, 2]
        assert not g["is_metric_scale"].is_cuda and g["pts3d"]._base is not None           # a view of the batched tensor
    assert int(gt[0]["memory_num_views"][0]) == 2


def test_collate_views_passes_a_reference_batch_through():
    batch = _batch(S.SyntheticScenes(2, 3, 32, 48, seed=4), 2)
    imgs, ts, gt = TD.collate_views(batch, "cpu")
    assert gt is batch and imgs.shape == (2, 3, 3, 32, 48) and torch.equal(imgs[:, 1], batch[1]["img"]) and ts.shape == (2, 3, 2)
    with pytest.raises(KeyError, match="depthmap"):
        TD.collate_views([{k: v for k, v in b.items() if k != "pts3d"} for b in batch], "cpu")
    with pytest.raises(ValueError):
        TD.collate_views([], "cpu")


def test_uint16_batches_collate(on_cpu):
    batch = _batch(TD.SyntheticDepthScenes(3, 1, 16, 32, seed=2, raw_depth=True), 3)
    assert batch[0]["depthmap"].dtype == torch.uint16 and batch[0]["depth_scale"].shape == (3, 2)
    _, _, gt = TD.collate_views(batch, "cpu")
    assert not bool(gt[0]["sky_mask"].any()) and bool(gt[0]["valid_mask"].any())
    z = DR.depth_values(batch[0]["depthmap"], batch[0]["depth_scale"])
    assert torch.equal(gt[0]["valid_mask"], z > 0)
