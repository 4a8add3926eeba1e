"""CPU: the oracle restatement (oracle/must3r_ref.py) against fixtures produced by the REAL reference
(oracle/make_golden.py), and the structural invariants of SURVEY.md section 4."""
import numpy as np
import pytest
import torch

from oracle import must3r_ref as R
from must3r_amd.config import TINY, SMALL, MUST3R_224
from must3r_amd import synthetic as S
from util import load_golden, rel_inf

# must3r224_v10 = BASELINE.json configs[1] at full depth (10 views, [2,1,...,1]); the 20-view 384x512 fixture
# (must3r512_v20, configs[2]) costs ~90 s of CPU per pass: the oracle is pinned on it by bench.py's cpu_baseline leg
# (oracle/cpu_baseline.py --check-fixture) on every `bench.py --full` run instead of here.
CASES = {"tiny_48x64_v4": TINY, "small_224_v3": SMALL, "must3r224_v2": MUST3R_224, "must3r224_v10": MUST3R_224}


def _scene(cfg, g):
    H, W, V, ps, tks = (int(v) for v in g["meta"][:5])
    mb = [int(v) for v in g["meta"][5:]]
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    imgs, ts = S.make_images(V, H, W, 0)
    with torch.no_grad():
        x, pos = R.encoder_forward(sde, cfg, imgs, ts, sdpa=True)
        mem, upd, i = None, [], 0
        for nb in mb:
            mem, pm = R.decoder_forward(sdd, cfg, x[i:i + nb].unsqueeze(0), pos[i:i + nb].unsqueeze(0), ts[i:i + nb].unsqueeze(0),
                                        mem, False, "kv", sdpa=True)
            upd.append(pm[0])
            i += nb
        _, ren = R.decoder_forward(sdd, cfg, x.unsqueeze(0), pos.unsqueeze(0), ts.unsqueeze(0), mem, True, "kv", sdpa=True)
    return x, pos, torch.cat(upd, 0), ren[0], mem, ps, tks


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_matches_reference_fixture(name):
    torch.set_num_threads(8)
    g = load_golden(name)
    x, pos, upd, ren, mem, ps, tks = _scene(CASES[name], g)
    tol = 2e-5  # fp32 round-off (different summation order / SDPA backend), observed ~1e-6
    assert rel_inf(x[:, ::tks, ::tks], g["x"]) < tol
    assert abs(x.double().abs().sum().item() - float(g["x_abs"])) / float(g["x_abs"]) < 1e-5
    assert np.array_equal(pos[:, ::tks].numpy(), g["pos"])
    assert rel_inf(upd[:, ::ps, ::ps], g["update"]) < tol
    assert rel_inf(ren[:, ::ps, ::ps], g["render"]) < tol
    assert abs(ren.double().abs().sum().item() - float(g["render_abs"])) / float(g["render_abs"]) < 1e-5
    assert rel_inf(mem[0][0][0, ::tks, ::tks], g["mem_first"]) < tol
    assert rel_inf(mem[0][-1][0, ::tks, ::tks], g["mem_last"]) < tol
    assert np.array_equal(mem[1].numpy(), g["labels"])          # invariant 4: labels
    assert [int(v) for v in mem[2:]] == [int(v) for v in g["tail"]]


def test_oracle_mixed_aspect_ratio_list_path():
    g = load_golden("tiny_mixed_ar")
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    ia, ta = S.make_images(2, 48, 64, 1)
    ib, tb = S.make_images(1, 32, 64, 2)
    L = lambda *t: [v.unsqueeze(0) for v in t]  # noqa: E731
    with torch.no_grad():
        xa, pa = R.encoder_forward(sde, cfg, ia, ta)
        xb, pb = R.encoder_forward(sde, cfg, ib, tb)
        mem, pm0 = R.decoder_forward(sdd, cfg, L(xa, xb), L(pa, pb), L(ta, tb), None)
        mem2, pm1 = R.decoder_forward(sdd, cfg, L(xb, xa), L(pb, pa), L(tb, ta), mem)
        _, pm2 = R.decoder_forward(sdd, cfg, L(xb, xa), L(pb, pa), L(tb, ta), mem2, render=True)
    for got, key in ((pm0[0], "init_a"), (pm0[1], "init_b"), (pm1[0], "upd_b"), (pm1[1], "upd_a"), (pm2[0], "ren_b"),
                     (pm2[1], "ren_a")):
        assert rel_inf(got[0], g[key]) < 2e-5, key
    assert rel_inf(mem2[0][-1][0], g["mem_last"]) < 2e-5
    assert np.array_equal(mem2[1].numpy(), g["labels"])
    assert [int(v) for v in mem2[2:]] == [int(v) for v in g["tail"]]


def test_invariants_memory_modes_and_render():
    """(1) norm_y == kv == raw, (2) forward_list([x]) == forward(x), (3) render leaves the
    memory tuple unchanged, (5) zero-initialised feedback is a no-op, (6) per-view independence of the encoder."""
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    imgs, ts = S.make_images(3, 48, 64, 0)
    with torch.no_grad():
        x, pos = R.encoder_forward(sde, cfg, imgs, ts)
        x1, _ = R.encoder_forward(sde, cfg, imgs[1:2], ts[1:2])
        assert rel_inf(x1, x[1:2]) < 1e-5
        outs = {}
        for mode in ("kv", "norm_y", "raw"):
            mem, _ = R.decoder_forward(sdd, cfg, x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None, False, mode)
            mem, _ = R.decoder_forward(sdd, cfg, x[2:].unsqueeze(0), pos[2:].unsqueeze(0), ts[2:].unsqueeze(0), mem, False, mode)
            mem_r, pm = R.decoder_forward(sdd, cfg, x.unsqueeze(0), pos.unsqueeze(0), ts.unsqueeze(0), mem, True, mode)
            assert mem_r[0] is not None and all(a is b or torch.equal(a, b) for a, b in zip(mem_r[0], mem[0]))
            assert mem_r[2:] == mem[2:]
            outs[mode] = pm
        assert rel_inf(outs["norm_y"], outs["kv"]) < 1e-5 and rel_inf(outs["raw"], outs["kv"]) < 1e-5
        mem_t, pm_t = R.decoder_forward(sdd, cfg, x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None)
        mem_l, pm_l = R.decoder_forward(sdd, cfg, [x[:2].unsqueeze(0)], [pos[:2].unsqueeze(0)], [ts[:2].unsqueeze(0)], None)
        assert torch.equal(pm_t, pm_l[0]) and all(torch.equal(a, b) for a, b in zip(mem_t[0], mem_l[0]))
        # zero feedback fc2 -> stored memory == prepare_y(layer inputs) == what the views attended
        sd0 = dict(sdd)
        sd0["feedback_layer.fc2.weight"] = torch.zeros_like(sdd["feedback_layer.fc2.weight"])
        sd0["feedback_layer.fc2.bias"] = torch.zeros_like(sdd["feedback_layer.fc2.bias"])
        mem_a, _, feats = R.decoder_forward(sd0, cfg, x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None,
                                            return_feats=True)
        y0 = R.prepare_y(sd0, "blocks_dec.1", feats[1].reshape(1, -1, cfg.dec_dim), "kv")
        assert rel_inf(mem_a[0][1], y0) < 1e-6


def test_postprocess_matches_formula():
    pm = torch.randn(2, 5, 6, 7)
    o = R.postprocess(pm)
    d = pm[..., :3].norm(dim=-1, keepdim=True)
    assert torch.allclose(o["pts3d"], pm[..., :3] / d * torch.expm1(d), atol=1e-6)
    assert torch.allclose(o["conf"], 1 + pm[..., 6].exp())


def test_cam_oracle_known_answers():
    """No golden vectors exist upstream for the two leaves; pin the restatement with analytic cases instead: an exact
    pinhole scene returns its focal, an exact rigid motion is recovered (proper rotation, det +1)."""
    from oracle import cam_ref
    torch.manual_seed(0)
    H, W, f = 24, 32, 37.5
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 1.0 + torch.rand(2, H, W)
    local = torch.stack(((xs - W / 2) / f * z, (ys - H / 2) / f * z, z), dim=-1)
    got = cam_ref.estimate_focal_knowing_depth(local, torch.tensor((W / 2, H / 2)))
    assert torch.allclose(got, torch.full((2,), f), rtol=1e-4)
    Q, _ = torch.linalg.qr(torch.randn(2, 3, 3))
    Q = Q * torch.sign(torch.det(Q)).view(2, 1, 1)
    t = torch.randn(2, 3)
    x = local.reshape(2, -1, 3)
    y = torch.einsum("nij,nkj->nki", Q, x) + t[:, None]
    w = torch.rand(2, x.shape[1]) + 0.1
    Rr, tr = cam_ref.rigid_points_registration(x, y, weights=w)
    assert torch.allclose(Rr, Q, atol=2e-5) and torch.allclose(tr, t, atol=2e-4)
    assert torch.allclose(torch.det(Rr), torch.ones(2), atol=1e-5)
    # reflection case: the sign fix must still return a proper rotation
    M = torch.diag(torch.tensor([1.0, 1.0, -1.0]))
    assert torch.det(cam_ref.special_procrustes(M)) > 0


def test_cam_oracle_matches_reference_fixture():
    """tests/golden/cam_40x56.npz = the reference's own postprocess(compute_cam=True) (oracle/make_golden.py cam)."""
    from oracle import cam_ref
    g = load_golden("cam_40x56")
    pm = torch.from_numpy(g["pm"])
    act = R.postprocess(pm)
    assert abs(act["conf"].double().sum().item() - float(g["conf_sum"])) < 1e-6 * float(g["conf_sum"])
    o = cam_ref.compute_cam(act["pts3d"], act["pts3d_local"], act["conf"])
    assert torch.allclose(o["focal"], torch.from_numpy(g["focal"]), rtol=1e-6)
    assert torch.allclose(o["c2w"], torch.from_numpy(g["c2w"]), rtol=1e-5, atol=1e-6)
    # the fp64 evaluation of the same formulas is the accuracy yardstick for the GPU path
    o64 = cam_ref.compute_cam(act["pts3d"], act["pts3d_local"], act["conf"], dtype=torch.float64)
    assert torch.allclose(o64["focal"].float(), o["focal"], rtol=1e-4)
    assert torch.allclose(o64["c2w"].float(), o["c2w"], atol=1e-4)


def test_nn_oracle_matches_reference_fixture():
    """tests/golden/nn_overlap.npz = the reference's searchers and get_overlap_score (oracle/make_golden.py nn)."""
    from oracle import nn_ref
    g = load_golden("nn_overlap")
    frames = S.make_overlap_frames(7, n_kf=4, H=48, W=64)
    for method in ("kdtree-scipy", "kdtree-scipy-quadrant_x2"):
        tree = nn_ref.get_searcher(method)
        for i, f in enumerate(frames):
            res = {k: f[k] for k in ("pts3d", "pts3d_local", "conf")}
            sc = [float(nn_ref.get_overlap_score(res, tree, f["cam"], mode=m, kf_x_subsamp=2, percentile=70)) for m in ("nn", "nn-norm")]
            assert sc == g[method + "/scores"][i].tolist(), (method, i)
            d = tree.query(f["pts3d"][0, 0, ::2, ::2].reshape(-1, 3), cam_center=f["cam"])
            assert np.array_equal(np.asarray(d, dtype=np.float64), g[method + "/dists"][i])
            tree.add_pts(f["pts3d"][0, 0][f["conf"][0, 0] > 1.5], cam_center=f["cam"])


def test_retrieval_oracle_matches_reference_fixture():
    """tests/golden/retrieval_small.npz = the reference's RetrievalModel (oracle/make_golden.py retrieval)."""
    from oracle import retrieval_ref as RR
    g = load_golden("retrieval_small")
    x = torch.randn((3, 48, 256), generator=torch.Generator().manual_seed(5))
    for tag, pre, resid in (("full", True, False), ("resid", False, True)):
        sd = S.make_retrieval_state_dict(256, seed=3, prewhiten=pre)
        f, a, i = RR.forward_local(sd, x, 20, resid)
        assert np.array_equal(i.numpy(), g[tag + "/idx"]) and np.array_equal(a.numpy(), g[tag + "/attn"])
        assert np.array_equal(f.numpy(), g[tag + "/feat"])
        assert np.array_equal(RR.forward_global(sd, x, resid).numpy(), g[tag + "/glob"])
    # multi-layer projector and Whitener(l2norm=dim)
    sd = S.make_retrieval_state_dict(256, seed=4, hdims=[320, 192])
    x = torch.randn((3, 48, 256), generator=torch.Generator().manual_seed(6))
    f, a, i = RR.forward_local(sd, x, 20)
    assert np.array_equal(i.numpy(), g["deep/idx"]) and np.array_equal(a.numpy(), g["deep/attn"]) and np.array_equal(f.numpy(), g["deep/feat"])
    assert np.array_equal(RR.forward_global(sd, x).numpy(), g["deep/glob"])
    for dim in (-1, 1):
        assert np.array_equal(RR.whiten(x, sd["prewhiten.m"], sd["prewhiten.p"], l2norm=dim).numpy(), g[f"l2norm{dim}/out"])


def test_gpu_baseline_harness_reproduces_the_port_on_cpu():
    """bench.py's ``torch_rocm_baseline`` leg runs the port with its leaves swapped for the torch ops the reference's modules call (oracle/gpu_baseline.py) so that
    autocast gives the reference's dtype flow.  Run on the CPU on the tiny network: with the all-fp32 policy the swapped leaves reproduce the port (1e-5), and under
    bf16 autocast the distance from the fp32 path is the reference's own bf16 envelope (~1e-2), not an arithmetic error of the harness."""
    import importlib.util
    import os
    from conftest import ROOT
    from oracle import must3r_ref as R0, gpu_baseline as G
    from must3r_amd.config import TINY
    from must3r_amd import synthetic as S
    spec = importlib.util.spec_from_file_location("must3r_ref_torch_leaves", os.path.join(ROOT, "oracle", "must3r_ref.py"))
    R1 = importlib.util.module_from_spec(spec)          # a private copy of the port: the swap must not leak into the other tests' oracle
    spec.loader.exec_module(R1)
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    imgs, ts = S.make_images(4, 48, 64, 0)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    with torch.no_grad():
        u0, r0, _ = R0.run_scene(sde, sdd, cfg, imgs, ts)
        G.install_torch_leaves(R1, "cpu")
        u1, r1, st = G.run_scene_gpu(R1, sde, sdd, cfg, imgs, ts, "cpu", torch.float32)
        u2, r2, _ = G.run_scene_gpu(R1, sde, sdd, cfg, imgs, ts, "cpu", torch.bfloat16)
    assert rel(u1, u0) < 1e-5 and rel(r1, r0) < 1e-5
    assert 1e-4 < rel(r2, r0) < 3e-2 and 1e-4 < rel(u2, u0) < 3e-2
    assert set(st) == {"encode", "update", "render"}

