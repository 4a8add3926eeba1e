"""CPU: the oracle restatement against the REAL reference (verbatim must3r/model on leaf shims).  The reference's side of
every test that takes a `ref` argument is stored in tests/golden/reference_values.pt (util.Reference: recorded with
M3R_RECORD_REFERENCE=1 where the reference tree exists, read back everywhere else); the tests without one run the reference
live and are skipped where its tree does not exist."""
import pytest
import torch

from conftest import HAS_REFERENCE
from must3r_amd.config import TINY
from must3r_amd import synthetic as S
from util import rel_inf, cam_scene, digest, Reference, RECORD_REFERENCE, save_reference_values

needs_reference = pytest.mark.skipif(not HAS_REFERENCE, reason="runs the reference's code live; its tree is not present")
if RECORD_REFERENCE and not HAS_REFERENCE:
    raise RuntimeError("M3R_RECORD_REFERENCE=1 needs the reference tree")


@pytest.fixture
def ref(request):
    return Reference(request.node.name)


@pytest.fixture(scope="module", autouse=True)
def _save_reference_values():
    yield
    save_reference_values()


def _reference_module(name):
    """one of the reference's own modules, imported on the leaf shims (record mode and the live tests only)"""
    import importlib
    from oracle import ref_shims
    ref_shims.install()
    return importlib.import_module(name)


def _build_reference(*a, **kw):
    from oracle import ref_shims
    return ref_shims.build_reference(*a, **kw)


def _build_reference_causal(*a, **kw):
    from oracle import ref_shims
    return ref_shims.build_reference_causal(*a, **kw)


@pytest.mark.parametrize("mode", ["kv", "norm_y", "raw"])
def test_restatement_equals_reference(mode, ref):
    from oracle import must3r_ref as R
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 3), S.make_decoder_state_dict(cfg, 3)
    imgs, ts = S.make_images(4, 64, 48, 3)  # portrait-shaped grid, 3 x 4 tokens
    enc, dec = ref.live(lambda: _build_reference(cfg, sde, sdd, mode)) or (None, None)  # strict load == state-dict key contract
    with torch.no_grad():
        xr, pr = ref(lambda: enc(imgs, ts))
        xo, po = R.encoder_forward(sde, cfg, imgs, ts)
        assert rel_inf(xo, xr) < 2e-5 and torch.equal(pr, po)
        memr = memo = None
        i = 0
        for nb in (2, 1, 1):
            sl = slice(i, i + nb)
            memr, pmr = ref(lambda: dec(xr[sl].unsqueeze(0), pr[sl].unsqueeze(0), ts[sl].unsqueeze(0), memr), sample=True)
            memo, pmo = R.decoder_forward(sdd, cfg, xr[sl].unsqueeze(0), pr[sl].unsqueeze(0), ts[sl].unsqueeze(0), memo, False, mode)
            assert rel_inf(ref.px(pmo), pmr) < 2e-5
            assert max(rel_inf(ref.px(a), b) for a, b in zip(memo[0], memr[0])) < 2e-5
            assert torch.equal(memo[1], memr[1]) and tuple(memo[2:]) == tuple(memr[2:])
            i += nb
        pmr = ref(lambda: dec(xr.unsqueeze(0), pr.unsqueeze(0), ts.unsqueeze(0), memr, render=True)[1], sample=True)
        _, pmo = R.decoder_forward(sdd, cfg, xr.unsqueeze(0), pr.unsqueeze(0), ts.unsqueeze(0), memo, True, mode)
        assert rel_inf(ref.px(pmo), pmr) < 2e-5


@pytest.mark.parametrize("mode,kw", [("kv", {}), ("norm_y", {"use_mem_mask": True}), ("kv", {"protected_imgs": 2})])
def test_causal_restatement_equals_reference(mode, kw, ref):
    """r06, SURVEY.md section 8f "later": CausalMUSt3R.forward (decoder.py:435-553), memory dropout off.  The reference's class itself on the leaf shims (both of its
    mask forms: the boolean attention mask and `use_mem_mask`'s physically removed rows) against the restatement's `causal=True`: calls of 3 (init: view 0 attends view 1,
    decoder.py:399-402), 2 and 1 views, render; pointmaps, memory, labels and the tuple's tail."""
    from oracle import must3r_ref as R
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 5), S.make_decoder_state_dict(cfg, 5)
    imgs, ts = S.make_images(6, 48, 64, 5)
    enc, plain = ref.live(lambda: _build_reference(cfg, sde, sdd, mode)) or (None, None)
    dec = ref.live(lambda: _build_reference_causal(cfg, sdd, mode, **kw))
    prot = kw.get("protected_imgs", 1)
    with torch.no_grad():
        x, pos = ref(lambda: enc(imgs, ts))
        memr = memo = None
        i = 0
        for nb in (3, 2, 1):
            sl = slice(i, i + nb)
            a = (x[sl].unsqueeze(0), pos[sl].unsqueeze(0), ts[sl].unsqueeze(0))
            memr, pmr = ref(lambda: dec(*a, memr), sample=True)
            memo, pmo = R.decoder_forward(sdd, cfg, *a, memo, False, mode, causal=True, protected_imgs=prot)
            assert rel_inf(ref.px(pmo), pmr) < 2e-5
            assert max(rel_inf(ref.px(u), v) for u, v in zip(memo[0], memr[0])) < 2e-5
            assert torch.equal(memo[1], memr[1]) and tuple(int(v) for v in memo[2:]) == tuple(int(v) for v in memr[2:])
            if i == 0:   # the causal mask is a different computation from MUSt3R's own-token mask as soon as a call holds more than one view
                pmp = ref(lambda: plain(*a, None)[1], sample=True)
                assert rel_inf(pmp, pmr) > 1e-2
            i += nb
        a = (x.unsqueeze(0), pos.unsqueeze(0), ts.unsqueeze(0))
        pmr = ref(lambda: dec(*a, memr, render=True)[1], sample=True)
        _, pmo = R.decoder_forward(sdd, cfg, *a, memo, True, mode, causal=True, protected_imgs=prot)
        assert rel_inf(ref.px(pmo), pmr) < 2e-5


def test_causal_fixture_is_what_the_restatement_computes():
    """tests/golden/small_224_causal.npz (oracle/make_golden.py main_causal: the REFERENCE's CausalMUSt3R, calls of [3, 2, 1] views + render) against the restatement."""
    import numpy as np
    import os
    from oracle import must3r_ref as R
    from must3r_amd.config import SMALL
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_224_causal.npz"))
    H, W, V, ps, tks = (int(v) for v in fx["meta"][:5])
    calls = [int(v) for v in fx["meta"][5:]]
    cfg = SMALL
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    imgs, ts = S.make_images(V, H, W, 0)
    with torch.no_grad():
        x, pos = R.encoder_forward(sde, cfg, imgs, ts)
        mem, upd, i = None, [], 0
        for k, nb in enumerate(calls):
            mem, pm = R.decoder_forward(sdd, cfg, x[i:i + nb].unsqueeze(0), pos[i:i + nb].unsqueeze(0), ts[i:i + nb].unsqueeze(0), mem, False, "kv", causal=True)
            upd.append(pm[0])
            assert [int(v) for v in mem[2:]] == [int(v) for v in fx["tails"][k]]
            i += nb
        _, ren = R.decoder_forward(sdd, cfg, x.unsqueeze(0), pos.unsqueeze(0), ts.unsqueeze(0), mem, True, "kv", causal=True)
    upd = torch.cat(upd, 0)
    assert rel_inf(upd[:, ::ps, ::ps], torch.from_numpy(fx["update"])) < 2e-5 and rel_inf(ren[0][:, ::ps, ::ps], torch.from_numpy(fx["render"])) < 2e-5
    assert rel_inf(mem[0][-1][0, ::tks, ::tks], torch.from_numpy(fx["mem_last"])) < 2e-5 and np.array_equal(mem[1].numpy(), fx["labels"])


def test_postprocess_equals_reference_geometry(ref):
    from oracle import must3r_ref as R
    G = ref.live(lambda: _reference_module("must3r.tools.geometry"))
    pm = ref(lambda: torch.randn(3, 8, 8, 7))   # (the recorded input: the global generator's state depends on the tests before)
    o = R.postprocess(pm)
    assert digest(o["pts3d"]) == ref(lambda: digest(G.apply_exp_to_norm(pm[..., :3])))
    assert digest(o["pts3d_local"]) == ref(lambda: digest(G.apply_exp_to_norm(pm[..., 3:6])))


def test_arg_rewriting_equals_reference(ref):
    RM = ref.live(lambda: _reference_module("must3r.model"))
    import must3r_amd.model as M
    train_str = ("CausalMUSt3R(img_size=(512, 512), feedback_type='single_mlp', memory_mode=\"kv\", mem_dropout=0.1, "
                 "dropout_mode='temporary', use_xformers_mask=True, use_mem_mask=True)")  # README.md:242
    assert M.convert_decoder_args(train_str) == ref(lambda: RM.convert_decoder_args(train_str))
    for s in ("Dust3rEncoder(img_size=(512,512),patch_embed='ManyAR_PatchEmbed')",
              "MUSt3R(img_size=(224, 224), pos_embed='RoPE100')",
              "MUSt3R(img_size=(224,224),pos_embed='RoPE100_224:512')"):
        for size in (224, 512, 768):
            assert M.set_image_size_in_args(s, size, verbose=False) == ref(lambda: RM.set_image_size_in_args(s, size, verbose=False))
    assert M.get_dtype("bf16") == torch.bfloat16 and M.get_dtype(False) == torch.float32


def test_streaming_schedule_equals_reference_driver(ref):
    """must3r_amd.engine.run_video restates inference_video_multi_ar (engine/inference.py:232-366).  Run the REAL reference
    driver with the REAL reference modules and compare the surviving memory / labels / first-pass pointmaps with run_video
    driven by the oracle forwards."""
    from oracle import must3r_ref as R
    from must3r_amd.engine import run_video
    RI = ref.live(lambda: _reference_module("must3r.engine.inference"))
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    enc, dec = ref.live(lambda: _build_reference(cfg, sde, sdd, "kv")) or (None, None)
    V = 11
    imgs, ts = S.make_images(V, 48, 64, 4)
    with torch.no_grad():
        def reference():
            mem, pm = RI.inference_video_multi_ar(enc, dec, [im for im in imgs], [t for t in ts], [2] + [1] * (V - 2),
                                                  return_mem=True, local_context_size=3, device=torch.device("cpu"))
            return mem, torch.stack([p["pts3d"] for p in pm], dim=0)
        mem_r, want = ref(reference, sample=True)
        enc_o = lambda im, t: R.encoder_forward(sde, cfg, im, t)  # noqa: E731
        dec_o = lambda x, p, t, m=None, render=False: R.decoder_forward(sdd, cfg, x, p, t, m, render, "kv")  # noqa: E731
        mem_o, pm_o, kf = run_video(enc_o, dec_o, imgs, ts, local_context_size=3)
    assert kf == [0, 1, 3, 6, 9]
    assert torch.equal(mem_r[1], mem_o[1]) and int(mem_r[2]) == int(mem_o[2])
    assert max(rel_inf(ref.px(a), b) for a, b in zip(mem_o[0], mem_r[0])) < 2e-5
    assert ref.px(pm_o).shape == want.shape and rel_inf(ref.px(pm_o), want) < 2e-5


def test_compute_cam_glue_equals_reference_postprocess(ref):
    """engine/inference.py:29-47 (pp, which maps feed the focal / the registration, conf-1 weights, c2w assembly) run
    VERBATIM from the reference with the restated third-party leaves plugged in, against oracle/cam_ref.compute_cam."""
    from oracle import cam_ref, must3r_ref as R
    E = ref.live(lambda: _reference_module("must3r.engine.inference"))
    torch.manual_seed(3)
    pm = cam_scene(2, 3, 24, 32)
    want = ref(lambda: {k: v for k, v in E.postprocess(pm, compute_cam=True).items() if k in ("focal", "c2w")})
    act = R.postprocess(pm)
    ours = cam_ref.compute_cam(act["pts3d"], act["pts3d_local"], act["conf"])
    assert want["focal"].shape == (2, 3) and want["c2w"].shape == (2, 3, 4, 4)
    assert torch.allclose(ours["focal"], want["focal"], rtol=1e-6, atol=0)
    assert torch.allclose(ours["c2w"], want["c2w"], rtol=1e-5, atol=1e-6)


def test_return_feats_equals_reference(ref):
    """decoder.py:344-347 (tensor) and :258-262 (forward_list): list of [encoder tokens, block outputs, norm_dec(last)]."""
    from oracle import must3r_ref as R
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    enc, dec = ref.live(lambda: _build_reference(cfg, sde, sdd, "kv")) or (None, None)
    imgs, ts = S.make_images(3, 48, 64, 2)
    with torch.no_grad():
        x, pos = ref(lambda: enc(imgs, ts))
        mem, _, feats = ref.live(lambda: dec(x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None,
                                             return_feats=True)) or (None,) * 3
        feats = ref(lambda: feats, sample=True)   # (mem only feeds the reference's own forward_list call below)
        memo, pmo, fo = R.decoder_forward(sdd, cfg, x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None, False, "kv",
                                          return_feats=True)
        assert len(feats) == len(fo) == cfg.dec_depth + 1
        for a, b in zip(feats, fo):
            b = ref.px(b)
            assert a.shape == b.shape and rel_inf(b, a) < 2e-5
        fl = ref(lambda: dec.forward_list([x[2:].unsqueeze(0)], [pos[2:].unsqueeze(0)], [ts[2:].unsqueeze(0)], mem, render=True,
                                          return_feats=True)[2], sample=True)
        _, pmlo, flo = R.decoder_forward(sdd, cfg, [x[2:].unsqueeze(0)], [pos[2:].unsqueeze(0)], [ts[2:].unsqueeze(0)], memo, True, "kv",
                                         return_feats=True)
        assert len(fl) == len(flo) == 1 and len(fl[0]) == len(flo[0])
        for a, b in zip(fl[0], flo[0]):
            b = ref.px(b)
            assert a.shape == b.shape and rel_inf(b, a) < 2e-5


def test_overlap_score_equals_reference(ref):
    """slam/nns.py + slam/model.py:62-91 run VERBATIM from the reference (numpy + scipy only) against oracle/nn_ref.py."""
    import numpy as np
    from oracle import nn_ref
    ref_nns = ref.live(lambda: _reference_module("must3r.slam.nns"))
    ref_tools = ref.live(lambda: _reference_module("must3r.slam.tools"))
    frames = S.make_overlap_frames(0)
    rays = frames[1]["pts3d"].reshape(-1, 3) - frames[0]["cam"][None]
    assert np.array_equal(ref(lambda: ref_tools.get_quadrant_id(rays.copy(), quadrant_divider=2)), nn_ref.get_quadrant_id(rays.copy(), 2))
    for method in ("kdtree-scipy", "kdtree-scipy-quadrant_x2"):
        tr, to = ref.live(lambda: ref_nns.get_searcher(method)), nn_ref.get_searcher(method)
        q = torch.from_numpy(frames[0]["pts3d"].reshape(-1, 3))
        assert np.array_equal(ref(lambda: tr.query(q, cam_center=torch.from_numpy(frames[0]["cam"]))), to.query(q.numpy(), cam_center=frames[0]["cam"]))
        for f in frames[:-1]:
            sel = f["pts3d"][0, 0][f["conf"][0, 0] > 1.5]
            ref.live(lambda: tr.add_pts(torch.from_numpy(sel), cam_center=torch.from_numpy(f["cam"])))
            to.add_pts(sel, cam_center=f["cam"])
            g = frames[-1]
            qq = torch.from_numpy(g["pts3d"][0, 0, ::2, ::2].reshape(-1, 3))
            dr = ref(lambda: tr.query(qq, cam_center=torch.from_numpy(g["cam"])))
            do = to.query(qq.numpy(), cam_center=g["cam"])
            assert np.array_equal(dr, do)


def _reference_function(path, name, namespace):
    """Compile ONE function of a reference file (``path`` relative to the reference tree) whose module cannot be imported here
    (un-vendored imports at the top): the function's own source is executed verbatim from the reference tree, nothing is copied
    into the repo."""
    import ast
    import os
    from oracle import ref_shims
    path = os.path.join(ref_shims.REFERENCE_ROOT, path)
    src = open(path).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name)
    code = compile(ast.Module(body=[node], type_ignores=[]), path, "exec")
    exec(code, namespace)
    return namespace[name]


@pytest.mark.parametrize("mode", ["nn", "nn-norm"])
@pytest.mark.parametrize("subsamp", [None, 2])
def test_get_overlap_score_equals_reference_source(mode, subsamp, ref):
    """slam/model.py:62-91 (its module needs dust3r.datasets; the function itself only numpy) vs oracle/nn_ref.py."""
    import numpy as np
    from oracle import nn_ref
    ref_nns = ref.live(lambda: _reference_module("must3r.slam.nns"))
    ref_score = ref.live(lambda: _reference_function("must3r/slam/model.py", "get_overlap_score", {"np": np}))
    frames = S.make_overlap_frames(1)
    tr, to = ref.live(lambda: ref_nns.get_searcher("kdtree-scipy-quadrant_x2")), nn_ref.get_searcher("kdtree-scipy-quadrant_x2")
    for i, f in enumerate(frames):
        res_t = {k: torch.from_numpy(f[k]) for k in ("pts3d", "pts3d_local", "conf")}
        res_n = {k: f[k] for k in ("pts3d", "pts3d_local", "conf")}
        if mode == "nn-norm" and subsamp is None and i > 0:
            # reference quirk: without subsampling `depths[msk]` indexes [H,W] depths with a [1,1,H,W] mask -> IndexError;
            # the restatement must fail the same way
            with pytest.raises(IndexError):
                ref(lambda: ref_score(res_t, tr, torch.from_numpy(f["cam"]), mode=mode, kf_x_subsamp=subsamp))
            with pytest.raises(IndexError):
                nn_ref.get_overlap_score(res_n, to, f["cam"], mode=mode, kf_x_subsamp=subsamp)
            mode_eff = "nn"
        else:
            mode_eff = mode
        if mode == "nn-norm" and subsamp is None and i == 0:
            mode_eff = "nn"
        s_ref = ref(lambda: ref_score(res_t, tr, torch.from_numpy(f["cam"]), mode=mode_eff, kf_x_subsamp=subsamp))
        s_ora = nn_ref.get_overlap_score(res_n, to, f["cam"], mode=mode_eff, kf_x_subsamp=subsamp)
        assert float(s_ref) == float(s_ora), (i, s_ref, s_ora)
        sel = f["pts3d"][0, 0][f["conf"][0, 0] > 1.5]
        ref.live(lambda: tr.add_pts(torch.from_numpy(sel), cam_center=torch.from_numpy(f["cam"])))
        to.add_pts(sel, cam_center=f["cam"])


@pytest.mark.parametrize("cfg", [dict(prewhiten=-1, postwhiten=-1), dict(prewhiten=None, postwhiten=-1, residual=True),
                                 dict(prewhiten=None, postwhiten=None), dict(prewhiten=-1, postwhiten=-1, hdims=[96, 160, 64])])
def test_retrieval_equals_reference(cfg, ref):
    """must3r/retrieval/model.py RetrievalModel (verbatim import) vs oracle/retrieval_ref.py: local and global paths."""
    from oracle import retrieval_ref as RR
    RM = ref.live(lambda: _reference_module("must3r.retrieval.model"))

    class _Backbone(torch.nn.Module):
        embed_dim = 128
    hdims = cfg.get("hdims", [128])
    model = ref.live(lambda: RM.RetrievalModel(_Backbone(), prewhiten=cfg.get("prewhiten"), postwhiten=cfg.get("postwhiten"), hdims=hdims,
                                               residual=cfg.get("residual", False), nfeat=17).eval())
    sd = S.make_retrieval_state_dict(128, seed=1, prewhiten=cfg.get("prewhiten") is not None, postwhiten=cfg.get("postwhiten") is not None,
                                     hdims=hdims)
    missing, unexpected = ref(lambda: tuple(list(v) for v in model.load_state_dict(sd, strict=False)))   # (missing_keys, unexpected_keys)
    assert not unexpected and not [k for k in missing if not k.startswith("backbone")]
    x = torch.randn((2, 40, 128), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want_local = ref(lambda: digest(tuple(model.forward_local(x))))
        want_global = ref(lambda: digest(model.forward_global(x)))
    fo, ao, io = RR.forward_local(sd, x, 17, cfg.get("residual", False))
    go = RR.forward_global(sd, x, cfg.get("residual", False))
    assert digest((fo, ao, io)) == want_local and digest(go) == want_global   # bit-equal, as torch.equal
    if cfg.get("prewhiten") is not None:      # Whitener(l2norm=dim) (:77-78), any dimension
        for dim in (-1, 1, 0):
            wh = ref.live(lambda: RM.Whitener(128, l2norm=dim))
            ref.live(lambda: wh.load_state_dict({"m": sd["prewhiten.m"], "p": sd["prewhiten.p"]}))
            with torch.no_grad():
                assert ref(lambda: digest(wh(x))) == digest(RR.whiten(x, sd["prewhiten.m"], sd["prewhiten.p"], l2norm=dim))


@pytest.mark.parametrize("fb", ["single_linear", None])
def test_feedback_types_equal_reference(fb, ref):
    """feedback_mechanism.py:11-22,39-53: 'single_linear' and no feedback layer (the released checkpoints use 'single_mlp')."""
    from oracle import must3r_ref as R
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0, feedback_type=fb)
    enc, dec = ref.live(lambda: _build_reference(cfg, sde, sdd, "kv", feedback_type=fb)) or (None, None)
    imgs, ts = S.make_images(3, 48, 64, 1)
    with torch.no_grad():
        x, pos = ref(lambda: enc(imgs, ts))
        mem, pm = ref(lambda: dec(x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None), sample=True)
        mem, pm2 = ref(lambda: dec(x[2:].unsqueeze(0), pos[2:].unsqueeze(0), ts[2:].unsqueeze(0), mem), sample=True)
        memo, pmo = R.decoder_forward(sdd, cfg, x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None, False, "kv")
        memo, pmo2 = R.decoder_forward(sdd, cfg, x[2:].unsqueeze(0), pos[2:].unsqueeze(0), ts[2:].unsqueeze(0), memo, False, "kv")
    assert rel_inf(ref.px(pmo), pm) < 2e-5 and rel_inf(ref.px(pmo2), pm2) < 2e-5
    for a, b in zip(memo[0], mem[0]):
        assert rel_inf(ref.px(a), b) < 2e-5


@pytest.mark.parametrize("mode", ["kv", "norm_y"])
def test_batch_elements_are_independent_in_reference(mode, ref):
    """Pins the fact the B > 1 route of must3r_amd.model.decoder rests on: the reference's B = 2 forward equals its two
    B = 1 forwards stacked (memory, labels and attention are per batch element, decoder.py:158-350)."""
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 5), S.make_decoder_state_dict(cfg, 5)
    imgs, ts = S.make_images(6, 48, 64, 5)

    def compare():
        """every quantity the test asserts on, per batch element: a statement about the reference alone, so what is recorded is
        the comparison itself (computed at full resolution), not the pointmaps"""
        enc, dec = _build_reference(cfg, sde, sdd, mode)
        with torch.no_grad():
            x, pos = enc(imgs, ts)
            x, pos, t = x.view(2, 3, *x.shape[1:]), pos.view(2, 3, *pos.shape[1:]), ts.view(2, 3, 2)
            c = lambda *a: [v.contiguous() for v in a]   # the reference .view()s its inputs (decoder.py:274)  # noqa: E731
            mem2, pm2 = dec(*c(x[:, :2], pos[:, :2], t[:, :2]), None)
            mem2, pm2b = dec(*c(x[:, 2:], pos[:, 2:], t[:, 2:]), mem2)
            _, pm2r = dec(x, pos, t, mem2, render=True)
            out = []
            for b in range(2):
                s = slice(b, b + 1)
                mem1, pm1 = dec(*c(x[s, :2], pos[s, :2], t[s, :2]), None)
                mem1, pm1b = dec(*c(x[s, 2:], pos[s, 2:], t[s, 2:]), mem1)
                _, pm1r = dec(x[s], pos[s], t[s], mem1, render=True)
                out.append({"pointmaps": [rel_inf(pm2[s], pm1), rel_inf(pm2b[s], pm1b), rel_inf(pm2r[s], pm1r)],
                            "memory": max(rel_inf(a[s], c) for a, c in zip(mem2[0], mem1[0])),
                            "labels_equal": torch.equal(mem2[1][s], mem1[1]), "tails": (tuple(mem2[2:]), tuple(mem1[2:]))})
            return out
    for r in ref(compare):
        assert max(r["pointmaps"]) < 1e-5 and r["memory"] < 1e-5
        assert r["labels_equal"] and r["tails"][0] == r["tails"][1]


# ----------------------------------------------------------------------------------------------------------------------
# L3 drivers: must3r_amd.inference against must3r/engine/inference.py, both driving the SAME
# (reference, CPU) modules -> every tensor must be bit-equal, every label / index / count identical.
# ----------------------------------------------------------------------------------------------------------------------
def _mixed_views(n, seed):
    """n views over three aspect ratios (16-px patches: 3x4, 4x3 and 2x4 tokens), deliberately interleaved."""
    g = torch.Generator().manual_seed(seed)
    sizes = [(48, 64), (64, 48), (32, 64)]
    imgs, ts = [], []
    for i in range(n):
        H, W = sizes[(i * 2 + i // 3) % 3]
        imgs.append(torch.rand((3, H, W), generator=g) * 2 - 1)
        ts.append(torch.tensor([H, W]))
    return imgs, ts


def _same(a, b):
    if a is None or b is None:
        assert a is None and b is None
    elif isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            _same(u, v)
    elif torch.is_tensor(a):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    else:
        assert a == b, (a, b)


def _drivers(mode="kv"):
    from oracle import ref_shims
    ref_shims.install()
    import must3r.engine.inference as RI
    import must3r_amd.inference as MI
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 2), S.make_decoder_state_dict(cfg, 2)
    enc, dec = ref_shims.build_reference(cfg, sde, sdd, mode)
    pp = lambda pm: RI.postprocess(pm, compute_cam=False)  # noqa: E731
    return RI, MI, enc, dec, pp


def test_stack_views_equals_reference(ref):
    import must3r_amd.inference as MI
    RI = ref.live(lambda: _reference_module("must3r.engine.inference"))
    imgs, ts = _mixed_views(9, 0)
    tst = torch.stack(ts)
    x = [torch.full((2,), float(i)) for i in range(9)]
    ids = [torch.tensor(i) for i in range(9)]
    for max_bs in (None, 1, 2, 5):
        _same(digest(MI.stack_views(tst, [x, ids], max_bs=max_bs)), ref(lambda: digest(RI.stack_views(tst, [x, ids], max_bs=max_bs))))
        # partially missing encoder tokens: those views are regrouped behind the complete ones
        for holes in ([1, 4], [0, 3, 6], list(range(9)), [8]):
            # (tokens and positions are missing together, like everywhere in the reference: a value that is only missing
            # for part of a regrouped chunk comes back as an unstacked list there, :112/:129-134, and crashes its caller)
            xh = [None if i in holes else v for i, v in enumerate(x)]
            ph = [None if i in holes else v + 1 for i, v in enumerate(x)]
            _same(digest(MI.stack_views(tst, [xh, ph, imgs], max_bs=max_bs)),
                  ref(lambda: digest(RI.stack_views(tst, [xh, ph, imgs], max_bs=max_bs))))
    got = MI.unstack_pointmaps([[2, 0], [1]], [{"a": torch.arange(4).view(2, 2)}, {"a": torch.arange(2).view(1, 2)}])
    _same(digest(got), ref(lambda: digest(RI.unstack_pointmaps([[2, 0], [1]], [{"a": torch.arange(4).view(2, 2)}, {"a": torch.arange(2).view(1, 2)}]))))


@needs_reference
@pytest.mark.parametrize("case", [dict(), dict(max_bs=2), dict(num_refinements_iterations=1), dict(to_render=[7, 2, 3], max_bs=2),
                                  dict(precompute="some"), dict(precompute="all", num_refinements_iterations=2, max_bs=1),
                                  dict(mode="norm_y", num_refinements_iterations=1)])
def test_inference_multi_ar_equals_reference(case):
    case = dict(case)
    RI, MI, enc, dec, pp = _drivers(case.pop("mode", "kv"))
    n = 8
    imgs, ts = _mixed_views(n, 1)
    ids = [torch.tensor(v) for v in (5, 0, 7, 2, 9, 4, 1, 3)]      # ids are arbitrary (keyframes first in the demo)
    mem_batches = [2, 1, 2]
    pre = case.pop("precompute", None)

    def feats(module):
        if pre is None:
            return None
        x, pos = module.encoder_multi_ar(enc, imgs, torch.stack(ts), max_bs=case.get("max_bs"), device=torch.device("cpu"))
        if pre == "some":
            for i in (1, 6):
                x[i] = pos[i] = None
        return x, pos
    with torch.no_grad():
        want = RI.inference_multi_ar(enc, dec, list(imgs), ids, list(ts), mem_batches, post_process_function=pp,
                                     encoder_precomputed_features=feats(RI), return_mem=True, device=torch.device("cpu"), **case)
        got = MI.inference_multi_ar(enc, dec, list(imgs), ids, list(ts), mem_batches, post_process_function=pp,
                                    encoder_precomputed_features=feats(MI), return_mem=True, device=torch.device("cpu"), **case)
    _same(list(got), list(want))
    assert all(p is not None for p in got[1]) and len(got[2]) == (3 if "to_render" in case else n)
    # render-only entry: a precomputed memory, nothing to update (engine/inference.py:461-463)
    with torch.no_grad():
        want2 = RI.inference_multi_ar(enc, dec, list(imgs), ids, list(ts), mem_batches, post_process_function=pp,
                                      precomputed_mem=want[0], to_render=[4, 5], device=torch.device("cpu"))
        got2 = MI.inference_multi_ar(enc, dec, list(imgs), ids, list(ts), mem_batches, post_process_function=pp,
                                     precomputed_mem=got[0], to_render=[4, 5], device=torch.device("cpu"))
        _same(list(got2), list(want2))
        _same(list(MI.inference_multi_ar(enc, dec, list(imgs), ids, list(ts), mem_batches, precomputed_mem=got[0], to_render=[],
                                         device=torch.device("cpu"))), [None, []])


@needs_reference
@pytest.mark.parametrize("case", [dict(), dict(local_context_size=2, max_bs=1), dict(num_refinements_iterations=1, local_context_size=3),
                                  dict(num_refinements_iterations=2, local_context_size=100), dict(batches=[3, 2, 2, 2, 2]),
                                  dict(stateful=True, local_context_size=4, num_refinements_iterations=1)])
def test_inference_video_multi_ar_equals_reference(case):
    case = dict(case)
    RI, MI, enc, dec, pp = _drivers()
    n = 11
    imgs, ts = _mixed_views(n, 3)
    mem_batches = case.pop("batches", [2] + [1] * (n - 2))
    kw = {}
    if case.pop("stateful", False):
        # a keyframe test that looks at the result and at a running scene state, like slam's (demo/inference.py:63-106)
        kw = dict(is_keyframe_function=lambda i, res, st: float(res["conf"].mean()) > st["thr"] or i % 4 == 0,
                  scene_state_update_function=lambda res, st: {"thr": 0.5 * st["thr"] + 0.5 * float(res["conf"].mean()),
                                                                "n": st["n"] + 1})
    with torch.no_grad():
        if kw:
            kw_r, kw_m = dict(kw, scene_state={"thr": 0.0, "n": 0}), dict(kw, scene_state={"thr": 0.0, "n": 0})
        else:
            kw_r = kw_m = {}
        want = RI.inference_video_multi_ar(enc, dec, list(imgs), list(ts), mem_batches, post_process_function=pp, return_mem=True,
                                           device=torch.device("cpu"), **case, **kw_r)
        got = MI.inference_video_multi_ar(enc, dec, list(imgs), list(ts), mem_batches, post_process_function=pp, return_mem=True,
                                          device=torch.device("cpu"), **case, **kw_m)
    _same(list(got), list(want))
    assert MI.get_Nmem(got[0]) == RI.get_Nmem(want[0]) > 0


@needs_reference
def test_tensor_inference_driver_equals_reference():
    """engine/inference.py:570-688 (`inference`, `inference_encoder`): B = 2 scenes of one aspect ratio, with and without
    max_bs slicing, to_render, train_decoder_skip."""
    RI, MI, enc, dec, _ = _drivers()
    imgs, ts = S.make_images(10, 48, 64, 6)
    imgs, ts = imgs.view(2, 5, 3, 48, 64), ts.view(2, 5, 2)
    for kw in (dict(), dict(max_bs=3), dict(to_render=[4, 0, 2], max_bs=4), dict(train_decoder_skip=1), dict(to_render=[])):
        with torch.no_grad():
            want = RI.inference(enc, dec, imgs, ts, [2, 1, 1], **kw)
            got = MI.inference(enc, dec, imgs, ts, [2, 1, 1], **kw)
        _same(list(got), list(want))


class _InPlaceMemoryDecoder:
    """The reference decoder's arithmetic behind the NATIVE module's memory management: the memory tuple it returns is made
    of prefix views of ``MUSt3R._writable_memory``'s over-allocated buffers and an update appends in place -- the aliasing
    the L3 drivers have to live with on the GPU (refinement scratch rows, in-place compaction, rewind), on CPU."""

    def __init__(self, ref_dec, cfg, host_labels=False):
        import must3r_amd.model as M
        self.host_labels = host_labels   # attach the host mirror of the label layout like MUSt3R._forward_scene does
        self.ref = ref_dec
        self.native = M.MUSt3R(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth,
                               num_heads=cfg.dec_heads, feedback_type="single_mlp", memory_mode="kv")
        self.copies = 0            # how often the memory had to be copied out into fresh buffers
        self.appends = 0

    @property
    def reserve_memory_tokens(self):
        return self.native.reserve_memory_tokens

    @reserve_memory_tokens.setter
    def reserve_memory_tokens(self, v):
        self.native.reserve_memory_tokens = v

    def __call__(self, x, pos, true_shape, current_mem=None, render=False):
        plain = None
        if current_mem is not None:
            plain = ([v.clone() for v in current_mem[0]], current_mem[1].clone(), *current_mem[2:])
        new_mem, pm = self.ref(x, pos, true_shape, plain, render=render)
        if render:
            return current_mem, pm
        Nm = 0 if current_mem is None else int(current_mem[0][0].shape[1])
        R = int(new_mem[0][0].shape[1]) - Nm
        before = None if current_mem is None else getattr(current_mem[0][0], "_m3r_owner", None)
        owner = self.native._writable_memory(None if current_mem is None else list(current_mem[0]), Nm, R, torch.float32,
                                             torch.device("cpu"))
        self.copies += int(current_mem is not None and owner is not before)
        self.appends += int(current_mem is not None and owner is before)
        for b, v in zip(owner.bufs, new_mem[0]):
            b[:, Nm:Nm + R] = v[:, Nm:]
        owner.valid = Nm + R
        labels = new_mem[1]
        if self.host_labels:
            from must3r_amd.engine import _label_runs, attach_label_runs
            runs = [] if current_mem is None else _label_runs(current_mem[1])
            if runs is not None and sum(c for _, c in runs) == Nm:
                runs = list(runs)
                first = 0 if current_mem is None else int(current_mem[2])
                for xg in (x if isinstance(x, (list, tuple)) else [x]):
                    runs += [(first + j, int(xg.shape[2])) for j in range(int(xg.shape[1]))]
                    first += int(xg.shape[1])
                assert sum(c for _, c in runs) == Nm + R
                attach_label_runs(labels, runs)
                self.mirrored = getattr(self, "mirrored", 0) + 1
        return (owner.views(Nm + R), labels, *new_mem[2:]), pm


@needs_reference
@pytest.mark.parametrize("host_labels", [False, True])
@pytest.mark.parametrize("video", [False, True])
def test_drivers_on_in_place_memory_equal_reference(video, host_labels):
    """``host_labels``: the label tensors carry the host mirror of their layout (``_m3r_runs``), so eviction / refresh /
    restore build their indices on the host (no nonzero read-back); without it the helpers use the reference's boolean masks."""
    RI, MI, enc, dec, pp = _drivers()
    n = 10
    imgs, ts = _mixed_views(n, 5)
    ids = [torch.tensor(v) for v in range(n)]
    native_like = _InPlaceMemoryDecoder(dec, TINY, host_labels)
    with torch.no_grad():
        if video:
            args = ([2] + [1] * (n - 2),)
            kw = dict(post_process_function=pp, return_mem=True, device=torch.device("cpu"), num_refinements_iterations=2,
                      local_context_size=3)
            want = RI.inference_video_multi_ar(enc, dec, list(imgs), list(ts), *args, **kw)
            got = MI.inference_video_multi_ar(enc, native_like, list(imgs), list(ts), *args, **kw)
        else:
            args = (ids, list(ts), [2, 1, 2, 1])
            kw = dict(post_process_function=pp, return_mem=True, device=torch.device("cpu"), num_refinements_iterations=2)
            want = RI.inference_multi_ar(enc, dec, list(imgs), *args, **kw)
            got = MI.inference_multi_ar(enc, native_like, list(imgs), *args, **kw)
    _same(list(got), list(want))
    # the memory stayed in the decoder's buffers the whole way: no update had to copy it out
    assert native_like.appends > 0 and native_like.copies == 0, (native_like.appends, native_like.copies)
    assert getattr(got[0][0][0], "_m3r_owner", None) is not None
    if host_labels:   # the mirror survived every surgery step and still describes the final labels
        from must3r_amd.engine import _label_runs
        runs = _label_runs(got[0][1])
        assert runs is not None and native_like.mirrored == native_like.appends + 1
        assert torch.equal(torch.cat([torch.full((c,), l) for l, c in runs]).view(1, -1), got[0][1])
    if not video:
        # rewind_mem is an optimisation, never a correctness requirement: without it the refinement passes copy the memory
        # out (the buffers still count the scratch rows) and the results are the same
        slow = _InPlaceMemoryDecoder(dec, TINY)
        keep, MI.rewind_mem = MI.rewind_mem, (lambda vals: vals)
        try:
            with torch.no_grad():
                again = MI.inference_multi_ar(enc, slow, list(imgs), *args, **kw)
        finally:
            MI.rewind_mem = keep
        _same(list(again), list(want))
        assert slow.copies > 0


@needs_reference
def test_forward_must3r_equals_reference_source():
    """slam/model.py:22-59 (the SLAM agent's forward wrapper; its module needs dust3r.datasets, the function does not)
    against must3r_amd.slam_nn.forward_must3r, both on the reference modules (CPU): update and render calls, views of
    different aspect ratios in one call."""
    from oracle import ref_shims
    ref_shims.install()
    import must3r.engine.inference as RI
    import must3r.model as RM
    from must3r_amd.slam_nn import forward_must3r
    ns = {"torch": torch, "postprocess": RI.postprocess, "get_pointmaps_activation": RM.get_pointmaps_activation}
    ref_forward = _reference_function("must3r/slam/model.py", "forward_must3r", ns)
    cfg = TINY
    sde, sdd = S.make_encoder_state_dict(cfg, 4), S.make_decoder_state_dict(cfg, 4)
    enc, dec = ref_shims.build_reference(cfg, sde, sdd, "kv")
    imgs, ts = _mixed_views(4, 11)
    views = [{"img": im[None], "true_shape": t.numpy()[None]} for im, t in zip(imgs, ts)]   # [1,2] like dust3r load_images
    import unittest.mock as mock
    with torch.no_grad(), mock.patch("torch.cuda.empty_cache", lambda: None):
        mem_r = mem_m = None
        for batch, render in ((views[:2], False), (views[2:3], False), (views, True), (views[3:], False)):
            out_r, mem_r = ref_forward((enc, dec), batch, mem_r, render=render, device="cpu")
            out_m, mem_m = forward_must3r((enc, dec), batch, mem_m, render=render, device="cpu", postprocess=RI.postprocess)
            _same(out_m, out_r)
            _same(list(mem_m), list(mem_r))


@needs_reference
def test_backend_switch_inside_the_reference(tmp_path, monkeypatch):
    """must3r_amd.backend.install(): the reference's own `must3r.model.load_model` (model/__init__.py:30-50) dispatches to the HIP-backed
    loader when the module-global switch is on (the attention.py:18-27 pattern), also for modules that imported the name earlier
    (slam/model.py:10 style), and is the untouched reference function when it is off / after uninstall()."""
    import types
    from oracle import ref_shims
    ref_shims.install()
    import must3r.model as RM
    import must3r_amd.backend as hb
    import must3r_amd.model as HM
    from must3r_amd.config import TINY
    orig = RM.load_model
    early = types.ModuleType("must3r._early_importer")       # a module that did `from must3r.model import load_model` before install()
    early.load_model = orig
    monkeypatch.setitem(__import__("sys").modules, "must3r._early_importer", early)
    # a checkpoint in the reference's format (constructor strings + state dicts)
    cfg = TINY
    enc_s = (f"Dust3rEncoder(img_size=({cfg.img_size},{cfg.img_size}), patch_size=16, embed_dim={cfg.enc_dim}, depth={cfg.enc_depth}, "
             f"num_heads={cfg.enc_heads})")
    dec_s = (f"MUSt3R(img_size=({cfg.img_size},{cfg.img_size}), patch_size=16, enc_embed_dim={cfg.enc_dim}, embed_dim={cfg.dec_dim}, "
             f"depth={cfg.dec_depth}, num_heads={cfg.dec_heads}, feedback_type='single_mlp', memory_mode='kv')")
    ck = tmp_path / "tiny.pth"
    torch.save({"args": types.SimpleNamespace(encoder=enc_s, decoder=dec_s), "encoder": S.make_encoder_state_dict(cfg, 0),
                "decoder": S.make_decoder_state_dict(cfg, 0)}, ck)
    try:
        hb.install()
        assert RM.load_model is not orig and early.load_model is RM.load_model and RM.load_model.__wrapped__ is orig
        assert RM.is_hip_backend_enabled() is False
        e0, d0 = RM.load_model(str(ck), device="cpu", verbose=False)                 # switch off: the reference's modules
        assert type(e0).__module__.startswith("must3r.model") and type(d0).__module__.startswith("must3r.model")
        RM.toggle_hip_backend(True)
        e1, d1 = early.load_model(str(ck), device="cpu", verbose=False)              # switch on: the HIP-backed mirrors, same state dict
        assert isinstance(e1, HM.Dust3rEncoder) and isinstance(d1, HM.MUSt3R)
        assert set(e1.state_dict()) == set(e0.state_dict()) and set(d1.state_dict()) == set(d0.state_dict())
        for k, v in d0.state_dict().items():
            assert torch.equal(v, d1.state_dict()[k]), k
        with pytest.raises(RuntimeError, match="no CPU"):                           # and they have no CPU route: the native path or nothing
            e1(torch.zeros((1, 3, cfg.img_size, cfg.img_size)), torch.tensor([[cfg.img_size, cfg.img_size]]))
        RM.toggle_hip_backend(False)
        assert type(RM.load_model(str(ck), device="cpu", verbose=False)[0]).__module__.startswith("must3r.model")
    finally:
        hb.uninstall()
    assert RM.load_model is orig and early.load_model is orig and not hasattr(RM, "toggle_hip_backend")
