"""GPU (-m gpu): the ASMK back-end of the retrieval mode (csrc/asmk.hip, include/must3r_hip.h ABI 11; must3r_amd.asmk, retrieval,
demo) against the restatement in tests/asmk_ref.py.

1. quantize: ids identical to the fp64 top-k wherever the fp64 gaps around the k-th neighbour exceed the fp32 bound, distances within
   the bound elsewhere; duplicated centroids give the lower id first; repeated calls give the same ids; split-and-merge at K = 65 536;
2. aggregate: words, counts and bits exactly equal to the sequential fp32 restatement, ragged images, all rows on one word;
3. scores on the kernel's own bits within 2e-7 of the row maximum, zero without a shared word, asymmetric, alpha / tau / normalize;
4. MUSt3R_Retriever from a synthetic checkpoint and codebook against the restatement on the same front-end features;
5. must3r_inference end to end (retrieval and linseq) against a direct inference_multi_ar call with the same order.
"""
import argparse
import os
import pickle

import numpy as np
import PIL.Image
import pytest
import torch

import asmk_ref as R
from must3r_amd import asmk as A
from test_ops_gpu import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fp32_bound(x, c):
    """per (row, centroid) bound of the fp32 ranking value |c|^2 - 2 x.c: the guide's 0.75-1.5e-7 * sum|a b| for the MFMA dot
    (taken as 2e-7), plus the roundings of |c|^2 and of the final subtraction"""
    xa, ca = np.abs(x).astype(np.float64), np.abs(c).astype(np.float64)
    dot = torch.from_numpy(xa) @ torch.from_numpy(ca).T
    csq = (ca * ca).sum(1)
    return (2 * 2e-7 * dot + 2e-7 * torch.from_numpy(csq)[None, :] + 2 ** -23 * (2 * dot + torch.from_numpy(csq)[None, :])).numpy()


def _data(M, K, D, seed):
    g = np.random.default_rng(seed)
    c = g.standard_normal((K, D)).astype(np.float32)
    x = (c[g.integers(0, K, M)] * 0.7 + g.standard_normal((M, D)).astype(np.float32) * 0.7).astype(np.float32)
    return x, c


def _quantize(x, c, k):
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV)
    return A.quantize(xd, cd, k).cpu().numpy()


@pytest.mark.parametrize("M,K,D,k", [(2049, 1000, 128, 5), (300, 16384, 256, 1), (300, 65536, 1024, 5), (1, 65536, 128, 1),
                                     (1, 1000, 1024, 5), (300, 1000, 256, 1), (2049, 16384, 128, 5)])
def test_quantize_against_fp64(M, K, D, k):
    x, c = _data(M, K, D, M + K + D + k)
    got = _quantize(x, c, k)
    d = R.sq_dist(x, c)
    order = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
    srt = np.take_along_axis(d, order, 1)
    eps = np.take_along_axis(_fp32_bound(x, c), order, 1).max(1)
    gaps = np.diff(srt, axis=1).min(1) if srt.shape[1] > 1 else np.full(M, np.inf)
    clear = gaps > 2 * eps
    assert clear.mean() > 0.9, clear.mean()   # the generator keeps most rows away from near-ties
    assert np.array_equal(got[clear], order[clear, :k])
    chosen = np.take_along_axis(d, got.astype(np.int64), 1)
    assert np.all(chosen <= srt[:, :k] + 2 * eps[:, None])
    assert np.all(np.sort(got, 1)[:, 1:] != np.sort(got, 1)[:, :-1]) if k > 1 else True
    assert np.array_equal(got, _quantize(x, c, k))                                  # repeatable bits
    record("asmk_quantize", M=M, K=K, D=D, k=k, clear_rows=float(clear.mean()),
           max_excess=float(np.max((chosen - srt[:, :k]) / eps[:, None])))


def test_quantize_ties_go_to_the_lower_id():
    x, c = _data(64, 1000, 128, 3)
    for dup in (500, 900, 999):
        c[dup] = c[17]
    x[:] = c[17] + np.random.default_rng(1).standard_normal((64, 128)).astype(np.float32) * 0.01
    got = _quantize(x, c, 5)
    assert np.all(got[:, :4] == np.array([17, 500, 900, 999]))


@pytest.mark.parametrize("K", [1000, 65536])
def test_quantize_non_finite_rows_give_real_ids(K):
    """a NaN or inf in a feature row makes every ranking value of the row NaN: the row still gets k real ids in [0, K)
    (quantize alone, no id is dereferenced here), and the other rows are unaffected"""
    x, c = _data(300, K, 128, 7)
    clean = _quantize(x, c, 5)
    x[3, 17] = np.nan
    x[40, :] = np.nan
    x[41, 5] = np.inf
    x[42, 9] = -np.inf
    got = _quantize(x, c, 5)
    assert got.min() >= 0 and got.max() < K
    assert np.all(np.sort(got, 1)[:, 1:] != np.sort(got, 1)[:, :-1])
    keep = np.setdiff1d(np.arange(300), [3, 40, 41, 42])
    assert np.array_equal(got[keep], clean[keep])
    c[5] = np.nan                                              # a NaN centroid is never preferred to a real one
    got = _quantize(x, c, 5)
    assert got.min() >= 0 and got.max() < K and not np.any(got[keep] == 5)


def test_non_finite_features_score_finite():
    x, c, _, offsets = _scores_case(11)
    x[offsets[1]] = np.nan
    x[offsets[2] + 1, 3] = np.inf
    got = A.ASMK(torch.from_numpy(c).to(DEV)).scores_numpy(torch.from_numpy(x).to(DEV), offsets)
    assert np.all(np.isfinite(got))


def test_aggregate_refuses_ids_outside_the_codebook():
    x, c = _data(300, 64, 128, 5)
    ids = _quantize(x, c, 5)
    offsets = np.array([0, 100, 200, 300])
    for bad in (0x7fffffff, 64, -1):
        wrong = ids.copy()
        wrong[150, 4] = bad                                   # image 1 only, in a column the database side does not read
        with pytest.raises(ValueError, match=r"images \[1\]"):
            _aggregate(x, c, wrong, offsets, 5)
        got, counts = _aggregate(x, c, wrong, offsets, 1)
        assert list(counts) == [len(w) for w, _ in R.aggregate(x, c, ids, offsets, 1)]
    with pytest.raises(ValueError, match="ids must be"):
        A.aggregate(torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(ids[:-1]).to(DEV), offsets, 5)


def test_centroid_norms_follow_in_place_updates():
    x, c = _data(300, 4096, 128, 8)
    cd = torch.from_numpy(c).to(DEV)
    before = A.quantize(torch.from_numpy(x).to(DEV), cd, 5).cpu().numpy()
    g = torch.Generator(device=DEV).manual_seed(0)
    cd.mul_(torch.rand((cd.shape[0], 1), device=DEV, generator=g) * 2)      # in place: the cached norms are stale
    assert torch.equal(A.centroid_sqnorm(cd), A.centroid_sqnorm(cd.clone()))
    after = A.quantize(torch.from_numpy(x).to(DEV), cd, 5).cpu().numpy()
    assert np.array_equal(after, A.quantize(torch.from_numpy(x).to(DEV), cd.clone(), 5).cpu().numpy())
    assert not np.array_equal(after, before)


def test_quantize_refusals():
    x, c = _data(8, 100, 96, 0)
    with pytest.raises(Exception, match="multiple of 64"):
        _quantize(x, c, 1)
    x, c = _data(8, 100, 128, 0)
    with pytest.raises(Exception, match="k must be"):
        _quantize(x, c, 9)
    x, c = _data(8, 4, 128, 0)
    with pytest.raises(Exception, match="exceeds"):
        _quantize(x, c, 5)


def _aggregate(x, c, ids, offsets, k_use):
    w, b, n = A.aggregate(torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(ids).to(DEV), offsets, k_use)
    w, b, n = w.cpu().numpy(), b.cpu().numpy().view(np.uint32), n.cpu().numpy()
    D = x.shape[1]
    return [(w[o * k_use:o * k_use + m], R.unpack_bits(b[o * k_use:o * k_use + m], D)) for o, m in zip(offsets[:-1], n)], n


@pytest.mark.parametrize("D", [128, 1024])
def test_aggregate_exact(D):
    rows = [300, 117, 1]
    offsets = np.concatenate([[0], np.cumsum(rows)])
    x, c = _data(int(offsets[-1]), 2048, D, D)
    x[:50] *= 1e3                         # large residuals: any change of summation order would show in the bits
    ids = _quantize(x, c, 5)
    for k_use in (1, 5):
        got, counts = _aggregate(x, c, ids, offsets, k_use)
        ref = R.aggregate(x, c, ids, offsets, k_use)
        assert list(counts) == [len(w) for w, _ in ref]
        for (gw, gb), (rw, rb) in zip(got, ref):
            assert np.all(np.diff(gw) > 0)
            assert np.array_equal(gw, rw) and np.array_equal(gb, rb)
    assert counts[2] <= 5


def test_aggregate_all_rows_on_one_word():
    x, c = _data(300, 64, 256, 9)
    g = np.random.default_rng(2)
    ids = np.stack([np.concatenate([[7], g.choice(np.setdiff1d(np.arange(64), [7]), 4, replace=False)]) for _ in range(300)]).astype(np.int32)
    offsets = np.array([0, 300])
    for k_use in (1, 5):
        got, counts = _aggregate(x, c, ids, offsets, k_use)
        ref = R.aggregate(x, c, ids, offsets, k_use)
        assert counts[0] == len(ref[0][0]) and (k_use == 5 or counts[0] == 1)
        assert np.array_equal(got[0][0], ref[0][0]) and np.array_equal(got[0][1], ref[0][1])


def test_aggregate_refuses_too_many_pairs():
    x, c = _data(820, 64, 128, 0)
    ids = _quantize(x, c, 5)
    with pytest.raises(ValueError, match="4096"):
        _aggregate(x, c, ids, np.array([0, 820]), 5)
    _aggregate(x, c, ids, np.array([0, 819, 820]), 5)


def _scores_case(seed, n=7, D=256, K=4096):
    g = np.random.default_rng(seed)
    rows = [int(v) for v in g.integers(1, 200, n)]
    rows[3] = 1
    offsets = np.concatenate([[0], np.cumsum(rows)])
    x, c = _data(int(offsets[-1]), K, D, seed)
    ids = _quantize(x, c, 5)
    # image 3 (one row) on words no other image uses: its scores against the others are 0
    others = np.delete(ids, offsets[3], axis=0)
    ids[offsets[3]] = np.setdiff1d(np.arange(K), others)[:5]
    return x, c, np.ascontiguousarray(ids, dtype=np.int32), offsets


@pytest.mark.parametrize("alpha,tau,normalize", [(3.0, 0.0, True), (3.0, 0.0, False), (1.0, 0.25, True), (2.5, 0.1, True)])
def test_scores_against_restatement(alpha, tau, normalize):
    x, c, ids, offsets = _scores_case(int(alpha * 10 + tau * 100))
    n, D = len(offsets) - 1, x.shape[1]
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV)
    idd = torch.from_numpy(ids).to(DEV)
    db = A.aggregate(xd, cd, idd, offsets, 1)
    q = A.aggregate(xd, cd, idd, offsets, 5)
    got = A.scores_from_aggregates(q, db, offsets, 5, 1, D, alpha, tau, normalize).cpu().numpy()
    qa, _ = _aggregate(x, c, ids, offsets, 5)
    da, _ = _aggregate(x, c, ids, offsets, 1)
    ref = R.scores(qa, da, D, alpha, tau, normalize)
    err = np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-300)
    record("asmk_scores", alpha=alpha, tau=tau, normalize=normalize, max_rel_row=float(err.max()))
    assert err.max() <= 2e-7, err
    assert np.all(got[3, np.arange(n) != 3] == 0) and np.all(got[np.arange(n) != 3, 3] == 0)
    assert not np.allclose(got, got.T)
    again = A.scores_from_aggregates(q, db, offsets, 5, 1, D, alpha, tau, normalize).cpu().numpy()
    assert np.array_equal(got, again)


def test_asmk_class_end_to_end_restatement():
    x, c, ids, offsets = _scores_case(5)
    m = A.ASMK(torch.from_numpy(c).to(DEV))
    got = m.scores_numpy(torch.from_numpy(x).to(DEV), offsets)
    ref = R.asmk_scores(x, c, offsets, ids=_quantize(x, c, 5))
    assert np.abs(got - ref).max() <= 2e-7 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4-5. MUSt3R_Retriever and must3r_inference
# ---------------------------------------------------------------------------------------------------------------------------------
def _models():
    from must3r_amd import synthetic as S
    from must3r_amd.config import SMALL
    import must3r_amd.model as M
    cfg = SMALL
    enc = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads)
    dec = M.MUSt3R(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth,
                   num_heads=cfg.dec_heads, feedback_type="single_mlp", memory_mode="kv")
    enc.load_state_dict(S.make_encoder_state_dict(cfg, 0))
    dec.load_state_dict(S.make_decoder_state_dict(cfg, 0))
    return cfg, enc.to(DEV).eval(), dec.to(DEV).eval()


def _retrieval_files(tmp_path, dim, K=1024, nfeat=100):
    from must3r_amd import synthetic as S
    args = argparse.Namespace(freeze_backbone=1, prewhiten=1, hdims=str(dim), residual=False, postwhiten=1, featweights="l2norm",
                              nfeat=nfeat, imsize=224, nclusters=K)
    ckpt = str(tmp_path / "ret_trainingfree.pth")
    torch.save({"args": args, "model": S.make_retrieval_state_dict(dim, seed=3)}, ckpt)
    cb = np.random.default_rng(4).standard_normal((K, dim)).astype(np.float32) * 0.05
    with open(tmp_path / "ret_codebook.pkl", "wb") as f:
        pickle.dump({"centroids": cb}, f)
    return ckpt, cb


def _pngs(tmp_path, n=6):
    g = np.random.default_rng(0)
    paths = []
    for i in range(n):
        H, W = (480, 640) if i % 2 else (700, 700)
        base = g.integers(0, 256, (H // 20 + 1, W // 20 + 1, 3)).astype(np.uint8)
        arr = np.asarray(PIL.Image.fromarray(base).resize((W, H), PIL.Image.BILINEAR))
        p = str(tmp_path / f"im{i}.png")
        PIL.Image.fromarray(arr).save(p)
        paths.append(p)
    return paths


def test_retriever_against_restatement(tmp_path):
    from must3r_amd import synthetic as S
    from must3r_amd.inference import encoder_multi_ar
    from must3r_amd.retrieval import MUSt3R_Retriever
    cfg, enc, _ = _models()
    ckpt, cb = _retrieval_files(tmp_path, cfg.enc_dim)
    ret = MUSt3R_Retriever(ckpt, backbone=enc, verbose=False)
    wide, square = S.make_images(3, 224, 288, 1)[0], S.make_images(3, 224, 224, 2)[0]
    imgs = [wide[0], square[0], wide[1], square[1], wide[2], square[2]]        # two aspect ratios, interleaved
    ts = torch.tensor([list(im.shape[-2:]) for im in imgs])
    x, _ = encoder_multi_ar(enc, [im.to(DEV) for im in imgs], ts, device=DEV)
    enc_list = [xi.unsqueeze(0).float() for xi in x]
    assert len({tuple(e.shape) for e in enc_list}) == 2
    got = ret(enc_list, device=DEV)
    assert got.dtype == np.float64 and got.shape == (6, 6)
    feats = [ret.model.forward_local(e)[0][0].cpu().numpy() for e in enc_list]   # the reference's per-image loop (:35-46)
    offsets = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])])
    flat = np.concatenate(feats)
    ids = _quantize(flat, cb, 5)
    ref = R.asmk_scores(flat, cb, offsets, ids=ids)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    record("asmk_retriever", max_rel=float(err))
    assert err <= 2e-7


@pytest.mark.parametrize("mode", ["retrieval", "linseq"])
def test_must3r_inference_end_to_end(tmp_path, mode):
    from must3r_amd import demo as Dm
    from must3r_amd.engine import postprocess
    from must3r_amd.image import load_images
    from must3r_amd.inference import encoder_multi_ar, inference_multi_ar
    from must3r_amd.retrieval import MUSt3R_Retriever
    cfg, enc, dec = _models()
    files = _pngs(tmp_path)
    retriever, seen = None, {}
    if mode == "retrieval":
        ckpt, _ = _retrieval_files(tmp_path, cfg.enc_dim)

        class Recording(MUSt3R_Retriever):
            def __call__(self, enc_list, device):
                seen["scores"] = super().__call__(enc_list, device)
                return seen["scores"]
        retriever = Recording(ckpt, backbone=enc, verbose=False)
    kw = dict(num_mem_images=4, max_bs=0, init_num_images=2, batch_num_views=1, render_once=False, is_sequence=mode == "linseq")
    np.random.seed(0)
    scene = Dm.must3r_inference((enc, dec), retriever, DEV, 224, False, files, verbose=False, **kw)
    order = [files.index(f) for f in scene.image_list]
    np.random.seed(0)
    keyframes = Dm.select_keyframes(seen.get("scores"), 6, 4, mode == "linseq")
    assert order[:4] == keyframes and sorted(order[4:]) == order[4:]
    # the same reconstruction, called directly
    views = load_images(files, 224, verbose=False)
    feats = None
    if mode == "retrieval":   # encoded in file order, as must3r_inference does before it ranks
        x, pos = encoder_multi_ar(enc, [v["img"] for v in views], torch.stack([torch.from_numpy(v["true_shape"]) for v in views]),
                                  device=DEV)
        feats = ([x[i] for i in order], [pos[i] for i in order])
    views = [views[i] for i in order]
    imgs = [v["img"] for v in views]
    shapes = [torch.from_numpy(v["true_shape"]).to(DEV) for v in views]
    mem_batches, to_render = Dm.memory_schedule(6, 4, 2, 1, False)
    _, direct = inference_multi_ar(enc, dec, imgs, [torch.tensor(i) for i in order], shapes, mem_batches, to_render=to_render,
                                   encoder_precomputed_features=feats, device=DEV, preserve_gpu_mem=True,
                                   post_process_function=lambda p: postprocess(p, compute_cam=True))
    for got, ref in zip(scene.x_out, direct):
        for key in ("pts3d", "conf", "focal", "c2w"):
            assert torch.equal(got[key].cpu(), ref[key].cpu()), key
    assert scene.focals == [float(d["focal"]) for d in direct]
    for im, s in zip(scene.imgs, scene.true_shape):
        assert im.shape == (int(s[0]), int(s[1]), 3) and im.min() >= 0 and im.max() <= 1
