"""Host side of the retrieval back-end (must3r_amd.asmk, graph, demo, retrieval.Retriever; include/must3r_hip.h ABI 11), no GPU needed:

1. farthest_point_sampling / make_pairs_fps equal the reference's retrieval/graph.py under the same np.random seed;
2. the keyframe order, mem_batches and to_render of the native must3r_inference equal the reference's own must3r_inference
   (demo/inference.py:109-242) driven with the same scores, its loaders, encoder, retriever and decoder stubbed;
3. the ASMK restatement (tests/asmk_ref.py) on hand-worked cases;
4. the codebook reader's accepted layouts and its refusals (a pickle naming any other global is refused without running it);
5. wherever asmk is installed: asmk's own ASMKMethod against the restatement (settles the points DESIGN.md lists as parity unpinned).
"""
import argparse
import importlib
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import asmk_ref as R
from conftest import HAS_REFERENCE
from must3r_amd import asmk as A
from must3r_amd import demo as Dm
from must3r_amd import graph as G


def _ref_module(name):
    if not HAS_REFERENCE:
        pytest.skip("runs the reference's code live; its tree is not present")
    from oracle import ref_shims
    ref_shims.install()
    return importlib.import_module(name)


def _sim(rng, n):
    """an asymmetric score matrix whose diagonal (self-similarity) dominates, like the ASMK scores"""
    s = rng.random((n, n)) + rng.random((n, n)) * 0.1
    s[np.diag_indices(n)] = 1.5
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. graph.py
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fps_and_pairs_equal_reference():
    ref = _ref_module("must3r.retrieval.graph")
    rng = np.random.default_rng(0)
    cases = 0
    for n in list(range(1, 16)) + [20, 31, 45, 60]:
        for rep in range(3):
            sim = _sim(rng, n)
            if rep == 2:
                sim = np.round(sim, 1)     # ties in every argmax / argmin
            dist = 1 - sim
            for N, thr in ((max(1, n // 2), None), (n, None), (None, 0.5), (n, 0.3), (n + 2, None)):
                seed = int(rng.integers(1 << 30))
                np.random.seed(seed)
                ri, rd = ref.farthest_point_sampling(dist, N=N, dist_thresh=thr)
                after_ref = np.random.random()
                np.random.seed(seed)
                gi, gd = G.farthest_point_sampling(dist, N=N, dist_thresh=thr)
                assert np.random.random() == after_ref    # the same draws from np.random
                assert np.array_equal(ri, gi) and ri.dtype == gi.dtype, (n, N, thr)
                assert np.array_equal(rd, gd) and rd.dtype == gd.dtype, (n, N, thr)
                cases += 1
            for Na in (0, 1, min(n, 5), 20):
                for tokK in (0, 1, 3):
                    for thr in (None, 0.4):
                        seed = int(rng.integers(1 << 30))
                        np.random.seed(seed)
                        rp, rk = ref.make_pairs_fps(sim, Na=Na, tokK=tokK, dist_thresh=thr)
                        np.random.seed(seed)
                        gp, gk = G.make_pairs_fps(sim, Na=Na, tokK=tokK, dist_thresh=thr)
                        assert rp == gp, (n, Na, tokK, thr)
                        assert np.array_equal(rk, gk) and rk.dtype == gk.dtype
                        cases += 1
    assert cases > 1000


def test_fps_needs_n_or_threshold():
    with pytest.raises(ValueError):
        G.farthest_point_sampling(np.zeros((3, 3)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. must3r_inference: keyframes, mem_batches, to_render
# ---------------------------------------------------------------------------------------------------------------------------------
class _Encoder:
    patch_size = 16


class _Decoder:
    pass


def _fake_views(n):
    views = []
    for i in range(n):
        h, w = (224, 288) if i % 3 else (288, 224)
        img = torch.full((3, h, w), (i - n / 2) / n, dtype=torch.float32)
        views.append(dict(img=img, true_shape=np.int32([h, w])))
    return views


class _Record:
    def __init__(self, sim):
        self.sim = sim
        self.calls = []

    def load_images(self, filelist, size, patch_size=16, verbose=True, **kw):
        return _fake_views(len(filelist))

    def encoder_multi_ar(self, encoder, imgs, true_shape, **kw):
        n = len(imgs)
        return [torch.full((4, 8), float(i)) for i in range(n)], [torch.zeros((4, 2), dtype=torch.int64) for _ in range(n)]

    def retriever_class(self):
        rec = self

        class Retriever:
            def __init__(self, *a, **k):
                pass

            def __call__(self, enc, device):
                assert [int(e[0, 0, 0]) for e in enc] == list(range(len(enc)))   # the encoder tokens, in file order
                return rec.sim.copy()
        return Retriever

    def inference_multi_ar(self, encoder, decoder, imgs, img_ids, true_shape, mem_batches, to_render=None,
                           encoder_precomputed_features=None, **kw):
        ids = [int(v) for v in img_ids]
        if encoder_precomputed_features is not None:
            assert [int(x[0, 0]) for x in encoder_precomputed_features[0]] == ids
        self.calls.append(dict(img_ids=ids, mem_batches=list(mem_batches), to_render=None if to_render is None else list(to_render)))
        per = lambda i: dict(focal=torch.tensor(float(i)), c2w=torch.eye(4) * i)   # noqa: E731
        n_mem = sum(mem_batches)
        rest = range(len(ids)) if to_render is None else to_render
        return [per(ids[i]) for i in range(n_mem)], [per(ids[i]) for i in rest]


@pytest.fixture
def ref_demo(monkeypatch):
    if not HAS_REFERENCE:
        pytest.skip("runs the reference's demo/inference.py live; its tree is not present")
    from oracle import ref_shims
    ref_shims.install()

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        monkeypatch.setitem(sys.modules, name, m)
        return m

    class IndexFlatL2:
        def __init__(self, dim):
            self.dim = dim
    mod("faiss", IndexFlatL2=IndexFlatL2)     # no StandardGpuResources: processor.py takes its AttributeError branch

    class FaissL2Index:
        def __init__(self, *a, **k):
            pass
    asmk = mod("asmk")
    asmk.index = mod("asmk.index", FaissL2Index=FaissL2Index)
    asmk.asmk_method = mod("asmk.asmk_method", ASMKMethod=object)
    mod("dust3r.viz", rgb=lambda img, true_shape=None: ("rgb", tuple(int(v) for v in true_shape)))
    mod("dust3r.datasets", ImgNorm=None)
    mod("dust3r.datasets.utils")
    mod("dust3r.datasets.utils.transforms", ImgNorm=None)
    monkeypatch.setattr(sys.modules["dust3r.utils.image"], "_resize_pil_image", lambda *a, **k: None, raising=False)
    for name in [k for k in sys.modules if k.startswith("must3r.demo") or k.startswith("must3r.retrieval.processor")
                 or k.startswith("must3r.slam")]:
        monkeypatch.delitem(sys.modules, name)
    return importlib.import_module("must3r.demo.inference")


def _drive(module, monkeypatch, rec, retrieval_attr, **kw):
    monkeypatch.setattr(module, "load_images", rec.load_images)
    monkeypatch.setattr(module, "encoder_multi_ar", rec.encoder_multi_ar)
    monkeypatch.setattr(module, "inference_multi_ar", rec.inference_multi_ar)
    monkeypatch.setattr(module, retrieval_attr, rec.retriever_class())
    return module.must3r_inference((_Encoder(), _Decoder()), device="cpu", image_size=224, amp=False, viser_server=None,
                                   num_refinements_iterations=0, verbose=False, **kw)


def _cases():
    out = []
    for n, mem, init, bnv, once in ((1, 1, 1, 1, False), (5, 3, 1, 1, False), (8, 5, 2, 1, True), (8, 8, 2, 2, False),
                                    (12, 7, 3, 2, True), (20, 10, 2, 4, False), (20, 20, 1, 3, True), (30, 11, 4, 3, True),
                                    (17, 6, 1, 5, False), (40, 25, 2, 1, True)):
        for is_seq in (True, False):
            for retrieval in ("ckpt.pth", None):
                out.append(dict(n=n, num_mem_images=mem, init_num_images=init, batch_num_views=bnv, render_once=once,
                                is_sequence=is_seq, retrieval=retrieval))
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: "n{n}-m{num_mem_images}-i{init_num_images}-b{batch_num_views}-"
                         "r{render_once:d}-s{is_sequence:d}-{r}".format(r="ret" if c["retrieval"] else "none", **c))
def test_keyframes_and_schedule_equal_reference(ref_demo, monkeypatch, case):
    n = case["n"]
    rng = np.random.default_rng(n * 7 + case["num_mem_images"])
    sim = _sim(rng, n)
    files = [f"img{i:03d}.png" for i in range(n)]
    args = dict(retrieval=case["retrieval"], filelist=files, num_mem_images=case["num_mem_images"], max_bs=0,
                init_num_images=case["init_num_images"], batch_num_views=case["batch_num_views"], render_once=case["render_once"],
                is_sequence=case["is_sequence"])
    rec_ref, rec_nat = _Record(sim), _Record(sim)
    np.random.seed(11 + n)
    scene_ref = _drive(ref_demo, monkeypatch, rec_ref, "MUSt3R_Retriever", **args)
    np.random.seed(11 + n)
    scene_nat = _drive(Dm, monkeypatch, rec_nat, "MUSt3R_Retriever", **args)
    assert rec_ref.calls == rec_nat.calls
    assert scene_ref.image_list == scene_nat.image_list
    assert scene_ref.focals == scene_nat.focals
    assert all(torch.equal(a, b) for a, b in zip(scene_ref.cams2world, scene_nat.cams2world))
    mem = case["num_mem_images"]
    ranked = case["retrieval"] is not None and not case["is_sequence"]
    np.random.seed(11 + n)
    assert rec_nat.calls[0]["img_ids"][:mem] == Dm.select_keyframes(sim if ranked else None, n, mem, not ranked)


def test_select_keyframes_is_pure_and_seeded():
    rng = np.random.default_rng(3)
    sim = _sim(rng, 15)
    keep = sim.copy()
    np.random.seed(5)
    a = Dm.select_keyframes(sim, 15, 6, False)
    np.random.seed(5)
    b = Dm.select_keyframes(sim, 15, 6, False)
    assert a == b and len(set(a)) == 6 and all(isinstance(v, int) for v in a)
    assert np.array_equal(sim, keep)
    assert Dm.select_keyframes(None, 10, 4, True) == [0, 3, 6, 9]


def test_rgb_crops_and_clips():
    img = torch.linspace(-1.5, 1.5, 3 * 6 * 8).reshape(3, 6, 8)
    out = Dm.rgb(img, torch.tensor([4, 5]))
    assert out.shape == (4, 5, 3)
    assert out.min() >= 0 and out.max() <= 1
    assert np.allclose(out, np.clip(img.numpy().transpose(1, 2, 0)[:4, :5] * 0.5 + 0.5, 0, 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the restatement on hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_hand_worked():
    D = 64
    # image 0: one row on word 2, image 1: one row on word 2 with 16 of 64 signs flipped
    c = np.zeros((4, D), np.float32)
    x0 = np.ones(D, np.float32)
    x1 = np.ones(D, np.float32)
    x1[:16] = -1
    c[2] = 0
    feat = np.stack([x0, x1])
    ids = np.array([[2], [2]])
    aggs = R.aggregate(feat, c, ids, [0, 1, 2], 1)
    assert [list(w) for w, _ in aggs] == [[2], [2]]
    s = 1 - 2 * 16 / 64                          # 0.5
    got = R.scores(aggs, aggs, D, alpha=3.0, tau=0.0)
    assert got[0, 1] == got[1, 0] == np.float32(s) ** 3 == 0.125
    assert got[0, 0] == 1.0
    assert R.scores(aggs, aggs, D, alpha=1.0, tau=0.0)[0, 1] == 0.5
    assert R.scores(aggs, aggs, D, alpha=3.0, tau=0.6)[0, 1] == 0.0        # below the threshold
    # normalisation: image 0 has words {1, 2}, image 1 has {2}; the shared word has identical bits
    feat = np.stack([x0, x0, x0])
    ids = np.array([[1], [2], [2]])
    aggs = R.aggregate(feat, c, ids, [0, 2, 3], 1)
    assert R.scores(aggs, aggs, D, normalize=False)[0, 1] == 1.0
    assert R.scores(aggs, aggs, D, normalize=True)[0, 1] == pytest.approx(1 / np.sqrt(2))
    # no shared word -> 0
    aggs = R.aggregate(feat, c, np.array([[1], [1], [3]]), [0, 2, 3], 1)
    assert R.scores(aggs, aggs, D)[0, 1] == 0.0


def test_restatement_residual_is_sequential_fp32():
    rng = np.random.default_rng(1)
    D = 64
    feat = (rng.standard_normal((50, D)) * 1e3).astype(np.float32)
    feat[1::2] += np.float32(1e-3)
    c = rng.standard_normal((3, D)).astype(np.float32)
    ids = np.zeros((50, 1), np.int64)
    (w, bits), = R.aggregate(feat, c, ids, [0, 50], 1)
    r = np.zeros(D, np.float32)
    for j in range(50):
        r = r + (feat[j] - c[0])
    assert np.array_equal(bits[0], r > 0)
    assert np.array_equal(R.unpack_bits(R.pack_bits(bits), D), bits)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. codebook reader
# ---------------------------------------------------------------------------------------------------------------------------------
class Boom:
    ran = []

    def __reduce__(self):
        return (Boom._explode, ())

    @staticmethod
    def _explode():
        Boom.ran.append(True)
        return np.zeros((2, 64), np.float32)


def test_codebook_layouts(tmp_path):
    c = np.random.default_rng(0).standard_normal((10, 64)).astype(np.float32)
    layouts = {
        "flat.pkl": c,
        "dict.pkl": {"centroids": c, "params": {"size": 10}},
        "nested.pkl": {"codebook": {"centroids": c.astype(np.float64), "meta": [1, 2.0, "x", (3,)]}},
        "other_key.pkl": {"state": {"cb": c}, "ids": np.arange(10)},
    }
    for name, obj in layouts.items():
        with open(tmp_path / name, "wb") as f:
            pickle.dump(obj, f)
        got = A.read_codebook(tmp_path / name, nclusters=10)
        assert np.array_equal(got.astype(np.float32), c), name
    np.save(tmp_path / "cb.npy", c)
    assert np.array_equal(A.read_codebook(tmp_path / "cb.npy"), c)
    torch.save(torch.from_numpy(c), tmp_path / "cb.pt")
    assert np.array_equal(A.read_codebook(tmp_path / "cb.pt"), c)
    torch.save({"centroids": torch.from_numpy(c)}, tmp_path / "cbd.pt")
    assert np.array_equal(A.read_codebook(tmp_path / "cbd.pt"), c)
    assert A.parse_nclusters("64k") == 65536 and A.parse_nclusters(65536) == 65536 and A.parse_nclusters("1000") == 1000
    with pytest.raises(ValueError, match="64k"):
        A.read_codebook(tmp_path / "cb.npy", nclusters="64k")


def test_codebook_refusals(tmp_path):
    with open(tmp_path / "evil.pkl", "wb") as f:
        pickle.dump({"centroids": Boom()}, f)
    with pytest.raises(pickle.UnpicklingError, match="evil.pkl"):
        A.read_codebook(tmp_path / "evil.pkl")
    assert Boom.ran == []
    with open(tmp_path / "ns.pkl", "wb") as f:
        pickle.dump({"centroids": argparse.Namespace(a=1)}, f)
    with pytest.raises(pickle.UnpicklingError, match="argparse.Namespace"):
        A.read_codebook(tmp_path / "ns.pkl")
    with open(tmp_path / "two.pkl", "wb") as f:
        pickle.dump({"a": np.zeros((2, 64)), "b": np.zeros((3, 64))}, f)
    with pytest.raises(ValueError, match="two.pkl"):
        A.read_codebook(tmp_path / "two.pkl")
    with open(tmp_path / "junk.pkl", "wb") as f:
        f.write(b"not a pickle at all")
    with pytest.raises((ValueError, pickle.UnpicklingError), match="junk.pkl"):
        A.read_codebook(tmp_path / "junk.pkl")
    with pytest.raises(FileNotFoundError):
        A.read_codebook(tmp_path / "missing.pkl")


def test_asmk_refuses_other_kernels():
    for kw in (dict(binary=False), dict(use_idf=True), dict(multiple_assignment=(1, 3))):
        with pytest.raises(NotImplementedError):
            A.ASMK(torch.zeros((4, 64)), **kw)


def test_codebook_path_follows_processor():
    from must3r_amd.retrieval import codebook_path
    assert codebook_path("/x/y/MUSt3R_512_retrieval_trainingfree.pth") == "/x/y/MUSt3R_512_retrieval_codebook.pkl"


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. asmk itself, wherever it is installed
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_against_asmk(tmp_path):
    pytest.importorskip("faiss")
    asmk_method = pytest.importorskip("asmk.asmk_method")
    rng = np.random.default_rng(0)
    D, K, n, per = 128, 64, 6, 40
    train = rng.standard_normal((4000, D)).astype(np.float32)
    params = {"index": {"gpu_id": 0}, "train_codebook": {"codebook": {"size": K}},
              "build_ivf": {"kernel": {"binary": True}, "ivf": {"use_idf": False}, "quantize": {"multiple_assignment": 1},
                            "aggregate": {}},
              "query_ivf": {"quantize": {"multiple_assignment": 5}, "aggregate": {}, "search": {"topk": None},
                            "similarity": {"similarity_threshold": 0.0, "alpha": 3.0}}}
    method = asmk_method.ASMKMethod.initialize_untrained(params)
    cache = str(tmp_path / "cb_codebook.pkl")
    method = method.train_codebook(train, cache_path=cache)
    centroids = A.read_codebook(cache, nclusters=K)                 # the pickle layout
    feat = rng.standard_normal((n * per, D)).astype(np.float32)
    ids = np.repeat(np.arange(n), per)
    ds = method.build_ivf(feat, ids)
    _, _, ranks, ranked = ds.query_ivf(feat, ids)
    scores = np.empty_like(ranked)
    scores[np.arange(ranked.shape[0])[:, None], ranks] = ranked
    ref = R.asmk_scores(feat, centroids, np.arange(n + 1) * per)  # normalisation and tie order
    assert np.allclose(scores, ref, rtol=1e-5, atol=1e-6)
