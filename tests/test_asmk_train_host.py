"""CPU: the references and bounds of the codebook / whitening training (tests/kmeans_ref.py, tests/whiten_ref.py) discriminate, the whitening reference is the
reference's own ``pcawhitenlearn_shrinkage``, the codebook writer round-trips through ``asmk.read_codebook``, and the C surface is declared."""
import ast
import ctypes as C
import os
import pickletools
import re

import numpy as np
import pytest
import torch

import kmeans_ref
import whiten_ref
from conftest import HAS_REFERENCE, ROOT
from must3r_amd import _lib, asmk, asmk_train, retrieval

# numpy.linalg.eig against numpy.linalg.eigh on the covariance of whiten_ref.separated_sample() (condition number 512, neighbouring eigenvalues a factor 1.16
# apart), compared through P P^T and relative to its largest entry: measured 2.56e-14 (profiles/asmk_train_parity.txt).  Ten times that is allowed, because eig on
# a symmetric matrix has no orthogonality guarantee.
EIG_VS_EIGH_MEASURED = 2.56e-14
PPT_TOL = 10 * EIG_VS_EIGH_MEASURED


def kmeans_case(M, D, K, seed=0):
    """rows in K clusters with: ids 0 and K - 1 used, one empty cluster (id 1), one cluster of a single row (id 0), one cluster (id K - 1) holding
    round(3000 M / 4099) of the rows (3000 of 4099), rows scaled by 2^20 and 2^-20"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((M, D)).astype(np.float32)
    c = g.standard_normal((K, D)).astype(np.float32)
    if K == 1:
        ids = np.zeros((M,), dtype=np.int32)
    else:
        big, single, empty = K - 1, 0, 1
        free = [k for k in range(K) if k not in (big, single, empty)]
        n_big = round(3000 * M / 4099)
        perm = g.permutation(M)
        ids = g.choice(free, size=M).astype(np.int32)
        ids[perm[:n_big]] = big
        ids[perm[n_big]] = single
    x[::7] *= np.float32(2.0 ** 20)
    x[3::7] *= np.float32(2.0 ** -20)
    return x, c, ids


def check_update(got_new, got_counts, got_dist, got_obj, ref):
    """names of the outputs outside their bounds"""
    bad = []
    if not np.array_equal(np.asarray(got_counts, dtype=np.int64), ref["counts"]):
        bad.append("counts")
    if not np.all(np.abs(np.asarray(got_new, dtype=np.float64) - ref["new"]) <= ref["new_bound"]):
        bad.append("new")
    if not np.all(np.abs(np.asarray(got_dist) - ref["dist"]) <= ref["dist_bound"]):
        bad.append("dist")
    err, bound = kmeans_ref.objective_check(got_dist, got_obj)
    if not err <= bound:
        bad.append("objective")
    return bad


@pytest.mark.parametrize("shape", [(259, 64, 7), (4099, 128, 7)])
def test_kmeans_bounds_accept_the_clean_reference_and_reject_every_defect(shape):
    x, c, ids = kmeans_case(*shape)
    ref = kmeans_ref.update(x, c, ids)
    clean32 = ref["new"].astype(np.float32)      # what a correct kernel stores
    assert check_update(clean32, ref["counts"], ref["dist"], ref["objective"], ref) == []
    empty = np.nonzero(ref["counts"] == 0)[0]
    assert len(empty) == 1 and np.array_equal(clean32[empty], c[empty]) and int(ref["counts"][-1]) == round(3000 * shape[0] / 4099) and int(ref["counts"][0]) == 1
    for defect in kmeans_ref.DEFECTS:
        if defect == "fp32" and shape[0] < 1000:
            continue      # fp32 accumulation shows in the large cluster only
        bad = kmeans_ref.update(x, c, ids, defect=defect)
        assert "new" in check_update(bad["new"].astype(np.float32), bad["counts"], bad["dist"], bad["objective"], ref), defect
    # a distance with its last column dropped, an objective with its first row dropped (one of the rows scaled by 2^20: next to them a small row is below the bound)
    d = ((x.astype(np.float64) - c[ids])[:, :-1] ** 2).sum(1)
    assert "dist" in check_update(clean32, ref["counts"], d, ref["objective"], ref)
    assert "objective" in check_update(clean32, ref["counts"], ref["dist"], float(np.sum(ref["dist"][1:])), ref)
    wrong = ref["counts"].copy()
    wrong[-1] -= 1
    assert "counts" in check_update(clean32, wrong, ref["dist"], ref["objective"], ref)


def test_reseed_rule_reference():
    counts = np.array([3, 0, 2, 0, 1])
    dist = np.array([1.0, 5.0, 2.0, 5.0, 0.5, 7.0])
    empty, donors = kmeans_ref.reseed(counts, dist)
    assert empty.tolist() == [1, 3] and donors.tolist() == [5, 1]      # 7.0 first, then the tie at 5.0 to the lower row


def whiten_case(M, D, seed=0):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((M, D)) * g.uniform(0.5, 2.0, D) + g.standard_normal(D)).astype(np.float32)
    shift = x[:max(1, M // 4)].astype(np.float64).mean(axis=0)      # the first chunk's mean: not the mean of all rows
    return x, shift


def check_stats(S, s, n, ref):
    bad = []
    if not np.all(np.abs(S - ref["S"]) <= ref["S_bound"]):
        bad.append("S")
    if not np.array_equal(S, S.T):
        bad.append("symmetry")
    if not np.all(np.abs(s - ref["s"]) <= ref["s_bound"]):
        bad.append("s")
    if n != ref["n"]:
        bad.append("n")
    return bad


@pytest.mark.parametrize("shape", [(259, 128), (4099, 80)])
def test_whitening_bounds_accept_the_clean_reference_and_reject_every_defect(shape):
    x, shift = whiten_case(*shape)
    ref = whiten_ref.stats(x, shift)
    assert check_stats(ref["S"], ref["s"], ref["n"], ref) == []
    for defect in whiten_ref.DEFECTS:
        bad = whiten_ref.stats(x, shift, defect=defect)
        assert "S" in check_stats(bad["S"], bad["s"], bad["n"], ref), defect
    assert "symmetry" in check_stats(whiten_ref.stats(x, shift, defect="no_mirror")["S"], ref["s"], ref["n"], ref)
    # another association of the same sums stays inside: two halves added
    h = shape[0] // 2
    a, b = whiten_ref.stats(x[:h], shift), whiten_ref.stats(x[h:], shift)
    assert check_stats(a["S"] + b["S"], a["s"] + b["s"], a["n"] + b["n"], ref) == []


def reference_function(path, name, namespace):
    """one function of a reference file whose module cannot be imported here (un-vendored imports at its top), compiled out of its source; nothing is copied"""
    from oracle import ref_shims
    path = os.path.join(ref_shims.REFERENCE_ROOT, path)
    node = next(n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
    return namespace[name]


@pytest.mark.skipif(not HAS_REFERENCE, reason="runs the reference's code live; its tree is not present")
@pytest.mark.parametrize("shrink", [1.0, 0.5])
def test_whiten_ref_is_the_references_pcawhitenlearn_shrinkage(shrink):
    try:
        import importlib
        fn = importlib.import_module("must3r.retrieval.model").pcawhitenlearn_shrinkage
    except Exception:      # tqdm / dust3r are not here: the function itself needs numpy alone
        fn = reference_function("must3r/retrieval/model.py", "pcawhitenlearn_shrinkage", {"np": np})
    x, _ = whiten_ref.separated_sample()
    X = x.astype(np.float64)
    N = X.shape[0]
    m_ref, P_ref = fn(X, s=shrink)
    Xc = X - m_ref
    cov_ref = np.dot(Xc.T, Xc)
    cov_ref = (cov_ref + cov_ref.T) / (2 * N)
    ev = np.linalg.eigvalsh(cov_ref)
    assert ev.max() / ev.min() <= 1e3
    shift = X[:1000].mean(axis=0)
    st = whiten_ref.stats(x, shift)
    m, P, Xcov = whiten_ref.finish(st["S"], st["s"], st["n"], shrink, shift)
    assert m.shape == m_ref.shape and P.shape == P_ref.shape and P.dtype == P_ref.dtype
    # m = shift + s / n: the sum's bound over n, and the roundings of the two means themselves
    d = st["s"] / N
    m_bound = st["s_bound"] / N + 4 * whiten_ref.U64 * (np.abs(shift) + np.abs(d) + np.abs(m_ref[0]))
    assert np.all(np.abs(m - m_ref)[0] <= m_bound)
    # Xcov = S / n - d d^T against the reference's centred product, which carries the same bound on its own operands
    own = (N + 4) * whiten_ref.U64 * (np.abs(Xc).T @ np.abs(Xc))
    cov_bound = (st["S_bound"] + own) / N + 2 * np.outer(np.abs(d), st["s_bound"] / N + 2 * whiten_ref.U64 * np.abs(d)) + 4 * whiten_ref.U64 * np.abs(cov_ref)
    assert np.all(np.abs(Xcov - cov_ref) <= cov_bound)
    ppt, ppt_ref = P @ P.T, P_ref @ P_ref.T
    err = np.abs(ppt - ppt_ref).max() / np.abs(ppt_ref).max()
    print(f"P P^T of eigh (whiten_ref) against the reference's eig, shrink {shrink}: {err:.3e} of the largest entry (allowed {PPT_TOL:.3e})")
    assert err <= PPT_TOL
    # and the package's own host part is whiten_ref's
    m2, P2 = retrieval.whitening_from_stats(st["S"], st["s"], st["n"], shift, shrink)
    assert np.array_equal(m2, m) and np.array_equal(P2, P)


def test_eig_and_eigh_disagree_by_what_the_tolerance_was_measured_from():
    x, _ = whiten_ref.separated_sample()
    Xc = x.astype(np.float64) - x.astype(np.float64).mean(axis=0, keepdims=True)
    cov = np.dot(Xc.T, Xc)
    cov = (cov + cov.T) / (2 * x.shape[0])

    def ppt(eigval, eigvec):
        o = eigval.argsort()[::-1]
        P = np.dot(np.linalg.inv(np.diag(np.power(np.clip(eigval[o], 1e-14, None), 0.5))), eigvec[:, o].T).T
        return P @ P.T
    a, b = ppt(*np.linalg.eig(cov)), ppt(*np.linalg.eigh(cov))
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"eig against eigh through P P^T: {err:.3e} of the largest entry")
    assert err <= PPT_TOL


@pytest.mark.parametrize("ext", [".pkl", ".npy"])
def test_write_codebook_round_trips_bit_for_bit(tmp_path, ext):
    g = np.random.default_rng(3)
    c = g.standard_normal((37, 64)).astype(np.float32)
    c[0, 0], c[1, 1] = np.float32(-0.0), np.float32(1e-42)      # a signed zero and a denormal keep their bits
    path = asmk_train.write_codebook(str(tmp_path / ("model_codebook" + ext)), torch.from_numpy(c))
    back = asmk.read_codebook(path, nclusters=37)
    assert back.dtype == np.float32 and back.shape == c.shape and np.array_equal(back.view(np.uint32), c.view(np.uint32))
    with pytest.raises(ValueError):
        asmk.read_codebook(path, nclusters="64k")
    if ext == ".pkl":
        named = set()
        for op, arg, _ in pickletools.genops(open(path, "rb").read()):
            assert op.name not in ("STACK_GLOBAL", "INST", "OBJ", "EXT1", "EXT2", "EXT4"), op.name      # protocol 2: every global is a GLOBAL opcode with its text
            if op.name == "GLOBAL":
                named.add(tuple(arg.split(" ")))
        assert named and named <= asmk._PICKLE_GLOBALS, named - asmk._PICKLE_GLOBALS


def test_header_declares_the_entry_points_and_abi_21():
    hdr = open(os.path.join(ROOT, "include", "must3r_hip.h")).read()
    assert re.search(r"#define\s+MUST3R_HIP_ABI_VERSION\s+21\b", hdr) and _lib.ABI_VERSION == 21
    sz, i32, i64, vp = C.c_size_t, C.c_int, C.c_int64, C.c_void_p
    protos = {"must3r_hip_kmeans_update_scratch_bytes": (sz, [i32, i32]),
              "must3r_hip_kmeans_update": (i32, [vp, i32, i32, vp, i32, vp, i64, vp, vp, vp, vp, vp, C.POINTER(C.c_double), vp, vp, sz]),
              "must3r_hip_cov_accumulate_scratch_bytes": (sz, [i32, i32]),
              "must3r_hip_cov_accumulate": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, sz])}
    lib = _lib.load()
    for name, proto in protos.items():
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == proto and hasattr(lib, name), name
    assert "asmk_train.hip" in open(os.path.join(ROOT, "must3r_amd", "csrc", "Makefile")).read()
    # the refusals that need no device
    assert lib.must3r_hip_kmeans_update_scratch_bytes(0, 4) == 0 and lib.must3r_hip_cov_accumulate_scratch_bytes(10, 24) == 0
    assert lib.must3r_hip_cov_accumulate(None, 4, 16, None, None, None, None, None, None, 0) != 0 and b"null" in lib.must3r_hip_last_error()
    assert lib.must3r_hip_cov_accumulate(16, 4, 24, 16, 16, 16, 16, None, 16, 0) != 0 and b"multiple of 16" in lib.must3r_hip_last_error()
    assert lib.must3r_hip_cov_accumulate(20, 4, 16, 16, 16, 16, 16, None, 16, 1 << 30) != 0 and b"aligned" in lib.must3r_hip_last_error()
    assert lib.must3r_hip_kmeans_update(16, 4, 16, 16, 0, 16, 1, 16, 16, 16, 16, 16, None, None, 16, 1 << 30) != 0 and b"K must be" in lib.must3r_hip_last_error()
    assert lib.must3r_hip_kmeans_update(16, 4, 24, 16, 2, 16, 1, 16, 16, 16, 16, 16, None, None, 16, 1 << 30) != 0 and b"multiple of 16" in lib.must3r_hip_last_error()
    assert lib.must3r_hip_kmeans_update(16, 4, 16, 16, 2, None, 1, 16, 16, 16, 16, 16, None, None, 16, 1 << 30) != 0 and b"null" in lib.must3r_hip_last_error()
    assert lib.must3r_hip_kmeans_update(24, 4, 16, 16, 2, 16, 1, 16, 16, 16, 16, 16, None, None, 16, 1 << 30) != 0 and b"aligned" in lib.must3r_hip_last_error()
    assert lib.must3r_hip_kmeans_update(16, 4, 16, 16, 2, 16, 1, 16, 16, 16, 16, 16, None, None, 16, 8) != 0 and b"scratch" in lib.must3r_hip_last_error()


def test_train_codebook_refusals():
    x = torch.zeros((10, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asmk_train.train_codebook(x, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asmk_train.kmeans_update(x, x[:4], torch.zeros((10,), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.WhiteningStats(64, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.learn_whitening(x)
    assert asmk.parse_nclusters("64k") == 65536
    with pytest.raises(ValueError, match="cannot seed"):
        asmk_train.train_codebook(x, 11)
    with pytest.raises(ValueError, match="cannot seed"):
        asmk_train.train_codebook(x, "64k")
    with pytest.raises(ValueError, match="multiple of 64"):
        asmk_train.train_codebook(torch.zeros((10, 48)), 4)
