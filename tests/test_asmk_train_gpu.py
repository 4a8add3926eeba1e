"""GPU (-m gpu): training the ASMK codebook and learning the whitening on the device (csrc/asmk_train.hip; must3r_amd.asmk_train, must3r_amd.retrieval) against
the float64 references and bounds of tests/kmeans_ref.py and tests/whiten_ref.py.

1. the update within its bounds at four shapes (one row; odd sizes; an empty cluster, a cluster of one row and one holding three quarters of the rows; rows scaled
   by 2^20 and 2^-20), exact counts, bit-equal repeats, a cluster's centroid independent of every other row, ids read through a row stride;
2. ids outside [0, K) refused with every output and the canaries around them untouched;
3. the covariance within its bounds at four shapes, exactly symmetric, bit-equal repeats; two chunkings agree within the sum of their bounds (NOT bit for bit:
   the sums associate differently); learn_whitening whitens a sample of known covariance;
4. train_codebook equals its steps written out by hand, recovers eight separated blobs, its objective never rises by more than the fp32 search can misrank, and
   its empty-cluster rule picks the reference rule's rows (with an exact tie);
5. both entry points run wholly on the caller's stream (the technique of tests/test_stream_order_gpu.py);
6. end to end: front-end features -> train_codebook -> write_codebook -> MUSt3R_Retriever scores equal to the restatement on the trained centroids.
"""
import os

import numpy as np
import pytest
import torch

import asmk_ref
import kmeans_ref
import stream_forms as SF
import test_stream_order_gpu as SO
import whiten_ref
from must3r_amd import _lib, asmk, asmk_train, retrieval
from test_asmk_train_host import check_stats, check_update, kmeans_case, whiten_case
from test_ops_gpu import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARITY = os.environ.get("M3R_ASMK_TRAIN_PARITY")      # a file that receives the measured figures (kept as profiles/asmk_train_parity.txt)
delay = SO.delay


def note(line):
    print(line)
    if PARITY:
        with open(PARITY, "a") as f:
            f.write(line + "\n")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_update(x, c, ids):
    new, counts, dist, obj = asmk_train.kmeans_update(dev(x), dev(c), ids if isinstance(ids, torch.Tensor) else dev(ids))
    return new, counts, dist, obj


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the update
# ---------------------------------------------------------------------------------------------------------------------------------
_ref_cache = {}


def update_case(shape):
    """(x, c, ids, reference): computed once per shape and shared, never modified"""
    if shape not in _ref_cache:
        x, c, ids = kmeans_case(*shape)
        _ref_cache[shape] = (x, c, ids, kmeans_ref.update(x, c, ids))
    return _ref_cache[shape]


SHAPES = [(1, 64, 1), (259, 64, 7), (4099, 128, 7), (4099, 192, 300)]


@pytest.mark.parametrize("shape", SHAPES)
def test_update_against_fp64(shape):
    x, c, ids, ref = update_case(shape)
    M, D, K = shape
    assert ids.min() == 0 and ids.max() == K - 1
    new, counts, dist, obj = run_update(x, c, ids)
    new_h, counts_h, dist_h, obj_h = new.cpu().numpy(), counts.cpu().numpy(), dist.cpu().numpy(), float(obj.item())
    assert new.dtype == torch.float32 and counts.dtype == torch.int32 and dist.dtype == torch.float64 and obj.dtype == torch.float64
    e_new = float((np.abs(new_h.astype(np.float64) - ref["new"]) / np.maximum(ref["new_bound"], 1e-300))[ref["counts"] > 0].max())
    e_dist = float((np.abs(dist_h - ref["dist"]) / np.maximum(ref["dist_bound"], 1e-300)).max())
    e_obj, b_obj = kmeans_ref.objective_check(dist_h, obj_h)
    note(f"kmeans_update {shape}: centroid error / bound {e_new:.3f}, dist error / bound {e_dist:.3f}, objective error {e_obj:.3e} (bound {b_obj:.3e})")
    record("kmeans_update", M=M, D=D, K=K, centroid_ratio=e_new, dist_ratio=e_dist)
    assert check_update(new_h, counts_h, dist_h, obj_h, ref) == []
    empty = np.nonzero(ref["counts"] == 0)[0]
    assert np.array_equal(new_h[empty].view(np.uint32), c[empty].view(np.uint32))      # an empty cluster's centroid comes back bit for bit
    if K > 1:
        assert len(empty) >= 1 and (ref["counts"] == 1).any()
    if M == 4099:
        assert int(ref["counts"][K - 1]) == 3000
    # the planted defects are seen at this shape too (tests/test_asmk_train_host.py shows it for every defect)
    if M > 1:
        bad = kmeans_ref.update(x, c, ids, defect="drop_last")
        assert "new" in check_update(bad["new"].astype(np.float32), bad["counts"], bad["dist"], bad["objective"], ref)


def test_update_is_repeatable_and_a_cluster_depends_on_its_own_rows_alone():
    x, c, ids, ref = update_case((4099, 128, 7))
    a, b = run_update(x, c, ids), run_update(x, c, ids)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    big = 6
    mine = ids == big
    # every other cluster's rows replaced by other data and spread over other clusters
    g = np.random.default_rng(9)
    x2, ids2 = x.copy(), ids.copy()
    x2[~mine] = g.standard_normal((int((~mine).sum()), x.shape[1])).astype(np.float32) * 3
    ids2[~mine] = g.integers(0, big, int((~mine).sum())).astype(np.int32)
    assert torch.equal(run_update(x2, c, ids2)[0][big], a[0][big])
    # and removed: the cluster alone, as cluster 0 of a one-cluster call
    alone = run_update(x[mine], c[big:big + 1], np.zeros((int(mine.sum()),), dtype=np.int32))
    assert torch.equal(alone[0][0], a[0][big]) and int(alone[1][0]) == int(mine.sum())
    # the ids as column 0 of a [M, 5] tensor, read in place through the row stride
    wide = torch.full((x.shape[0], 5), -7, dtype=torch.int32, device=DEV)      # the other columns hold bad ids: they are not read
    wide[:, 0] = dev(ids)
    c5 = run_update(x, c, wide)
    assert all(torch.equal(p, q) for p, q in zip(a, c5))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_id", ["K", "-1"])
def test_update_refuses_ids_outside_the_codebook(bad_id):
    M, D, K = 259, 64, 7
    x, c, ids, _ = update_case((M, D, K))
    ids = ids.copy()
    ids[100] = K if bad_id == "K" else -1
    xd, cd, idd = dev(x), dev(c), dev(ids)
    order = torch.sort(idd, stable=True).indices
    lib = _lib.load()
    sizes = dict(new=K * D * 4, counts=K * 4, dist=M * 8, objective=8)
    guard = 4096
    arena = torch.full((guard * (len(sizes) + 1) + sum((n + 255) // 256 * 256 for n in sizes.values()),), 0xA5, dtype=torch.uint8, device=DEV)
    ptr, off = {}, guard
    for k, n in sizes.items():
        ptr[k] = arena.data_ptr() + off
        off += (n + 255) // 256 * 256 + guard
    assert arena.data_ptr() % 256 == 0
    nbytes = lib.must3r_hip_kmeans_update_scratch_bytes(M, K)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    rc = lib.must3r_hip_kmeans_update(xd.data_ptr(), M, D, cd.data_ptr(), K, idd.data_ptr(), 1, order.data_ptr(), ptr["new"], ptr["counts"], ptr["dist"],
                                      ptr["objective"], None, _lib.stream_ptr(DEV), scratch.data_ptr(), nbytes)
    assert rc != 0
    with pytest.raises(_lib.HipError, match=r"outside \[0, 7\)"):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((arena == 0xA5).all()), "a refused call wrote an output or a canary"
    with pytest.raises(_lib.HipError, match="outside"):      # and through the wrapper
        asmk_train.kmeans_update(xd, cd, idd)
    # a good call into the same arena writes the outputs and nothing else
    good = dev(update_case((M, D, K))[2])
    order = torch.sort(good, stable=True).indices
    _lib.check(lib.must3r_hip_kmeans_update(xd.data_ptr(), M, D, cd.data_ptr(), K, good.data_ptr(), 1, order.data_ptr(), ptr["new"], ptr["counts"], ptr["dist"],
                                            ptr["objective"], None, _lib.stream_ptr(DEV), scratch.data_ptr(), nbytes))
    torch.cuda.synchronize()
    keep = torch.ones_like(arena, dtype=torch.bool)
    for k, n in sizes.items():
        o = ptr[k] - arena.data_ptr()
        keep[o:o + n] = False
    assert bool((arena[keep] == 0xA5).all())
    ref_new = asmk_train.kmeans_update(xd, cd, good)[0]
    o = ptr["new"] - arena.data_ptr()
    assert torch.equal(arena[o:o + sizes["new"]].view(torch.float32).view(K, D), ref_new)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the covariance and the whitening
# ---------------------------------------------------------------------------------------------------------------------------------
def run_cov(chunks, shift, D):
    st = retrieval.WhiteningStats(D, DEV)
    st.shift = dev(shift)
    for ch in chunks:
        st.add(dev(ch))
    return st.S.cpu().numpy(), st.s.cpu().numpy(), float(st.n.item())


COV_SHAPES = [(1, 16), (5, 80), (259, 128), (4099, 80)]


@pytest.mark.parametrize("shape", COV_SHAPES)
def test_cov_against_fp64(shape):
    M, D = shape
    x, shift = whiten_case(M, D)
    if M == 5:
        shift = shift + 0.25      # (a shift that is not a mean of the rows either)
    ref = whiten_ref.stats(x, shift)
    S, s, n = run_cov([x], shift, D)
    ratio = float((np.abs(S - ref["S"]) / np.maximum(ref["S_bound"], 1e-300)).max()) if M > 1 else 0.0
    note(f"cov_accumulate {shape}: S error / bound {ratio:.3f}")
    record("cov_accumulate", M=M, D=D, S_ratio=ratio)
    assert check_stats(S, s, n, ref) == []
    assert np.array_equal(S, S.T)
    S2, s2, n2 = run_cov([x], shift, D)
    assert np.array_equal(S, S2) and np.array_equal(s, s2) and n == n2 == M
    if M > 16:
        for defect in whiten_ref.DEFECTS:
            bad = whiten_ref.stats(x, shift, defect=defect)
            assert "S" in check_stats(bad["S"], bad["s"], bad["n"], ref), defect


def test_cov_chunkings_agree_within_their_bounds_not_bit_for_bit():
    """one call over 4099 rows and three calls over (1000, 3000, 99) of them sum in different associations: equal within the sum of the two bounds, and the test
    does not ask for equal bits"""
    M, D = 4099, 80
    x, shift = whiten_case(M, D)
    ref = whiten_ref.stats(x, shift)
    S1, s1, n1 = run_cov([x], shift, D)
    S3, s3, n3 = run_cov([x[:1000], x[1000:4000], x[4000:]], shift, D)
    assert n1 == n3 == M
    assert np.all(np.abs(S1 - S3) <= 2 * ref["S_bound"]) and np.all(np.abs(s1 - s3) <= 2 * ref["s_bound"])
    assert check_stats(S3, s3, n3, ref) == [] and np.array_equal(S3, S3.T)
    note(f"cov_accumulate chunkings (4099,) against (1000, 3000, 99): bit-equal S {np.array_equal(S1, S3)}, largest difference / bound "
         f"{float((np.abs(S1 - S3) / ref['S_bound']).max()):.3f}")


def test_learn_whitening_whitens_a_sample_of_known_covariance():
    D = 64
    x, cov_true = whiten_ref.separated_sample(N=4099, D=D, seed=11)
    m, P = retrieval.learn_whitening(dev(x))
    assert m.shape == (1, D) and P.shape == (D, D) and m.dtype == P.dtype == np.float64
    shift = x.astype(np.float64).mean(axis=0)      # (any shift gives the same covariance)
    st = whiten_ref.stats(x, shift)
    m_ref, _, cov_ref = whiten_ref.finish(st["S"], st["s"], st["n"], 1.0, shift)
    N, u = x.shape[0], whiten_ref.U64
    # m = shift + s / n: the rounding of the shift itself cancels in the sum; what is left is the bound of s over n (twice: the reference's own) and the
    # roundings of the division and the addition
    assert np.all(np.abs(m - m_ref)[0] <= 2 * st["s_bound"] / N + 8 * u * np.abs(m_ref[0]))
    # E = P^T cov_ref P - I.  P whitens the covariance eigh saw exactly up to eigh's backward error (a perturbation of norm <= D u |cov|_2, taken entrywise) and the
    # roundings of forming P ((D + 4) u per entry of the triple product); that covariance differs from cov_ref by the two bounds of the statistics over n
    # (the device's sums and the reference's, whose shifts differ: both are bounded by their own |u| sums; the device's is at most the reference's taken around
    # the first-chunk mean, which here is the mean of all rows).
    d = st["s"] / N
    cov_bound = 2 * st["S_bound"] / N + 2 * np.outer(np.abs(d) + np.abs(m - m_ref)[0], st["s_bound"] / N + 2 * u * (np.abs(d) + np.abs(m - m_ref)[0]))

    def whitening_error(P):
        aP = np.abs(P)
        bound = aP.T @ (cov_bound + D * u * np.linalg.norm(cov_ref, 2)) @ aP + 2 * (D + 4) * u * (aP.T @ np.abs(cov_ref) @ aP)
        E = P.T @ cov_ref @ P - np.eye(D)
        return E, float((np.abs(E) / bound).max())
    E, ratio = whitening_error(P)
    note(f"learn_whitening D {D}, 4099 rows, condition number 500: |P^T cov P - I| max {np.abs(E).max():.3e}, largest error / propagated bound {ratio:.3f}")
    record("learn_whitening", D=D, max_abs=float(np.abs(E).max()), ratio=ratio)
    assert ratio <= 1.0
    # the sample's covariance is the planted one to sampling error: the test's data is what it says
    assert np.abs(cov_ref - cov_true).max() < 0.1
    # Whitener.learn_ writes the same numbers in place, from a sample or from statistics fed in chunks of another size
    w = retrieval.Whitener(D).to(DEV)
    w.learn_(dev(x))
    assert np.array_equal(w.m.detach().cpu().numpy(), m) and np.array_equal(w.p.detach().cpu().numpy(), P)
    stats = retrieval.WhiteningStats(D, DEV)
    for lo in range(0, N, 1500):
        stats.add(dev(x[lo:lo + 1500]).view(-1, 1, D))      # [..., dim]
    w.learn_(stats)
    assert whitening_error(w.p.detach().cpu().numpy())[1] <= 1.0
    # the whitened sample has unit covariance at the precision of the fp32 output: each entry of y carries a relative 2^-24, so an entry of the covariance
    # 2 * 2^-24 * mean |y_a| |y_b| <= 1.2e-7 (Cauchy-Schwarz, unit variances); 1e-5 leaves room for E and the fp64 affine map
    y = w(dev(x).view(1, N, D))
    yc = y[0].double().cpu().numpy()
    assert np.abs(yc.T @ yc / N - np.eye(D)).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the loop
# ---------------------------------------------------------------------------------------------------------------------------------
def blobs(n_per=50, D=64, K=8, seed=2):
    """K Gaussian blobs of unit standard deviation whose centres lie 25 sqrt 2 = 35 standard deviations apart: no assignment is near a tie in fp32"""
    g = np.random.default_rng(seed)
    labels = np.repeat(np.arange(K), n_per).astype(np.int32)
    x = (g.standard_normal((K * n_per, D)) + 25.0 * np.eye(K, D)[labels]).astype(np.float32)
    perm = g.permutation(K * n_per)
    return x[perm], labels[perm]


def test_train_codebook_equals_its_steps_by_hand_and_recovers_blobs():
    x, labels = blobs()
    first = np.array([int(np.nonzero(labels == k)[0][0]) for k in range(8)])      # one initial point per blob
    xd = dev(x)
    C0 = xd[dev(first)].clone()
    cent, log = asmk_train.train_codebook(xd, 8, niter=3, init=C0)
    hand = C0.clone()
    objs = []
    for _ in range(3):
        ids = asmk.quantize(xd, hand, 1, c_sqnorm=asmk.centroid_sqnorm(hand, refresh=True))
        new, counts, dist, obj = asmk_train.kmeans_update(xd, hand, ids)
        assert int((counts == 0).sum()) == 0
        objs.append(float(obj.item()))
        hand = new
    assert torch.equal(cent, hand) and [e["objective"] for e in log] == objs and all(e["empty"] == 0 for e in log)
    assert torch.equal(C0, xd[dev(first)])      # init is not written
    final = asmk.quantize(xd, cent, 1).cpu().numpy()[:, 0]
    assert np.array_equal(final, labels)
    ref = kmeans_ref.update(x, np.zeros((8, 64), dtype=np.float32), labels)
    assert np.all(np.abs(cent.cpu().numpy().astype(np.float64) - ref["new"]) <= ref["new_bound"])
    # the same with the seeded initialisation: rows torch.randperm(M, seeded CPU generator)[:K]
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(5))[:8]
    a, _ = asmk_train.train_codebook(xd, 8, niter=2, seed=5)
    b, _ = asmk_train.train_codebook(xd, 8, niter=2, init=xd[perm.to(DEV)])
    assert torch.equal(a, b)


def test_objective_never_rises_by_more_than_the_search_can_misrank():
    """Lloyd's step lowers the objective twice: the mean minimises the sum over a cluster (the stored centroid is its fp32 rounding: a relative 2^-24 of |c|, far
    inside the slack), and the nearest centroid minimises each row's term.  The search ranks by |c|^2 - 2 x.c in fp32, whose error per (row, centroid) is at most
    (D + 3) 2^-24 (|x|^2 + |c|^2); a row can therefore be given a centroid whose true distance exceeds the smallest by twice that: the slack of one iteration is
    sum_rows (D + 3) 2^-23 (|x|^2 + max_c |c|^2).  Overlapping data, K = 20, so that the assignment keeps changing."""
    g = np.random.default_rng(4)
    M, D, K = 2000, 64, 20
    x = (g.standard_normal((M, D)) * 2.0 + g.standard_normal((1, D))).astype(np.float32)
    xd = dev(x)
    cent = xd[:K].clone()
    prev, objs = None, []
    x2 = (x.astype(np.float64) ** 2).sum(1)
    for it in range(6):
        c2 = float((cent.double() ** 2).sum(1).max())
        cent_next, log = asmk_train.train_codebook(xd, K, niter=1, init=cent)
        obj = log[0]["objective"]
        slack = float(((D + 3) * 2.0 ** -23 * (x2 + c2)).sum())
        if prev is not None:
            note(f"k-means objective, iteration {it}: {obj:.9e} after {prev:.9e} (slack {slack:.3e})")
            assert obj <= prev + slack
        prev, cent = obj, cent_next
        objs.append(obj)
    assert objs[-1] < objs[0]      # and it did fall


def test_empty_clusters_take_the_rows_of_the_reference_rule():
    g = np.random.default_rng(6)
    M, D, K = 300, 64, 6
    x = g.standard_normal((M, D)).astype(np.float32)
    x[40] = x[40] * 0 + 9.0                      # the largest distance
    x[200] = x[200] * 0 - 7.0                    # then an exact tie: rows 77 and 200 are the same vector
    x[77] = x[200]
    init = x[[0, 1, 2, 3]].copy()
    far = np.full((2, D), 1000.0, dtype=np.float32)
    init = np.concatenate([init[:1], far[:1], init[1:3], far[1:], init[3:]])      # clusters 1 and 4 stay empty
    xd, cd = dev(x), dev(init)
    ids = asmk.quantize(xd, cd, 1)
    new, counts, dist, _ = asmk_train.kmeans_update(xd, cd, ids)
    dist_h = dist.cpu().numpy()
    assert dist_h[77] == dist_h[200] and np.argsort(-dist_h, kind="stable")[:3].tolist() == [40, 77, 200]
    empty_ref, donors_ref = kmeans_ref.reseed(counts.cpu().numpy(), dist_h)
    assert empty_ref.tolist() == [1, 4] and donors_ref.tolist() == [40, 77]
    before = new.clone()
    empty, donors = asmk_train.reseed_empty(new, counts, dist, xd)
    assert empty.tolist() == empty_ref.tolist() and donors.tolist() == donors_ref.tolist()
    assert torch.equal(new[1], xd[40]) and torch.equal(new[4], xd[77])
    keep = [0, 2, 3, 5]
    assert torch.equal(new[keep], before[keep])      # the donors stay in their old clusters' means
    cent, log = asmk_train.train_codebook(xd, K, niter=1, init=cd)
    assert log[0]["empty"] == 2 and torch.equal(cent, new)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. stream order: the technique of tests/test_stream_order_gpu.py on the two new entry points (through ctypes: the stream argument is _lib.stream_ptr's)
# ---------------------------------------------------------------------------------------------------------------------------------
def _kmeans_spec():
    M, D, K = 700, 64, 9
    ids = torch.randint(0, K, (M,), generator=SF.gen(0, 300), dtype=torch.int32)
    order = torch.sort(ids, stable=True).indices

    def inputs(s):
        g = SF.gen(s, 301)
        return dict(feat=SF.rn(g, M, D), cent=SF.rn(g, K, D), ids=ids.clone(), order=order.clone())

    def run(d):
        sc = d["scratch"]
        _lib.check(SF.L().must3r_hip_kmeans_update(SF.P(d["feat"]), M, D, SF.P(d["cent"]), K, SF.P(d["ids"]), 1, SF.P(d["order"]), SF.P(d["new"]), SF.P(d["counts"]),
                                                    SF.P(d["dist"]), SF.P(d["obj"]), None, SF.ST(), SF.P(sc), sc.numel()))
    return SF.Spec(inputs, run, outs=("new", "dist", "obj"), shared=("ids", "order"), ranges=dict(ids=(0, K), order=(0, M)),
                   bufs=dict(new=((K, D), SF.f32), counts=((K,), SF.i32), dist=((M,), SF.f64), obj=((1,), SF.f64),
                             scratch=SF.nbytes(lambda: SF.L().must3r_hip_kmeans_update_scratch_bytes(M, K))))


def _cov_spec():
    M, D = 700, 80

    def inputs(s):
        g = SF.gen(s, 302)
        a = SF.rn(g, D, D).double()
        return dict(x=SF.rn(g, M, D) + 0.5, shift=SF.rn(g, D).double(), S=a + a.t(), s=SF.rn(g, D).double(), n=torch.tensor([3.0 + s], dtype=SF.f64))

    def run(d):
        sc = d["scratch"]
        _lib.check(SF.L().must3r_hip_cov_accumulate(SF.P(d["x"]), M, D, SF.P(d["shift"]), SF.P(d["S"]), SF.P(d["s"]), SF.P(d["n"]), SF.ST(), SF.P(sc), sc.numel()))
    return SF.Spec(inputs, run, outs=("S", "s", "n"), bufs=dict(scratch=SF.nbytes(lambda: SF.L().must3r_hip_cov_accumulate_scratch_bytes(M, D))))


STREAM_CASES = {
    "kmeans_update": SF.Case("kmeans_update", ["must3r_hip_kmeans_update"], "asmk_train.hip", _kmeans_spec, True,
                             "include/must3r_hip.h, must3r_hip_kmeans_update: the call reads one 16-byte record back to refuse bad ids: it synchronises `stream`; only "
                             "the bits are held, as for must3r_hip_export_count", True),
    "cov_accumulate": SF.Case("cov_accumulate", ["must3r_hip_cov_accumulate"], "asmk_train.hip", _cov_spec, False, None, True),
}
_bound = {}


def stream_bound(name):
    if name not in _bound:
        b = SO.Bound(STREAM_CASES[name])
        ref_a = b.reference("A")
        ref_a2, host_ms, _ = b.reference("A", timed=True)
        assert not SO.same_bits(ref_a, ref_a2)
        ref_b = b.reference("B")
        assert SO.differing_fraction(ref_a, ref_b) > 0.5
        _bound[name] = (b, ref_a, ref_b, host_ms)
    return _bound[name]


@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_entry_point_runs_on_the_callers_stream(delay, name):
    case = STREAM_CASES[name]
    b, ref_a, ref_b, host0_ms = stream_bound(name)
    ms = SO.delay_for(host0_ms)
    b.load("B")
    b.fill()
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        b.load("A")
        outs = b.call()
        premise = not done.query()
        got = {k: v.clone() for k, v in outs.items()}
        b.load("B")
        b.fill()
    s.synchronize()
    if not case.syncs:
        assert premise, f"{name}: delay too short or undocumented host synchronisation"
    bad = SO.same_bits(got, ref_a)
    assert not bad, f"{name}: on a side stream {bad} differ from the default-stream bits (equal to the decoy's: {not SO.same_bits(got, ref_b)})"


@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_control_on_the_null_stream_reads_the_decoy(delay, name):
    b, ref_a, ref_b, host0_ms = stream_bound(name)
    ms = SO.delay_for(host0_ms)
    b.load("B")
    b.fill()
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        b.load("A")
        with SO.null_stream():
            outs = b.call()
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.cuda.default_stream().synchronize()
            got = {k: v.clone() for k, v in outs.items()}
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"{name}: the delay ({ms:.1f} ms) ended before the null stream was idle"
    bad = SO.same_bits(got, ref_b)
    assert not bad, f"{name}: a call on the null stream did not give the decoy's bits in {bad}"


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trained_codebook_serves_the_retriever(tmp_path):
    from must3r_amd import synthetic as S
    from must3r_amd.inference import encoder_multi_ar
    from test_asmk_gpu import _models, _quantize, _retrieval_files
    K = 64
    cfg, enc, _ = _models()
    ckpt, _ = _retrieval_files(tmp_path, cfg.enc_dim, K=K)
    wide, square = S.make_images(3, 224, 288, 1)[0], S.make_images(3, 224, 224, 2)[0]
    imgs = [wide[0], square[0], wide[1], square[1], wide[2], square[2]]
    ts = torch.tensor([list(im.shape[-2:]) for im in imgs])
    x, _ = encoder_multi_ar(enc, [im.to(DEV) for im in imgs], ts, device=DEV)
    enc_list = [xi.unsqueeze(0).float() for xi in x]
    model, _ = retrieval.load_frontend(ckpt, enc, DEV)
    feat, offsets = retrieval.frontend_local_features(model, enc_list, DEV)
    assert feat.shape[0] >= K and feat.shape[1] % 64 == 0
    cent, log = asmk_train.train_codebook(feat, K, niter=4, seed=1)
    assert len(log) == 4 and log[-1]["objective"] < log[0]["objective"]
    path = asmk_train.write_codebook(retrieval.codebook_path(ckpt), cent)
    assert np.array_equal(asmk.read_codebook(path, nclusters=K).view(np.uint32), cent.cpu().numpy().view(np.uint32))
    m = asmk.ASMK(path)
    assert torch.equal(m.codebook, cent)
    ret = retrieval.MUSt3R_Retriever(ckpt, backbone=enc, verbose=False)      # loads the trained codebook next to the checkpoint
    got = ret(enc_list, device=DEV)
    flat, cb = feat.cpu().numpy(), cent.cpu().numpy()
    ref = asmk_ref.asmk_scores(flat, cb, offsets, ids=_quantize(flat, cb, 5))
    err = np.abs(got - ref).max() / np.abs(ref).max()
    record("asmk_train_retriever", max_rel=float(err))
    assert got.shape == (6, 6) and err <= 2e-7
    assert np.abs(m.scores_numpy(feat, offsets) - ref).max() <= 2e-7 * np.abs(ref).max()


def test_command_line_writes_the_codebook_the_retriever_loads(tmp_path, capsys):
    """python -m must3r_amd.asmk_train: a MUSt3R checkpoint, a retrieval checkpoint and a folder of images in, the codebook next to the retrieval checkpoint out"""
    import must3r_amd.model as M
    from must3r_amd.config import SMALL
    from test_asmk_gpu import _pngs, _retrieval_files
    from test_zz_r04_gpu import _ckpt
    K = 64
    weights = _ckpt(tmp_path, SMALL)
    ckpt, _ = _retrieval_files(tmp_path, SMALL.enc_dim, K=K)
    os.remove(retrieval.codebook_path(ckpt))      # the synthetic one: the tool has to make its own
    (tmp_path / "imgs").mkdir()
    _pngs(tmp_path / "imgs", n=4)
    out = asmk_train.main(["--weights", weights, "--retrieval", ckpt, "--images", str(tmp_path / "imgs"), "--nclusters", str(K), "--niter", "2", "--image_size", "224"])
    assert out == retrieval.codebook_path(ckpt) and "k-means iteration 1" in capsys.readouterr().out
    cb = asmk.read_codebook(out, nclusters=K)
    assert cb.shape == (K, SMALL.enc_dim) and np.isfinite(cb).all()
    enc, _ = M.load_model(weights, device="cuda", verbose=False)
    ret = retrieval.MUSt3R_Retriever(ckpt, backbone=enc, verbose=False)
    assert np.array_equal(ret.asmk.codebook.cpu().numpy().view(np.uint32), cb.view(np.uint32))
