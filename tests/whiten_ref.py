"""The reference arithmetic of the whitening statistics (csrc/asmk_train.hip, must3r_hip_cov_accumulate; must3r_amd.retrieval.WhiteningStats) in numpy float64,
with bounds that count the roundings of a correct kernel.  u_r = double(x_r) - shift carries one rounding per element; with u = 2^-53:

    S[a, b]   |got - ref| <= (M + 4) u sum_r |u_ra| |u_rb|     M products (the fp64 MFMA rounds each fused step once) and M - 1 additions in any order, the two
                                                               subtractions behind each product, and the reference's own rounding
    s[a]      |got - ref| <= (M + 1) u sum_r |u_ra|

``finish`` is the host part of ``pcawhitenlearn_shrinkage`` (must3r/retrieval/model.py:18-35) from those statistics, with ``numpy.linalg.eigh``.

``defect`` plants what a wrong kernel could do, for the CPU test that shows the bounds see it: ``"fp32"`` (products and sums in fp32), ``"no_mirror"`` (the upper
triangle of S never written), ``"shift_one"`` (the shift left out of the row operand: sum_r x_r u_r^T), ``"drop_tail"`` (the rows behind the last whole 16-row slab
left out).  Shared by tests/test_asmk_train_host.py and tests/test_asmk_train_gpu.py.
"""
import numpy as np

U64 = 2.0 ** -53
DEFECTS = ("fp32", "no_mirror", "shift_one", "drop_tail")


def stats(x, shift, defect=None):
    """-> dict(S [D, D], s [D], n, S_bound, s_bound) of fp32 rows ``x`` [M, D] and a float64 ``shift`` [D]"""
    x64, shift = np.asarray(x, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    M, D = x64.shape
    u = x64 - shift
    S_clean, s_clean = u.T @ u, u.sum(axis=0)
    S, s = S_clean, s_clean
    if defect == "fp32":
        u32 = u.astype(np.float32)
        S, s = (u32.T @ u32).astype(np.float64), u32.sum(axis=0, dtype=np.float32).astype(np.float64)
    elif defect == "no_mirror":
        S = np.tril(S_clean)
    elif defect == "shift_one":
        S = x64.T @ u
    elif defect == "drop_tail":
        keep = u[:M - M % 16] if M % 16 else u[:M - 16]
        S, s = keep.T @ keep, keep.sum(axis=0)
    a = np.abs(u)
    return dict(S=S, s=s, n=float(M), S_bound=(M + 4) * U64 * (a.T @ a), s_bound=(M + 1) * U64 * a.sum(axis=0))


def finish(S, s, n, shrink=1.0, shift=None):
    """-> (m [1, D], P [D, D], Xcov [D, D]): d = s / n, m = shift + d, Xcov = S / n - d d^T, then model.py:27-35 with eigh"""
    S, s = np.asarray(S, dtype=np.float64), np.asarray(s, dtype=np.float64)
    d = s / n
    m = (d if shift is None else np.asarray(shift, dtype=np.float64) + d)[None, :]
    Xcov = S / n - np.outer(d, d)
    eigval, eigvec = np.linalg.eigh(Xcov)
    order = eigval.argsort()[::-1]
    eigval, eigvec = np.clip(eigval[order], a_min=1e-14, a_max=None), eigvec[:, order]
    P = np.dot(np.linalg.inv(np.diag(np.power(eigval, 0.5 * shrink))), eigvec.T)
    return m, P.T, Xcov


def separated_sample(N=4000, D=32, cond=5e2, seed=5, mean=0.5):
    """fp32 rows [N, D] whose covariance has geometrically spaced eigenvalues from 1 down to 1 / cond (so the sample's are separated too), around ``mean``"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = np.geomspace(1.0, 1.0 / cond, D)
    return ((rng.standard_normal((N, D)) * np.sqrt(lam)) @ q.T + mean).astype(np.float32), (q * lam) @ q.T
