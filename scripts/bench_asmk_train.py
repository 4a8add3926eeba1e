"""Training the retrieval mode's artefacts on the GPU (must3r_amd.asmk_train, must3r_amd.retrieval.WhiteningStats; csrc/asmk_train.hip).

(a) one k-means iteration at D = 1024, K = 65 536, M = 655 360 (10 rows per centroid), split into the search (asmk.quantize, k = 1), the grouping
    (torch.sort(ids, stable=True)) and the update (must3r_hip_kmeans_update); the update also as bytes moved over time against the 6.3 TB/s copy rate the README
    uses, and against the composed torch form on the same tensors (index_add_ into fp64, bincount, a gathered distance).
(b) must3r_hip_cov_accumulate at D = 1024 on 768 x 1000 rows: time and fp64 FLOP/s (the lower triangle's M D (D + 64) flops it performs, and the 2 M D^2 of the
    full product for comparison), against torch.matmul in float64 on the same centred tensor on the same GPU, and against the reference's numpy routine
    (pcawhitenlearn_shrinkage's mean, centring and [D, M] x [M, D] product) on <= 16 host threads.

Every figure is a median with its min and max over the repetitions of ONE run in which the forms alternate (native, torch, native, ...), device-event times.
One JSON line per part; --out appends nothing, it rewrites the file.  --quick: a tenth of the rows and K.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from must3r_amd import asmk, asmk_train, retrieval  # noqa: E402

COPY_RATE = 6.3e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))


def torch_update(x, c, ids):
    """the composed torch form of the update: fp64 index_add_ (atomics: not repeatable), bincount, gathered distance"""
    idl = ids.reshape(-1).long()
    sums = torch.zeros(c.shape, dtype=torch.float64, device=x.device).index_add_(0, idl, x.double())
    counts = torch.bincount(idl, minlength=c.shape[0])
    new = torch.where(counts[:, None] > 0, (sums / counts.clamp(min=1)[:, None]).float(), c)
    dist = (x.double() - c.double()[idl]).square().sum(1)
    return new, counts, dist, dist.sum()


def bench_kmeans(M, K, D, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    c = torch.randn((K, D), device="cuda", generator=g)
    x = torch.empty((M, D), device="cuda")
    for r0 in range(0, M, 65536):
        n = min(65536, M - r0)
        x[r0:r0 + n] = c[torch.randint(0, K, (n,), device="cuda", generator=g)] * 0.7 + torch.randn((n, D), device="cuda", generator=g) * 0.7
    csq = asmk.centroid_sqnorm(c)
    ids = asmk.quantize(x, c, 1, c_sqnorm=csq)
    asmk_train.kmeans_update(x, c, ids)
    torch_update(x, c, ids)
    torch.cuda.synchronize()
    t = dict(search=[], grouping=[], update=[], torch_update=[])
    for _ in range(reps):
        t["search"].append(timed(lambda: asmk.quantize(x, c, 1, c_sqnorm=csq))[0])
        t["grouping"].append(timed(lambda: torch.sort(ids[:, 0], stable=True))[0])
        t["update"].append(timed(lambda: asmk_train.kmeans_update(x, c, ids))[0])      # (includes the grouping: the wrapper sorts)
        t["torch_update"].append(timed(lambda: torch_update(x, c, ids))[0])
    upd = [u - s for u, s in zip(t["update"], t["grouping"])]
    nbytes = 2.0 * M * D * 4 + 2.0 * K * D * 4 + M * (8 + 8 + 4)      # the rows twice (sums, distances), centroids read and written, dist, order, ids
    new, counts, dist, obj = asmk_train.kmeans_update(x, c, ids)
    tn, tc, td, to = torch_update(x, c, ids)
    line = dict(part="kmeans_iteration", M=M, K=K, D=D, search=summary(t["search"]), grouping=summary(t["grouping"]),
                update_with_grouping=summary(t["update"]), update_kernels=summary(upd), torch_composed_update=summary(t["torch_update"]),
                search_tflops=2.0 * M * K * D / statistics.median(t["search"]) / 1e9,
                update_bytes=nbytes, update_tb_per_s=nbytes / statistics.median(upd) / 1e9, update_frac_of_copy_rate=nbytes / statistics.median(upd) / 1e-3 / COPY_RATE,
                update_over_torch=statistics.median(t["update"]) / statistics.median(t["torch_update"]),
                agreement=dict(counts_equal=bool(torch.equal(counts.long(), tc)), centroid_max_abs=float((new - tn).abs().max()),
                               objective_rel=float(abs(obj.item() - to.item()) / to.item())))
    return line


def bench_cov(M, D, reps, cpu):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty((M, D), device="cuda")
    for r0 in range(0, M, 65536):
        n = min(65536, M - r0)
        x[r0:r0 + n] = torch.randn((n, D), device="cuda", generator=g) * 0.5 + 0.1
    shift = (x.sum(dim=0, dtype=torch.float64) / M).contiguous()

    def native():
        st = retrieval.WhiteningStats(D, "cuda")
        st.shift = shift
        return st.add(x)
    xc = x.double() - shift

    def torch_f64():
        return xc.t() @ xc
    native()
    torch_f64()
    torch.cuda.synchronize()
    t = dict(native=[], torch_f64=[])
    for _ in range(reps):
        t["native"].append(timed(native)[0])
        t["torch_f64"].append(timed(torch_f64)[0])
    st, ref = native(), torch_f64()
    med, medt = statistics.median(t["native"]), statistics.median(t["torch_f64"])
    nt = (D + 63) // 64
    done = 2.0 * M * 64 * 64 * nt * (nt + 1) / 2
    line = dict(part="cov_accumulate", M=M, D=D, native=summary(t["native"]), torch_matmul_f64=summary(t["torch_f64"]),
                native_fp64_tflops_performed=done / med / 1e9, native_fp64_tflops_full_product_equivalent=2.0 * M * D * D / med / 1e9,
                torch_matmul_f64_tflops_measured=2.0 * M * D * D / medt / 1e9, native_over_torch=med / medt,
                note="torch.matmul float64 runs on the already centred float64 tensor (its 2 x larger input is not counted); the native call centres fp32 rows itself",
                agreement_max_rel=float(((st.S - ref).abs().max() / ref.abs().max()).item()), symmetric=bool(torch.equal(st.S, st.S.t())))
    if cpu:
        X = x.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        m = X.mean(axis=0, keepdims=True)
        Xc = X - m
        np.dot(Xc.T, Xc)
        line["reference_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        line["reference_numpy"] = f"mean, centring and np.dot(Xc.T, Xc) of pcawhitenlearn_shrinkage in float64 on {torch.get_num_threads()} host threads, one run"
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true")
    p.add_argument("--no-cpu", action="store_true")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    K = 6144 if a.quick else 65536
    lines = [bench_kmeans(10 * K, K, 1024, a.reps)]
    print(json.dumps(lines[-1]), flush=True)
    lines.append(bench_cov(76800 if a.quick else 768000, 1024, a.reps, cpu=not a.no_cpu))
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    main()
