"""Retrieval back-end (must3r_amd.asmk; csrc/asmk.hip) on the GPU: n images x 300 local features, D = 1024, K = 65 536.

Reported per size (one JSON line each): device-event times of the quantize (top-5 search, split + merge), the two aggregates
(database k = 1, query k = 5) and the scores; the quantize's achieved TF/s (2 M K D FLOP) and its share of the fp32 matrix peak
(157.3 TF/s); and MUSt3R_Retriever.__call__ end to end from encoder tokens [1, 768, 1024] (front-end + back-end, host result).
Baseline, labelled as such: the same top-5 search as a torch fp32 GEMM + topk on <= 16 CPU threads (the reference's own route --
asmk with a faiss index -- cannot run on these machines).  Kernel names: run this under `rocprofv3 --kernel-trace --stats`
(a separate run; --quick shortens it).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from must3r_amd import asmk as A  # noqa: E402

PEAK_F32 = 157.3e12


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def _cpu_quantize(x, c, k, chunk=2048):
    csq = (c * c).sum(1)
    for r0 in range(0, x.shape[0], chunk):
        torch.topk(csq[None, :] - 2 * x[r0:r0 + chunk] @ c.T, k, dim=1, largest=False)


def bench(n, per, D, K, reps, cpu):
    g = torch.Generator(device="cuda").manual_seed(n)
    c = torch.randn((K, D), device="cuda", generator=g)
    x = c[torch.randint(0, K, (n * per,), device="cuda", generator=g)] * 0.7 + torch.randn((n * per, D), device="cuda", generator=g) * 0.7
    offsets = np.arange(n + 1) * per
    A.centroid_sqnorm(c)
    q_ms, ids = _time(lambda: A.quantize(x, c, 5), reps)
    db_ms, db = _time(lambda: A.aggregate(x, c, ids, offsets, 1), reps)
    qa_ms, qa = _time(lambda: A.aggregate(x, c, ids, offsets, 5), reps)
    s_ms, _ = _time(lambda: A.scores_from_aggregates(qa, db, offsets, 5, 1, D), reps)
    flop = 2.0 * n * per * K * D
    line = dict(n_images=n, features_per_image=per, D=D, K=K, quantize_ms=q_ms, aggregate_db_ms=db_ms, aggregate_query_ms=qa_ms,
                scores_ms=s_ms, backend_ms=q_ms + db_ms + qa_ms + s_ms, quantize_tflops=flop / q_ms / 1e9,
                quantize_peak_frac=flop / q_ms / 1e-3 / PEAK_F32)
    if cpu:
        xc, cc = x.cpu(), c.cpu()
        t0 = time.perf_counter()
        _cpu_quantize(xc, cc, 5)
        line["baseline_cpu_torch_quantize_ms"] = (time.perf_counter() - t0) * 1e3
        line["baseline"] = f"torch fp32 GEMM + topk on {torch.get_num_threads()} CPU threads (quantize only)"
    return line


def bench_retriever(n, reps, tmp):
    import argparse as ap
    import pickle
    from must3r_amd import synthetic as S
    from must3r_amd.retrieval import MUSt3R_Retriever
    dim = 1024
    args = ap.Namespace(freeze_backbone=1, prewhiten=1, hdims=str(dim), residual=False, postwhiten=1, featweights="l2norm", nfeat=300,
                        imsize=512, nclusters="64k")
    ckpt = os.path.join(tmp, "bench_trainingfree.pth")
    torch.save({"args": args, "model": S.make_retrieval_state_dict(dim, seed=0)}, ckpt)
    with open(os.path.join(tmp, "bench_codebook.pkl"), "wb") as f:
        pickle.dump({"centroids": np.random.default_rng(0).standard_normal((65536, dim)).astype(np.float32) * 0.05}, f)

    class Backbone:
        enc_embed_dim = dim
    ret = MUSt3R_Retriever(ckpt, backbone=Backbone(), verbose=False)
    g = torch.Generator(device="cuda").manual_seed(1)
    enc = [torch.randn((1, 768 if i % 2 else 672, dim), device="cuda", generator=g) for i in range(n)]
    ret(enc, "cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ret(enc, "cuda")
    return dict(n_images=n, retriever_call_ms=(time.perf_counter() - t0) * 1e3 / reps, tokens="672 / 768 x 1024, two aspect ratios")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quick", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sizes = [20, 200] if a.quick else [20, 200, 1000]
    lines = []
    for n in sizes:
        lines.append(bench(n, 300, 1024, 65536, 2 if a.quick else 5, cpu=(n <= 200 and not a.quick)))
        print(json.dumps(lines[-1]), flush=True)
    with tempfile.TemporaryDirectory() as tmp:   # a 256 MiB codebook: never next to the results
        for n in ([20] if a.quick else [20, 200]):
            lines.append(bench_retriever(n, 3, tmp))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
