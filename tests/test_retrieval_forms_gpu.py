"""GPU (-m gpu): every entry point of csrc/retrieval.hip through the C ABI (must3r_hip_affine in fp64 and fp32, _row_norm, _topk_gather, _weighted_spoc,
_l2_normalize, _layernorm_act_f32) and the Python layer over them, against fp64 references of the same fp32 inputs (tests/retrieval_forms.py: case tables,
operands, references, per-element bounds, canary-filled destinations, checks; tests/test_retrieval_forms_host.py shows that those checks see planted defects).
The shapes are the smallest at which each kernel can still go wrong: sizes around the 64-wide tiles and waves, K around the 16-wide K tile, one element, several
blocks.  Besides the values: canaries round every output, repeats bit-equal, a block of rows alone against the same rows in the batch, NaN / inf confined to
their row, top-k without any tolerance (NaN keys included: the library under test is the one with the total order).

Every row is printed before anything is asserted on it, and goes to the file M3R_RETRIEVAL_TABLE names (kept as profiles/retrieval_forms.txt).  The ratios there
are measurements; the bounds are not, and do not move to fit a run."""
import math
import os
import time

import pytest
import torch

import retrieval_forms as R
from test_ops_gpu import record   # the suite's one metrics log

pytestmark = pytest.mark.gpu
DEV = "cuda"
_rows = []     # (entry point, case, what, figure)


@pytest.fixture(scope="module", autouse=True)
def _table():
    t0 = time.time()
    yield
    path = os.environ.get("M3R_RETRIEVAL_TABLE")
    if not (_rows and path):
        return
    with open(path, "w") as f:
        f.write("# tests/test_retrieval_forms_gpu.py: every entry point of csrc/retrieval.hip against fp64.  ratio = max |got - fp64| / bound per element, bounds of\n"
                "# tests/retrieval_forms.py (affine fp32 (K + 4) u (s + |resid|); fp64 u |v| + u |v + resid| + (K + 4) 2^-53 (s + |resid|); row_norm (C/2 + 2) u; l2 (L/2 + 4) u;\n"
                "# spoc: sum, norm and normalisation terms); layernorm_act: grad_parity.compare per row kind, e in units of 2^-24 max|fp64|, ratio = e_gpu / (4 e_ref + 32);\n"
                "# top-k: cases that equal the stable descending sort bit for bit (no tolerance).\n"
                f"# wall time of the file: {time.time() - t0:.0f} s\n")
        f.write(f"{'entry point':<20}{'case':<44}{'what':<34}{'figure':>12}\n")
        for e, c, w, v in _rows:
            f.write(f"{e:<20}{c:<44}{w:<34}{v:>12}\n")
        worst = {}
        for e, c, w, v in _rows:
            if w.startswith("ratio"):
                worst[e] = max(worst.get(e, 0.0), float(v))
        for e, v in worst.items():
            f.write(f"# worst ratio, {e}: {v:.4f}\n")


def row(entry, case, what, figure):
    fig = f"{figure:.4f}" if isinstance(figure, float) else str(figure)
    print(f"{entry} {case}: {what} {fig}")
    _rows.append((entry, case, what, fig))


@pytest.fixture(scope="module")
def lib():
    from must3r_amd import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- affine
def run_affine(lib, ops, A=None, resid=None, rows=None):
    """one must3r_hip_affine call into a fresh canary-filled destination; A / resid / rows: a block of rows of the case"""
    c = ops["case"]
    A = ops["A"] if A is None else A
    M = c["M"] if rows is None else rows
    resid = ops["resid"] if resid is None else resid
    dest = R.Guarded((M, c["N"]), DEV)
    if ops["alias"]:
        dest.fill(resid)
    rp = dest.view if ops["alias"] else resid
    lib.check(lib.load().must3r_hip_affine(c["double"], _p(A), _p(ops["sub"]), _p(ops["B"]), c["bt"], _p(ops["bias"]), _p(rp), _p(dest.view), M, c["N"], c["K"],
                                           _stream()))
    torch.cuda.synchronize()
    return dest


@pytest.mark.parametrize("shape", R.AFFINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bt", [0, 1])
@pytest.mark.parametrize("double", [1, 0], ids=["f64", "f32"])
def test_affine_against_fp64(lib, double, bt, shape):
    bad = []
    worst = 0.0
    for c in R.affine_cases():
        if (c["double"], c["bt"], (c["M"], c["N"], c["K"])) != (double, bt, shape):
            continue
        M, N, K = shape
        ops = R.affine_operands(c, DEV)
        dest = run_affine(lib, ops)
        r, fails = R.affine_check(ops, dest)
        row("affine", c["name"], "ratio", r)
        worst = max(worst, r)
        again = run_affine(lib, ops)
        if not torch.equal(again.bits, dest.bits):
            fails.append("a second launch gives other bits")
        r0 = M // 3                      # the rows from M / 3 on, alone: other places in the tiles, the same bits
        part = run_affine(lib, ops, A=ops["A"][r0:], resid=None if ops["resid"] is None else ops["resid"][r0:], rows=M - r0)
        fails += part.failures("rows alone")
        if not torch.equal(R.bits(part.view), R.bits(dest.view[r0:])):
            fails.append("a block of rows alone gives other bits than in the batch")
        if c["opt"] in ("all", "none") and c["kind"] == "scaled":      # NaN and inf in one row of A stay in that row
            A2 = ops["A"].clone()
            rr = M // 2
            A2[rr, 0], A2[rr, K - 1] = float("nan"), (float("inf") if K > 1 else float("nan"))
            hot = run_affine(lib, ops, A=A2)
            keep = torch.ones(M, dtype=torch.bool, device=DEV)
            keep[rr] = False
            fails += hot.failures("NaN row")
            if not torch.equal(R.bits(hot.view[keep]), R.bits(dest.view[keep])):
                fails.append("NaN / inf in one row of A changes other rows")
            if bool(torch.isfinite(hot.view[rr]).any()):
                fails.append("NaN / inf in a row of A does not reach the whole row of the output")
        if fails:
            bad.append((c["name"], fails))
    record("retrieval_forms_affine", double=double, bt=bt, shape=list(shape), worst_ratio=worst)
    assert not bad, bad


# ---- row_norm
@pytest.mark.parametrize("name", [c["name"] for c in R.ROWNORM_CASES])
def test_row_norm_against_fp64(lib, name):
    c = next(c for c in R.ROWNORM_CASES if c["name"] == name)
    ops = R.rownorm_operands(c, DEV)
    outs = []
    for _ in range(2):
        dest = R.Guarded((c["M"],), DEV)
        lib.check(lib.load().must3r_hip_row_norm(_p(ops["x"]), c["M"], c["C"], _p(dest.view), _stream()))
        torch.cuda.synchronize()
        outs.append(dest)
    r, fails = R.value_check(outs[0], *R.rownorm_ref(ops))
    row("row_norm", name, "ratio", r)
    assert fails == [] and torch.equal(outs[0].bits, outs[1].bits), fails


# ---- top-k
def run_topk(lib, feat, attn, k):
    Bn, N, Cc = feat.shape
    dests = R.topk_dests(Bn, k, Cc, DEV)
    lib.check(lib.load().must3r_hip_topk_gather(_p(feat), _p(attn), Bn, N, Cc, k, _p(dests["feat"].view), _p(dests["attn"].view), _p(dests["idx"].view), _stream()))
    torch.cuda.synchronize()
    return dests


@pytest.mark.parametrize("N", R.TOPK_N)
def test_topk_equals_the_stable_descending_sort(lib, N):
    """indices, keys and rows bit for bit, for every k, C, image count and key kind of the table -- ties, infinities and NaN keys (1, 3, N // 10 + 1, all)"""
    bad, n = [], 0
    for Bn in R.TOPK_IMAGES:
        feats = {Cc: R.topk_feat(Bn, N, Cc, DEV) for Cc in R.TOPK_C}
        for kind in R.TOPK_KEYS + R.TOPK_NAN_KEYS:
            attn = R.topk_keys(kind, Bn, N).to(DEV)
            ok = 0
            for Cc in R.TOPK_C:
                for k in R.topk_ks(N):
                    dests = run_topk(lib, feats[Cc], attn, k)
                    fails = R.topk_check(feats[Cc], attn, k, dests)
                    if k == N and Cc == 4:       # a second launch
                        again = run_topk(lib, feats[Cc], attn, k)
                        if not all(torch.equal(again[m].bits, dests[m].bits) for m in dests):
                            fails.append("a second launch gives other bits")
                    if fails:
                        bad.append((N, Bn, kind, Cc, k, fails))
                    else:
                        ok += 1
                    n += 1
            row("topk_gather", f"N{N}-images{Bn}-{kind}", f"exact cases of {len(R.TOPK_C) * len(R.topk_ks(N))}", ok)
    record("retrieval_forms_topk", N=N, cases=n, failed=len(bad))
    assert not bad, bad[:5]


# ---- weighted_spoc
@pytest.mark.parametrize("name", [c["name"] for c in R.SPOC_CASES])
def test_weighted_spoc_against_fp64(lib, name):
    c = next(c for c in R.SPOC_CASES if c["name"] == name)
    ops = R.spoc_operands(c, DEV)
    outs = []
    for _ in range(2):
        dest = R.Guarded((3, c["C"]), DEV)
        lib.check(lib.load().must3r_hip_weighted_spoc(_p(ops["feat"]), _p(ops["attn"]), 3, c["N"], c["C"], _p(dest.view), _stream()))
        torch.cuda.synchronize()
        outs.append(dest)
    r, fails = R.spoc_check(ops, outs[0])
    row("weighted_spoc", name, "ratio (ordinary, zero, tiny)", r)
    assert fails == [] and torch.equal(outs[0].bits, outs[1].bits), fails


# ---- l2_normalize
@pytest.mark.parametrize("in_place", [0, 1], ids=["copy", "in_place"])
@pytest.mark.parametrize("name", [c["name"] for c in R.L2_CASES])
def test_l2_normalize_against_fp64(lib, name, in_place):
    c = next(c for c in R.L2_CASES if c["name"] == name)
    ops = R.l2_operands(c, DEV)
    shape = (c["outer"], c["L"], c["inner"])
    outs = []
    for _ in range(2):
        dest = R.Guarded(shape, DEV)
        src = dest.fill(ops["x"]).view if in_place else ops["x"]
        lib.check(lib.load().must3r_hip_l2_normalize(_p(src), c["outer"], c["L"], c["inner"], _p(dest.view), _stream()))
        torch.cuda.synchronize()
        outs.append(dest)
    r, fails = R.l2_check(ops, outs[0])
    row("l2_normalize", name + ("-in_place" if in_place else "-copy"), "ratio", r)
    assert fails == [] and torch.equal(outs[0].bits, outs[1].bits), fails


# ---- layernorm_act_f32
@pytest.mark.parametrize("M", [1, 5, 70])
@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 320])
def test_layernorm_act_parity_per_row_kind(lib, Cc, M):
    bad, prows = [], []
    for c in R.LN_CASES:
        if (c["C"], c["M"]) != (Cc, M):
            continue
        ops = R.ln_operands(c, DEV)
        dest = R.Guarded((M, Cc), DEV)
        lib.check(lib.load().must3r_hip_layernorm_act_f32(_p(ops["x"]), _p(ops["w"]), _p(ops["b"]), R.LN_EPS, M, Cc, c["gelu"], _p(dest.view), _stream()))
        torch.cuda.synchronize()
        n0 = len(prows)
        fails = R.ln_check(ops, dest, prows)          # prints its rows
        for (tag, kind, m, e_gpu, e_ref, ratio) in prows[n0:]:
            _rows.append(("layernorm_act_f32", tag, f"ratio {kind} (e_gpu {e_gpu:.2f}, e_ref {e_ref:.2f})", f"{ratio:.4f}"))
        if fails:
            bad.append((c["name"], fails))
    assert not bad, bad


# ---- the Python layer
@pytest.mark.parametrize("nfeat,k", [(-0.5, 50), (-0.37, 37), (1000, 100), (100, 100), (0, 0), (-0.001, 0), (7.9, 7)])
def test_how_select_local_k_and_order(nfeat, k):
    """fractional nfeat (a share of N), nfeat > N, and nfeat that yields k = 0 (empty outputs, nothing launched)"""
    from must3r_amd.retrieval import how_select_local
    feat = R.topk_feat(2, 100, 12, DEV)
    attn = R.topk_keys("quant", 2, 100, seed=3).to(DEV)
    f, a, i = how_select_local(feat, attn, nfeat)
    row("how_select_local", f"nfeat {nfeat}", "k", int(i.shape[1]))
    assert f.shape == (2, k, 12) and a.shape == (2, k) and i.shape == (2, k) and i.dtype == torch.int64
    want = R.topk_expected(attn, k).to(DEV)
    assert torch.equal(i, want)
    if k:
        assert torch.equal(R.bits(a), R.bits(torch.gather(attn, 1, want))) and torch.equal(f, torch.gather(feat, 1, want[:, :, None].expand(-1, -1, 12)))


@pytest.mark.parametrize("dim", [-1, 1, 0])
def test_whitener_l2norm_dims(dim):
    """Whitener(l2norm=dim) at (2, 7, 20) tokens: the fp64 affine within its bound, and the normalisation of ITS fp32 result within (L/2 + 4) u"""
    from must3r_amd.retrieval import Whitener
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 7, 20), generator=g) * 3 + 5
    m = torch.randn((1, 20), generator=g, dtype=torch.float64) + 5
    p = torch.randn((20, 20), generator=g, dtype=torch.float64)
    plain, normed = Whitener(20).to(DEV), Whitener(20, l2norm=dim).to(DEV)
    for w in (plain, normed):
        w.load_state_dict({"m": m, "p": p})
    y = plain(x.to(DEV))
    c = dict(M=14, N=20, K=20, double=1, bt=0, opt="sub", kind="scaled", name="whitener")
    ops = dict(case=c, A=x.view(14, 20), sub=m.view(20), Bl=p, B=p, bias=None, resid=None, alias=False)
    ref, bound = R.affine_ref(ops)
    r_aff = R._ratio((y.cpu().double().view(14, 20) - ref).abs(), bound)
    z = normed(x.to(DEV))
    d = dim % 3
    shape3 = (math.prod(x.shape[:d]), x.shape[d], math.prod(x.shape[d + 1:]))
    zref, zbound = R.l2_ref(y.view(shape3))
    r_l2 = R._ratio((z.cpu().double().view(shape3) - zref).abs(), zbound)
    row("Whitener", f"l2norm={dim}", "ratio affine fp64", r_aff)
    row("Whitener", f"l2norm={dim}", "ratio l2 of its result", r_l2)
    assert z.shape == x.shape and z.dtype == x.dtype and r_aff <= 1.0 and r_l2 <= 1.0
    nrm = z.double().norm(dim=dim)
    assert bool(((nrm - 1).abs() < 1e-5).all())
