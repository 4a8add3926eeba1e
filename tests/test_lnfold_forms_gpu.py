"""GPU (-m gpu): every GEMM launch form of the LN fold of a one-view update, through must3r_hip_op_gemm_lnfold_ex (ABI 18), against fp64 (tests/lnfold_forms.py: dispatch
restated, case tables, row kinds, operands, reference, bounds, destinations, checks, chain).  Producers (embed, proj, fc2 with split and plain weights, the last fc2): the
kernel the restated dispatch names ran; out against fp64; copy32 == out and x16 == fp16_sat(out - shift) bit for bit; the fragment sums inside their a-priori bound;
canaries around every destination; ln_shift untouched.  Consumers (qkv with and without ln_shift_init, projq, fc1 with split and plain weights): the kernel; out inside the
conditioning-dependent bound per row kind; ln_shift == (init ? 0 : old) + mu, once; canaries; a second run gives the same bits; projq with M3R_BK128 = 0 runs g48 and gives
the same bits.  Then three blocks chained through the entry point in both weight modes, and the refusals.  The measured ratios go through test_ops_gpu.record and, as a
table, to the file M3R_LNFOLD_FORMS_TABLE names (kept as profiles/lnfold_forms_errors.txt)."""
import ctypes as C
import os
import time

import pytest
import torch

import gemm_forms as G
import lnfold_forms as F
from test_gemm_forms_gpu import DEFAULTS, rope_table
from test_ops_gpu import record

pytestmark = pytest.mark.gpu
_rows = []   # (role, form, weights, kernel, case, gpu report, emulation report)


@pytest.fixture(scope="module")
def lib():
    from must3r_amd import _lib
    t0 = time.time()
    for n, v in DEFAULTS:
        _lib.set_option(n, v)
    yield _lib
    for n, v in DEFAULTS:
        _lib.set_option(n, v)
    table = os.environ.get("M3R_LNFOLD_FORMS_TABLE")
    if _rows and table:
        with open(table, "w") as f:
            f.write("# tests/test_lnfold_forms_gpu.py: the LN-fold GEMM forms of a one-view update against fp64, worst ratio error / bound over the form's cases (M = 12, 196, 700, 768, 1024);\n"
                    "# `emulated` = the same ratio of the fp32 emulation (tests/lnfold_forms.py) on the same operands and device.  A ratio <= 1 passes; the host test holds the\n"
                    "# emulation on the CPU to 0.5.\n"
                    f"# consumer bound: |out - ref| <= C_R u |ref| + g(C_A u kappa ||W'_n|| + C_V 2^-24 kappa^2 |pre - c_n|), C_R = {F.C_R:g}, C_A = {F.C_A:g}, C_V = {F.C_V:g}; rows with\n"
                    f"# kappa > {F.KAPPA_CONTRACT:g}: row-wise against C_V_OUT = {F.C_V_OUT:g} x the kappa^2 term (`kappa>300`); W_SCALE = {F.W_SCALE:g}\n"
                    "# producer bounds: out 1e-5 / 1e-4 (plain), 2e-6 / 8e-6 (split); fragment sums (n - 1) 2^-24 sum |term|\n"
                    f"# wall time of the file: {time.time() - t0:.0f} s\n")
            agg = {}
            for role, form, w, kern, name, rep, emu in _rows:
                a = agg.setdefault((role, form, w, kern), {})
                cols = dict(rep.get("kinds", {}))
                cols.update({k: rep[k] for k in ("err", "s1", "s2", "shift", "out_of_contract") if k in rep})
                ecols = dict(emu.get("kinds", {}))
                ecols.update({k: emu[k] for k in ("err", "s1", "s2", "shift", "out_of_contract") if k in emu})
                for k in cols:
                    g0, e0 = a.get(k, (0.0, 0.0))
                    a[k] = (max(g0, cols[k]), max(e0, ecols.get(k, 0.0)))
            f.write(f"{'role':<10}{'form':<10}{'weights':<8}{'kernel':<20}{'quantity':<18}{'gpu':>8}{'emulated':>10}\n")
            for (role, form, w, kern), a in agg.items():
                for k, (gv, ev) in a.items():
                    q = {"err": "out (all kinds)", "s1": "sum y", "s2": "sum y^2", "shift": "ln_shift", "out_of_contract": "kappa>300"}.get(k, k)
                    f.write(f"{role:<10}{form:<10}{w:<8}{kern:<20}{q:<18}{gv:>8.3f}{ev:>10.3f}\n")


def _p(t):
    return t.data_ptr() if t is not None else None


def launch(lib, op, expect_error=False, **override):
    """one must3r_hip_op_gemm_lnfold_ex call on the current stream from a launch of tests/lnfold_forms.py; returns the kernel it reports"""
    L = lib.load()
    d = lib.LnFoldOp()
    d.dtype, d.epi = 1, op["epi"]
    d.A, d.W, d.bias, d.out = _p(op["A"]), _p(op["W"]), _p(op["bias"]), _p(op["out"])
    d.M, d.N, d.K, d.lda, d.ldc, d.wsplit = op["M"], op["N"], op["K"], op["K"], op["N"], op["wsplit"]
    d.ln_shift = _p(op["shift"])
    if op["role"] == "producer":
        d.x16_out, d.copy32_out, d.stats_out = _p(op["x16"]), _p(op["copy"]), _p(op["stats"])
        d.bias2, d.row_start2 = _p(op["bias2"]), op["row_start2"]
    else:
        d.ln_stats, d.ln_s, d.ln_eps, d.ln_shift_init = _p(op["stats"]), _p(op["s_n"]), op["eps"], op["init"]
        if op["epi"] == F.EPI_QKV_ROPE:
            d.pos, d.rope_tab, d.rope_cols, d.rope_npos = _p(op["pos"]), _p(rope_table(lib)), op["rope_cols"], G.NPOS
        if op["scale_cols"]:
            d.out_scale, d.scale_cols = G.OUT_SCALE, op["scale_cols"]
    for k, a in override.items():
        setattr(d, k, a)
    picked = C.c_char_p()
    d.picked = C.pointer(picked)
    rc = L.must3r_hip_op_gemm_lnfold_ex(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect_error:
        return rc, L.must3r_hip_last_error().decode()
    lib.check(rc)
    return picked.value.decode() if picked.value else None


def _same_bits(a, b):
    for k in a:
        x, y = a[k], b[k]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), f"{k}: bits differ"


@pytest.mark.parametrize("name", [c["name"] for c in F.PCASES])
def test_producer_against_fp64(lib, name):
    case = F.CASE[name]
    ops = F.make_producer(case, "cuda")
    outs = F.alloc_producer(ops, "cuda")
    picked = launch(lib, F.producer_op(ops, outs))
    assert picked == ops["kernel"], (picked, ops["kernel"])
    emu = F.alloc_producer(ops, "cuda")
    F.emulate(F.producer_op(ops, emu))
    erep = F.check_producer(ops, emu, strict=False)   # (torch.matmul in fp32 on the GPU: noisier than the kernels at K = 3072; the host test holds it on the CPU)
    again = F.alloc_producer(ops, "cuda")
    launch(lib, F.producer_op(ops, again))
    _same_bits(outs, again)
    try:
        rep = F.check_producer(ops, outs)
    finally:
        print(name, picked, "emulated", erep)
    print(name, picked, rep)
    _rows.append(("producer", case["form"], case["weights"], picked, name, rep, erep))
    record("lnfold_form", case=name, kernel=picked, report=rep)


@pytest.mark.parametrize("name", [c["name"] for c in F.CCASES])
def test_consumer_against_fp64(lib, name):
    case = F.CASE[name]
    ops = F.make_consumer(case, "cuda")
    outs = F.alloc_consumer(ops, "cuda")
    picked = launch(lib, F.consumer_op(ops, outs))
    assert picked == ops["kernel"], (picked, ops["kernel"])
    R = F.consumer_reference(ops)
    emu = F.alloc_consumer(ops, "cuda")
    F.emulate(F.consumer_op(ops, emu))
    erep = F.check_consumer(ops, emu, R, strict=False)
    again = F.alloc_consumer(ops, "cuda")
    launch(lib, F.consumer_op(ops, again))
    _same_bits(outs, again)
    if case["form"] == "projq":   # 64-deep K-tiles: another kernel symbol, the same bits
        try:
            lib.set_option("BK128", 0)
            k64 = F.alloc_consumer(ops, "cuda")
            assert launch(lib, F.consumer_op(ops, k64)) == F.consumer_kernel(case["epi"], case["weights"], bk128=0)
        finally:
            lib.set_option("BK128", 1)
        _same_bits(outs, k64)
    got = outs["out"][F.LEAD:F.LEAD + case["M"]].contiguous().view(torch.float16).double()
    q = (got - R["ref"]).abs() / R["bound"]
    kinds = torch.arange(case["M"], device="cuda") % F.NK
    print(name, picked, "every kind, contract or not:", {F.KINDS[i]: round(float(q[kinds == i].max()), 3) for i in range(min(F.NK, case["M"]))}, "emulated", erep)
    rep = F.check_consumer(ops, outs, R)
    print(name, picked, rep)
    _rows.append(("consumer", case["form"] + ("-first" if case["init"] else ""), case["weights"], picked, name, rep, erep))
    record("lnfold_form", case=name, kernel=picked, report=rep)


@pytest.mark.parametrize("precision", ["fp16w2", "fp16wa"])
def test_chain_of_three_blocks(lib, precision):
    """embed -> 3 x (qkv, proj, projq, proj, fc1, fc2) through the entry point alone, as decode_impl launches them in a folding call"""
    ch = F.make_chain(precision, "cuda")
    kernels = []
    reps = F.run_chain(ch, lambda op: kernels.append(launch(lib, op)), "cuda")
    print(precision, kernels)
    for r in reps:
        print(precision, r)
    record("lnfold_chain", precision=precision, reports=reps)
    mlp = 1 if precision == "fp16wa" else 2
    assert kernels[0] == "g64p/e4/w1/n64" and kernels[5] == ("g64/e1/w1/n64" if mlp == 1 else "g96/e1/w2/n96") and kernels[6] == f"g64p/e3/w{mlp}/n64", kernels
    assert len(reps) == 3 * F.CHAIN_L
    for r in reps:
        assert r["kappa"] <= 2.0, ("a condition on the inputs: the rows of the chain are benign", r)
        assert r["shift"] <= 1.0 and r["err"] <= 1.0, r


REFUSALS = [   # (what, case, override, a word of the message)
    ("bf16 operands", "proj-split-M12", dict(dtype=0), "dtype"),
    ("wsplit = 1", "proj-split-M12", dict(wsplit=1), "wsplit"),
    ("a consumer with producer outputs", "projq-split-M12", dict(x16_out=1), "exclude"),
    ("a consumer without ln_s", "projq-split-M12", dict(ln_s=None), "ln_s"),
    ("a consumer without ln_shift", "fc1-plain-M12", dict(ln_shift=None), "ln_shift"),
    ("a consumer with K = 1024", "qkv-split-M12", dict(K=1024, lda=1024), "K = 768"),
    ("stats_out without x16_out", "fc2-plain-M12", dict(x16_out=None), "x16_out"),
    ("producer outputs with ldc != N", "fc2-split-M12", dict(ldc=1024), "ldc"),
    ("bias2 on the residual epilogue", "proj-split-M12", dict(bias2=1), "bias2"),
    ("scale_cols that is no multiple of 64", "projq-split-M12", dict(scale_cols=100), "scale_cols"),
]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refusals_launch_nothing(lib, what):
    """What the kernels would misread returns an error that names it and writes nothing; the same descriptor without the override is served."""
    _, name, over, word = next(r for r in REFUSALS if r[0] == what)
    case = F.CASE[name]
    prod = case["role"] == "producer"
    ops = (F.make_producer if prod else F.make_consumer)(case, "cuda")
    outs = (F.alloc_producer if prod else F.alloc_consumer)(ops, "cuda")
    before = {k: v.clone() for k, v in outs.items()}
    op = (F.producer_op if prod else F.consumer_op)(ops, outs)
    over = {k: (_p(ops["W"]) if v == 1 and k in ("x16_out", "bias2") else v) for k, v in over.items()}   # (any non-null pointer: nothing is launched)
    rc, msg = launch(lib, op, expect_error=True, **over)
    assert rc != 0 and "op_gemm_lnfold_ex" in msg and word in msg, (rc, msg)
    _same_bits(before, outs)
    assert launch(lib, op) == ops["kernel"]
    (F.check_producer if prod else F.check_consumer)(ops, outs)
