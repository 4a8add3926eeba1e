"""GPU (-m gpu): every LayerNorm launch form the model uses, through must3r_hip_op_layernorm_ex (ABI 15), against fp64 evaluations of the same operands
(tests/ln_forms.py: case table, operands and row kinds, reference, restatement, bounds, buffers, checks).  Per case: the kernel the dispatch names ran; values
by row kind against fp64; the bit relations inside one launch; the same bits from the other kernel (LN_ROWS = 0), from a launch with all six outputs, from the
fp32 input of the same 16-bit rows, from per-group launches and from a second run; canaries around and between everything written.  Then the refusals of the
entry point and the fp16 saturation of raw16.  The measured errors go through test_ops_gpu.record and, as a table, to the file M3R_LN_FORMS_TABLE names (kept as profiles/layernorm_forms_errors.txt)."""
import ctypes as C
import os
import time

import pytest
import torch

import ln_forms as F
from test_ops_gpu import record   # the suite's one metrics log

pytestmark = pytest.mark.gpu
_rows = []   # (form, C, M, dt, kernel, kind, out, n, kernel error, restatement error, bound)


@pytest.fixture(scope="module")
def lib():
    from must3r_amd import _lib
    t0 = time.time()
    yield _lib
    _lib.set_option("LN_ROWS", 1)
    table = os.environ.get("M3R_LN_FORMS_TABLE")
    if _rows and table:
        with open(table, "w") as f:
            f.write("# tests/test_layernorm_forms_gpu.py: max |out - fp64| / (1 + |fp64|) per form, C, kernel and row kind (worst over the cases' M); `restated` = the fp32 two-pass restatement on the CPU on the\n"
                    "# same rows, bound = max(1e-5, 4 x restated) for out32, max(2u, B + u (1 + B)) for out16 (tests/ln_forms.py).  kernel = layernorm_last_kernel()\n"
                    f"# wall time of the file: {time.time() - t0:.0f} s\n")
            f.write(f"{'form':<15}{'C':>5} {'dt':<5}{'kernel':<10}{'kind':<7}{'out':<6}{'cases':>6}{'rows':>8}{'kernel err':>12}{'restated':>12}{'bound':>12}\n")
            agg = {}   # per form, C, dt, kernel, kind and output over the cases' M: worst errors, smallest bound
            for (form, Cc, M, dt, kern, kind, out, n, err, rst, bnd) in _rows:
                a = agg.setdefault((form, Cc, dt, kern, kind, out), [0, 0, 0.0, 0.0, float("inf")])
                a[0], a[1], a[2], a[3], a[4] = a[0] + 1, a[1] + n, max(a[2], err), max(a[3], rst or 0.0), min(a[4], bnd)
            for (form, Cc, dt, kern, kind, out), a in agg.items():
                f.write(f"{form:<15}{Cc:>5} {dt:<5}{kern:<10}{kind:<7}{out:<6}{a[0]:>6}{a[1]:>8}{a[2]:>12.3e}{a[3]:>12.3e}{a[4]:>12.3e}\n")


def launch(lib, ops, outs, expect_error=False, **override):
    """one must3r_hip_op_layernorm_ex call on the current stream with the outputs `outs` requests; returns the kernel it reports"""
    L = lib.load()
    v = outs["view"]
    d = lib.LnOp()
    d.dtype = F.DT[ops["dt"]][0]
    for n in ("x", "x16", "add", "w", "b"):
        setattr(d, n, ops[n].data_ptr() if ops[n] is not None else None)
    for n in outs["req"]:
        setattr(d, n, v[n].data_ptr())
    d.ld16 = outs["ld16"]
    d.M, d.C, d.eps, d.rows_per_group, d.add_groups = ops["M"], ops["C"], ops["eps"], ops["R"], ops["add_groups"]
    for k, a in override.items():
        setattr(d, k, a)
    picked = C.c_char_p()
    d.picked = C.pointer(picked)
    rc = L.must3r_hip_op_layernorm_ex(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if expect_error:
        return rc, L.must3r_hip_last_error().decode()
    lib.check(rc)
    return picked.value.decode() if picked.value else None


def run(lib, ops, form=None):
    outs = F.alloc_outputs(ops, "cuda", form)
    return outs, launch(lib, ops, outs)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", [c["name"] for c in F.CASES])
def test_form_against_fp64(lib, name, dt):
    case = F.CASE[name]
    M, Cc = case["M"], case["C"]
    ops = F.make_operands(case, dt, "cuda")
    reps = {}
    try:
        lib.set_option("LN_ROWS", 1)
        outs, picked = run(lib, ops)
        assert picked == F.kernel_name(M, Cc), picked
        F.check_canaries(ops, outs)
        F.check_bits(ops, outs)
        reps["form"] = F.value_report(ops, outs)
        # all six outputs of the same input: values at fp32 resolution for every form, and the form's outputs are the same bits
        full, picked_full = run(lib, ops, "full")
        assert picked_full == picked
        F.check_canaries(ops, full)
        F.check_bits(ops, full)
        reps["full"] = F.value_report(ops, full)
        F.outputs_equal(outs, full)
        # a second launch
        again, _ = run(lib, ops)
        F.check_canaries(ops, again)
        F.outputs_equal(outs, again)
        del again
        # the other kernel
        lib.set_option("LN_ROWS", 0)
        outs0, picked0 = run(lib, ops)
        full0, _ = run(lib, ops, "full")
        assert picked0 == "ln" and (picked0 != picked) == (M >= F.WALK_MIN), (picked0, picked)
        F.check_canaries(ops, outs0)
        F.check_canaries(ops, full0)
        F.outputs_equal(outs, outs0)
        F.outputs_equal(full, full0)
        del outs0, full0
        lib.set_option("LN_ROWS", 1)
        if ops["x16"] is not None:      # from_raw(x16) == plain16(float(x16))
            of, _ = run(lib, F.with_float_input(ops), "plain16")
            F.outputs_equal(outs, of, ["out16"])
            del of
        if ops["R"]:                    # grouped == the groups one by one (21504 / 5463 rows each: the one-row kernel against the walker)
            R = ops["R"]
            for gi in range(ops["G"]):
                gops = F.group_slice(ops, gi)
                og, pg = run(lib, gops, "full")
                assert pg == F.kernel_name(R, Cc)
                for n in F.ALL_OUTS:
                    if n == "copy32" and gops["add"] is None:
                        assert torch.equal(og["view"][n], gops["x"])
                    assert torch.equal(og["view"][n], full["view"][n][gi * R:(gi + 1) * R]), (gi, n)
                del og
    finally:
        lib.set_option("LN_ROWS", 1)
    for tag, rep in reps.items():
        for kn, r in (rep or {}).items():
            _rows.append((case["form"] + ("" if tag == "form" else "+all"), Cc, M, dt, picked, kn, r["out"], r["n"], r["err"], r["restated"], r["bound"]))
    record("layernorm_form", case=name, dt=dt, kernel=picked, reports=reps)
    print(name, dt, picked, reps)
    for tag, rep in reps.items():
        F.assert_values(rep, (name, dt, tag))
    del outs, full, ops
    torch.cuda.empty_cache()


REFUSALS = [
    ("both x and x16", lambda ops, o: dict(x16=ops["x"].data_ptr())),
    ("neither x nor x16", lambda ops, o: dict(x=None)),
    ("null w", lambda ops, o: dict(w=None)),
    ("null b", lambda ops, o: dict(b=None)),
    ("ld16 < C", lambda ops, o: dict(ld16=ops["C"] - 4)),
    ("ld16 not a multiple of 4", lambda ops, o: dict(ld16=3 * ops["C"] + 2)),
    ("add_groups < 0", lambda ops, o: dict(add_groups=-1)),
    ("rows_per_group < 0", lambda ops, o: dict(rows_per_group=-7)),
    ("C not a multiple of 4", lambda ops, o: dict(C=ops["C"] - 2)),
    ("bad dtype", lambda ops, o: dict(dtype=2)),
]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refusals_launch_nothing(lib, what):
    """Every combination the kernels cannot serve returns an error with a message, and no output element is written."""
    ops = F.make_operands(F._case("head", 40, 768), "fp16", "cuda")
    outs = F.alloc_outputs(ops, "cuda")
    over = dict(REFUSALS)[what](ops, outs)
    rc, msg = launch(lib, ops, outs, expect_error=True, **over)
    assert rc != 0 and "layernorm" in msg, (rc, msg)
    for n, t in outs["buf"].items():
        assert bool((t == F.CANARY16).all()) if t.dtype == torch.int16 else bool(torch.isnan(t).all()), n
    # the same descriptor without the override is served
    assert launch(lib, ops, outs) == "ln"
    F.check_canaries(ops, outs)


@pytest.mark.parametrize("M", [1000, F.WALK_MIN + 37])
def test_raw16_saturates_in_fp16_and_the_stored_rows_normalise(lib, M):
    """memory_mode 'raw' in the fp16 modes: a token beyond +-65504 is stored as +-65504 (common.hpp cvt4_sat, as every other 16-bit store of the residual
    stream), never as inf, in both kernels; the LayerNorm of the stored rows (x16) is finite and equals fp64 of those rows.  bf16 keeps its plain rounding."""
    case = F._case("mem_raw", M, 768)
    for dt in ("fp16", "bf16"):
        ops = F.make_operands(case, dt, "cuda")
        big = ops["kinds"] == F.BIG
        assert int(big.sum()) > 3
        for ln_rows in (1, 0):
            try:
                lib.set_option("LN_ROWS", ln_rows)
                outs, picked = run(lib, ops)
                assert picked == F.kernel_name(M, 768, ln_rows)
                raw = F.as16(outs["view"]["raw16"].contiguous(), dt)
                got = raw[big].float()
                print(dt, picked, "raw16 of +-1e5:", got[0, 0].item(), got[0, -1].item(), "finite:", bool(torch.isfinite(raw.float()).all()))
                assert torch.isfinite(raw.float()).all()
                want, edge = (65504.0, 65504.0) if dt == "fp16" else (float(torch.tensor(1e5).bfloat16()), float(torch.tensor(65504.0).bfloat16()))
                assert (got[:, 0] == want).all() and (got[:, -1] == -want).all() and (got[:, 2] == -edge).all() and (got[:, -3] == edge).all()
                F.check_bits(ops, outs)
                F.check_canaries(ops, outs)
                # the stored rows through kv_source's LayerNorm
                s_case = F._case("from_raw", M, 768)
                sops = dict(F.make_operands(s_case, dt, "cuda"), x16=raw, x=None)
                so, _ = run(lib, sops)
                y = F.as16(so["view"]["out16"].contiguous(), dt).float()
                assert torch.isfinite(y).all(), "LayerNorm of the stored rows is not finite"
                F.assert_values(F.value_report(sops, so), (dt, picked, "from_raw of the stored rows"))
            finally:
                lib.set_option("LN_ROWS", 1)


@pytest.mark.parametrize("form,M,Cc", [("add_copy", 1000, 768), ("add_copy", 5, 200), ("add_copy", F.WALK_MIN + 37, 768), ("grouped", 35, 768)])
def test_mean_out_is_the_row_mean_and_changes_nothing_else(lib, form, M, Cc):
    """mean_out (ABI 18; the first shift of the LN fold: block 0's norm1 of a one-view update leaves it): row r gets the mean of x + add the statistics used (always by the one-row
    kernel, also where the launch without it walks rows); nothing in front of or behind the M entries is written; every other output keeps its bits.  Bound: a lane adds its <= 16 values in order, the wave adds
    the 64 partial sums in 6 pairwise steps, one division: (15 + 6 + 1) 2^-24 mean |x + add| + 2^-24 |mean|."""
    case = F._case(form, M, Cc, R=7, add_groups=4) if form == "grouped" else F._case(form, M, Cc)
    ops = F.make_operands(case, "fp16", "cuda")
    rows = torch.arange(M, device="cuda")
    xin, add, _, _ = F.resolve(ops, rows)
    s = xin.double() if add is None else (xin.float() + add.float()).double()      # the kernel adds in fp32 first
    want = s.mean(1)
    tol = 22 * 2.0 ** -24 * s.abs().mean(1) + 2.0 ** -24 * want.abs() + 1e-30
    for ln_rows in (1, 0):
        try:
            lib.set_option("LN_ROWS", ln_rows)
            base, picked = run(lib, ops)
            outs = F.alloc_outputs(ops, "cuda")
            mean = torch.full((2 + M + 3,), float("nan"), device="cuda")
            assert picked == F.kernel_name(M, Cc, ln_rows) and launch(lib, ops, outs, mean_out=mean[2:].data_ptr()) == "ln"   # the one-row kernel carries it
        finally:
            lib.set_option("LN_ROWS", 1)
        assert bool(torch.isnan(mean[:2]).all()) and bool(torch.isnan(mean[2 + M:]).all()), "mean_out written outside its M entries"
        got = mean[2:2 + M].double()
        assert bool(torch.isfinite(got).all()), "mean_out not written"
        r = float(((got - want).abs() / tol).max())
        print(form, M, Cc, picked, "mean_out against fp64, ratio of the bound:", r)
        assert r <= 1.0, (picked, r)
        F.check_canaries(ops, outs)
        F.outputs_equal(base, outs)
