"""GPU (-m gpu): the grouped and per-scene argument forms in which the batched decoder launches its GEMMs, through must3r_hip_op_gemm_ex (ABI 17), against fp64 over the
operands the kernel multiplies (tests/gemm_forms.py: dispatch restated, case table, operands, reference, bounds, destinations, checks).  Per case, dtype and weight mode,
under the default options: the kernel the restated dispatch names ran; values against fp64; canaries in front of, behind and between the destinations; a second run gives
the same bits; a grouped launch with its problems and out_table permuted together gives every problem the same bits; projq stores T(v32 * out_scale) of its fp32 twin.  Then
the refusals of the entry point.  The measured errors go through test_ops_gpu.record and, as a table, to the file M3R_GEMM_FORMS_TABLE names (kept as
profiles/gemm_forms_errors.txt)."""
import ctypes as C
import math
import os
import time

import pytest
import torch

import gemm_forms as F
from test_ops_gpu import record   # the suite's one metrics log

pytestmark = pytest.mark.gpu
_rows = []   # (kind, weights, dt, kernel, case, ratio, abs error, emulation ratio, rtol, atol)
DEFAULTS = (("PERSIST", 0), ("GEMM256", 1), ("G256K", 1), ("G256P", 1), ("G256P_SPLIT", 1), ("SPARSE_256", 1), ("SPARSE_LO", 1), ("BK128", 1), ("LNFOLD256", 0),
            ("G256_GM", 4))   # csrc/misc.hip kOpts: what the restated dispatch assumes


@pytest.fixture(scope="module")
def lib():
    from must3r_amd import _lib
    t0 = time.time()
    for n, v in DEFAULTS:
        _lib.set_option(n, v)
    yield _lib
    for n, v in DEFAULTS:
        _lib.set_option(n, v)
    table = os.environ.get("M3R_GEMM_FORMS_TABLE")
    if _rows and table:
        with open(table, "w") as f:
            f.write("# tests/test_gemm_forms_gpu.py: worst max |out - fp64| / (atol + rtol |fp64|) per form, weights, dtype and picked kernel (gemm_last_kernel()) over the form's cases; `abs` = worst\n"
                    "# |out - fp64|; `emulated` = the same ratio of the fp32 emulation (tests/gemm_forms.py) on the same operands, its products taken by torch.matmul in fp32 ON THE GPU\n"
                    "# over all rows (noisier than the kernels on the fp32 split forms; on the CPU, where tests/test_gemm_forms_host.py holds it to half of every bound, the same\n"
                    "# emulation measures 0.37 - 0.38 over all rows of the largest embed and kv_all fp32 cases); bound = rtol / atol, the figures of test_ops_gpu.py\n"
                    "# (2u / 2u 16-bit stores, 2u / 4u with RoPE, 2u / 8u with a sparse low part; fp32 1e-5 / 1e-4 plain, 2e-6 / 8e-6 split or sparse; EPI_HEAD as fp32 plain): no form\n"
                    "# needed a wider one.  A ratio <= 1 passes.\n"
                    f"# wall time of the file: {time.time() - t0:.0f} s\n")
            f.write(f"{'form':<10}{'weights':<8}{'dt':<5}{'kernel':<20}{'cases':>6}{'ratio':>10}{'abs':>11}{'emulated':>10}{'rtol':>10}{'atol':>10}\n")
            agg = {}
            for (kind, w, dt, kern, name, err, ab, emu, rtol, atol) in _rows:
                a = agg.setdefault((kind, w, dt, kern), [0, 0.0, 0.0, 0.0, rtol, atol])
                a[0], a[1], a[2], a[3] = a[0] + 1, max(a[1], err), max(a[2], ab), max(a[3], emu)
            for (kind, w, dt, kern), a in agg.items():
                f.write(f"{kind:<10}{w:<8}{dt:<5}{kern:<20}{a[0]:>6}{a[1]:>10.3f}{a[2]:>11.2e}{a[3]:>10.3f}{a[4]:>10.2e}{a[5]:>10.2e}\n")


_tab = {}


def rope_table(lib):
    if "t" not in _tab:
        buf = (C.c_float * (F.NPOS * 32))()
        lib.check(lib.load().must3r_hip_rope_table(100.0, 1.0, F.NPOS, buf))
        _tab["t"] = torch.tensor(list(buf), device="cuda")
    return _tab["t"]


def pack_sparse(lib, ops):
    """the packed 2:4-sparse low part of the whole parameter (all L N rows): vals [K/64][L N][32] fp16, idx [K/64][L N / 32][64] dwords"""
    if "packed" not in ops:
        case = ops["case"]
        rows, K = case["L"] * case["N"], case["K"]
        vals = torch.empty((K // 64, rows, 32), device="cuda", dtype=torch.float16)
        idx = torch.empty((K // 64, rows // 32, 64), device="cuda", dtype=torch.int32)
        lib.check(lib.load().must3r_hip_op_sparse24_pack(ops["Wf"].data_ptr(), rows, K, vals.data_ptr(), idx.data_ptr(), torch.cuda.current_stream().cuda_stream))
        ops["packed"] = (vals, idx)
    return ops["packed"]


def launch(lib, ops, outs, order=None, expect_error=False, **override):
    """one must3r_hip_op_gemm_ex call on the current stream.  order: problem j of the launch is problem order[j] of `ops` (A's blocks and out_table permuted together).
    Returns the kernel it reports."""
    L = lib.load()
    case = ops["case"]
    P, M, N, K = case["P"], case["M"], case["N"], case["K"]
    d = lib.GemmOp()
    A = ops["A"] if order is None else ops["A"].view(P, M, K)[torch.tensor(order, device="cuda")].reshape(P * M, K).contiguous()
    d.dtype, d.epi = F.DT[ops["dt"]][0], case["epi"]
    d.A, d.W, d.bias = A.data_ptr(), ops["W"].data_ptr(), ops["bias"].data_ptr()
    d.M, d.N, d.K, d.lda, d.ldc = M, N, K, K, case["ldc"]
    d.wsplit = 0 if ops["weights"] == "plain" else 2
    if ops["weights"] == "sparse":
        vals, idx = pack_sparse(lib, ops)
        d.Wlo_sp, d.Widx_sp, d.wsp_rows = vals.data_ptr(), idx.data_ptr(), case["L"] * N
    if case["scale_cols"]:
        d.out_scale, d.scale_cols = F.OUT_SCALE, case["scale_cols"]
    table = None
    if case["kind"] in F.GROUPED:
        views = outs["views"] if order is None else [outs["views"][g] for g in order]
        table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device="cuda")
        d.batch, d.strideA, d.out_table = P, M * K, table.data_ptr()
        if case["kind"] == "kv_all":
            d.wdiv, d.strideW, d.strideB = case["S"], N * K * (1 if ops["weights"] == "plain" else 2), N
    else:
        d.out = outs["base"].data_ptr()
    if case["epi"] == F.EPI_QKV_ROPE:
        d.pos, d.rope_tab, d.rope_cols, d.rope_npos = ops["pos"].data_ptr(), rope_table(lib).data_ptr(), case["rope_cols"], F.NPOS
    if ops["bias2"] is not None:
        d.bias2, d.row_start2, d.row_period2 = ops["bias2"].data_ptr(), case["row_start2"], case["row_period2"]
    if case["epi"] == F.EPI_HEAD:
        d.ntok, d.gw, d.H, d.Wimg = case["gh"] * case["gw"], case["gw"], case["gh"] * 16, case["gw"] * 16
        d.head_views, d.head_scene_skip = case["hv"], case["skip"]
    for k, a in override.items():
        setattr(d, k, a)
    picked = C.c_char_p()
    d.picked = C.pointer(picked)
    rc = L.must3r_hip_op_gemm_ex(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del table, A
    if expect_error:
        return rc, L.must3r_hip_last_error().decode()
    lib.check(rc)
    return picked.value.decode() if picked.value else None


def run(lib, ops, order=None):
    outs = F.alloc_outputs(ops, "cuda")
    return outs, launch(lib, ops, outs, order)


def problem_order(case):
    """a permutation of the problems that keeps every problem in its weight group (kv_all: the scenes of layer l rotated by l + 1); None when there is none but the identity"""
    P, S = case["P"], case["S"]
    if case["kind"] == "kv_scene":
        pi = [(g * next(s for s in (3, 5, 7, 11, 1) if math.gcd(s, P) == 1) + 1) % P for g in range(P)]
    else:
        pi = [(g // S) * S + (g % S + g // S + 1) % S for g in range(P)]
    return pi if pi != list(range(P)) else None


@pytest.mark.parametrize("name,dt,weights", F.COMBOS, ids=[f"{n}-{dt}-{w}" for n, dt, w in F.COMBOS])
def test_form_against_fp64(lib, name, dt, weights):
    case = F.CASE[name]
    ops = F.make_operands(case, dt, weights, "cuda")
    outs, picked = run(lib, ops)
    assert picked == ops["kernel"], (picked, ops["kernel"])
    F.check_canaries(ops, outs)
    rep = F.value_report(ops, outs, emu=True)
    # a second launch
    again, _ = run(lib, ops)
    F.outputs_equal(outs, again)
    del again
    # the problems and their destinations permuted together: same kernel, same grid, and every problem the same bits
    order = problem_order(case) if case["kind"] in F.GROUPED else None
    if order is not None:
        perm, picked_p = run(lib, ops, order)
        assert picked_p == picked
        F.outputs_equal(outs, perm)
        del perm
    if case["kind"] == "projq":   # the fp32 twin of the launch: acc + bias, no scale
        twin = torch.full((F.LEAD + case["M"] + F.PAD, case["N"]), float("nan"), device="cuda")
        view = twin[F.LEAD:F.LEAD + case["M"]]
        launch(lib, dict(ops, case=dict(case, epi=F.EPI_F32, scale_cols=0)), dict(base=view))
        assert bool(torch.isnan(twin[:F.LEAD]).all()) and bool(torch.isnan(twin[F.LEAD + case["M"]:]).all()) and not bool(torch.isnan(view).any())
        outs["twin"] = [view]
        F.check_scale_bits(ops, outs)
    _rows.append((case["kind"], weights, dt, picked, name, rep["err"], rep["abs"], rep["emu"], rep["rtol"], rep["atol"]))
    record("gemm_form", case=name, dt=dt, weights=weights, kernel=picked, report=rep)
    print(name, dt, weights, picked, rep)
    F.assert_values(rep, (name, dt, weights, picked))
    del outs, ops
    torch.cuda.empty_cache()


REFUSALS = [   # (what, case, weights, override, a word of the message)
    ("batch > 1 with a null out_table", "kv_scene-r12-S2", "plain", dict(out_table=None), "out_table"),
    ("wdiv that does not divide batch", "kv_all-L3-S4-r12", "split", dict(wdiv=5), "wdiv"),
    ("row_period2 without bias2", "embed-r392-S5-s196-p392", "plain", dict(bias2=None), "bias2"),
    ("head_views on another epilogue", "kv_scene-r12-S2", "plain", dict(head_views=2), "EPI_HEAD"),
    ("head_scene_skip on another epilogue", "embed-r392-S5-s196-p392", "split", dict(head_scene_skip=8), "EPI_HEAD"),
    ("head_scene_skip % 4 != 0", "head-S5-V3-3x4-skip4", "plain", dict(head_scene_skip=6), "multiple of 4"),
    ("wsp_rows smaller than the rows the groups index", "kv_all-L4-S7-r12", "sparse", dict(wsp_rows=3 * 1536), "wsp_rows"),
    ("wsp_rows of one group", "kv_all-L4-S7-r12-f32", "sparse", dict(wsp_rows=1536), "wsp_rows"),
    ("one sparse operand alone", "kv_scene-r12-S28", "sparse", dict(Widx_sp=None), "Widx_sp"),
    ("scale_cols that is no multiple of 64", "projq-M12", "split", dict(scale_cols=100), "scale_cols"),
    ("out_scale on an fp32 epilogue", "embed-r392-S1-s196-p0", "plain", dict(out_scale=0.5, scale_cols=64), "out_scale"),
    ("bad dtype", "kv_scene-r12-S2", "plain", dict(dtype=2), "dtype"),
]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refusals_launch_nothing(lib, what):
    """What the kernels would silently misread returns an error that names it, and no output element is written; the same descriptor without the override is served."""
    _, name, weights, over, word = next(r for r in REFUSALS if r[0] == what)
    ops = F.make_operands(F.CASE[name], "fp16", weights, "cuda")
    outs = F.alloc_outputs(ops, "cuda")
    rc, msg = launch(lib, ops, outs, expect_error=True, **over)
    assert rc != 0 and "op_gemm_ex" in msg and word in msg, (rc, msg)
    assert F._clean(outs["buf"])
    assert launch(lib, ops, outs) == ops["kernel"]
    F.check_canaries(ops, outs)
    F.assert_values(F.value_report(ops, outs))
