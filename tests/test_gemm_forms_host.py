"""CPU: the checks of tests/test_gemm_forms_gpu.py discriminate.  The same operands, reference, bounds and check functions (tests/gemm_forms.py).  The clean fp32
emulation of what the kernels write stays within HALF of every case's bound -- the reference and the bounds leave the kernels room --, and each plausible defect of a
grouped or per-scene launch (wrong weight group, unstrided bias, sparse rows of group 0, the period or the start of the second bias, the scaled columns, the scale applied
to the rounded value, the scene offset of the head, a row past a ragged problem, exchanged destinations) fails at least one case.  A defect that slips through is a case to
add or a check to sharpen."""
import pytest
import torch

import gemm_forms as F

FAMILIES = {   # the kernels the table must reach (csrc/gemm.hip launch_epi under the default options), by weights: (family, tile width or None)
    "plain": [("g64p", None), ("g64", None), ("g48*", None), ("g128", None), ("g256p", 256), ("g256k", None)],
    "split": [("g64p", None), ("g64", None), ("g48*", None), ("g96", None), ("g128", 64), ("g256p", 128), ("g256", 192), ("g256", 256)],
    "sparse": [("g256ps", 128), ("g256s", 256)],
}


def test_case_table_reaches_every_family_and_form():
    hit = {w: set() for w in FAMILIES}
    for name, dt, w in F.COMBOS:
        fam, epi, ws, bn = F.kernel_of(F.CASE[name], w).split("/")
        hit[w] |= {(fam, None), (fam, int(bn[1:])), ("g48*" if fam.startswith("g48") else fam, None)}
    for w, want in FAMILIES.items():
        assert not [f for f in want if f not in hit[w]], (w, [f for f in want if f not in hit[w]])
    assert any(F.kernel_of(c, "plain").startswith("g256k/e2") for c in F.CASES)                     # the RoPE epilogue on the chip-filling plain tiles
    assert any(F.kernel_of(c, "plain").startswith("g256p/e5") for c in F.CASES if c["kind"] == "head")
    for c in F.CASES:
        if c["kind"] == "kv_all":
            assert c["L"] != c["S"] and c["P"] == c["L"] * c["S"]
        if c["kind"] in F.GROUPED:   # the destinations are not in problem order
            assert sorted(F.slot_of(c, g) for g in range(c["P"])) == list(range(c["P"])) and [F.slot_of(c, g) for g in range(c["P"])] != list(range(c["P"]))
    # sparse kernels with weight groups: rows of the packed low part beyond group 0
    assert {F.kernel_of(c, "sparse").split("/")[0] for c in F.CASES if c["kind"] == "kv_all"} >= {"g256ps", "g256s"}
    assert any(c["row_period2"] and c["M"] // c["row_period2"] * c["row_period2"] == c["M"] and c["row_period2"] % 256 for c in F.CASES)   # period boundaries inside tiles


@pytest.mark.parametrize("name", [c["name"] for c in F.CASES])
def test_clean_emulation_stays_within_half_of_every_bound(name):
    """every case, dtype and weight mode; the large problems on their first and last rows and on both sides of every scene boundary and second-bias start (a row's
    value does not depend on the others)"""
    case = F.CASE[name]
    worst = {}
    for dt in ("bf16", "fp16"):
        for w in F.weight_modes(case, dt):
            ops = F.make_operands(case, dt, w, "cpu")
            rtol, atol = F.bound(case, dt, ops["kernel"])
            rows = F.all_rows(ops) if case["M"] <= 64 else F.boundary_rows(case)
            probs = range(case["P"]) if case["P"] <= 8 else sorted({0, 1, case["S"] - 1, case["S"] % case["P"], case["P"] // 2, case["P"] - 1})
            e = max(F.ratio(F.emulated(ops, g, rows).double(), F.reference(ops, g, rows), rtol, atol) for g in probs)
            worst[(dt, w)] = round(e, 3)
            assert e <= 0.5, (name, dt, w, ops["kernel"], e)
    print(name, worst)


SMALL = ["kv_scene-r12-S2", "kv_all-L3-S4-r12", "kv_all-L3-S4-r12-f32", "kv_all-L4-S7-r12", "kv_all-L4-S7-r12-f32", "embed-r392-S1-s196-p0", "embed-r392-S5-s196-p392",
         "projq-M12", "projq-M600", "dec_qkv-M12", "head-S5-V3-3x4-contig", "head-S5-V3-3x4-views0", "head-S5-V3-3x4-skip4", "head-S5-V3-3x4-skip448"]


def _run(name, dt, w, **defect):
    ops = F.make_operands(F.CASE[name], dt, w, "cpu")
    outs = F.alloc_outputs(ops, "cpu")
    F.emulate(ops, outs, **defect)
    return ops, outs


def _failures(ops, outs):
    out = []
    for fn in (F.check_canaries, lambda o, u: F.assert_values(F.value_report(o, u)), F.check_scale_bits):
        try:
            fn(ops, outs)
        except AssertionError as e:
            out.append(str(e)[:100])
    return out


def _combos(names):
    return [(n, dt, w) for n in names for dt in ("bf16", "fp16") for w in F.weight_modes(F.CASE[n], dt)]


@pytest.mark.parametrize("name", SMALL)
def test_clean_emulation_passes_every_check(name):
    for n, dt, w in _combos([name]):
        ops, outs = _run(n, dt, w)
        assert _failures(ops, outs) == [], (n, dt, w)
        assert F.value_report(ops, outs)["err"] <= 0.5


def _rejected(names, only=None, **defect):
    for n, dt, w in _combos(names):
        if only and not only(n, dt, w):
            continue
        ops, outs = _run(n, dt, w, **defect)
        assert _failures(ops, outs), (n, dt, w, defect)


KV_ALL = ["kv_all-L3-S4-r12", "kv_all-L3-S4-r12-f32", "kv_all-L4-S7-r12", "kv_all-L4-S7-r12-f32"]


def test_wrong_weight_groups_are_rejected():
    _rejected(KV_ALL, w_mod_L=True)            # g % L for g / wdiv
    _rejected(KV_ALL, bias_unstrided=True)
    # the sparse rows of group 0 under every group: a difference of two low parts, ~2^-12 of the product -- below the rounding of a 16-bit store, so the fp32 twin sees it
    sparse = lambda n, dt, w: w == "sparse"   # noqa: E731
    assert F.kernel_of(F.CASE["kv_all-L4-S7-r12-f32"], "sparse") == "g256ps/e4/w3/n128"
    _rejected(["kv_all-L4-S7-r12-f32"], only=sparse, sp_row0_zero=True)


def test_wrong_second_bias_rows_are_rejected():
    _rejected(["embed-r392-S5-s196-p392"], no_period=True)
    for off in (1, -1):
        _rejected(["embed-r392-S5-s196-p392", "embed-r392-S1-s196-p0"], start2_off=off)


def test_wrong_scaling_is_rejected():
    _rejected(["dec_qkv-M12"], scale_cols_off=64)
    _rejected(["dec_qkv-M12", "projq-M12", "projq-M600"], scale_cols_off=-64)
    for n, dt, w in _combos(["projq-M12", "projq-M600"]):     # the scale on the rounded value: inside 2u, the bits tell
        ops, outs = _run(n, dt, w, scale_after_round=True)
        with pytest.raises(AssertionError, match="out_scale"):
            F.check_scale_bits(ops, outs)


def test_wrong_head_scene_offsets_are_rejected():
    _rejected(["head-S5-V3-3x4-skip4", "head-S5-V3-3x4-skip448"], skip_dropped=True)
    _rejected(["head-S5-V3-3x4-skip4", "head-S5-V3-3x4-skip448"], scene_mod=True)
    for n in ("head-S5-V3-3x4-skip4", "head-S5-V3-3x4-skip448"):
        ops, outs = _run(n, "fp16", "plain", skip_dropped=True)
        with pytest.raises(AssertionError, match="canaries"):
            F.check_canaries(ops, outs)


def test_wrong_destinations_are_rejected():
    for n, dt, w in _combos(["kv_scene-r12-S2"] + KV_ALL):
        ops, outs = _run(n, dt, w, extra_row=True)         # a ragged problem writing one row past its M
        with pytest.raises(AssertionError, match="canaries"):
            F.check_canaries(ops, outs)
    _rejected(["kv_scene-r12-S2"] + KV_ALL, swap_dest=True)
