"""CPU: the checks of tests/test_layernorm_forms_gpu.py discriminate.  The same operands, reference, bounds and check functions (tests/ln_forms.py); what a
plausibly wrong LayerNorm kernel would write is emulated in fp64 and must be rejected -- where the issue is a value, by at least 4x the bound on the row kind
that is there to see it.  A defect that slips through is a case to add or a bound to tighten.  The fp32 two-pass restatement the stress bounds are taken
from must itself pass every check, the benign 1e-5 included."""
import pytest
import torch

import ln_forms as F

MARGIN = 4.0
HOST_CASES = ([F._case(f, 1000, 768) for f in F.FORMS if f != "grouped"] +
              [F._case("split", 1000, C) for C in (1024, 128, 200, 260, 772)] + [F._case("head", 5, 200), F._case("head_wide", 37, 772)] +
              [F._case("grouped", 35, 200, R=7, add_groups=a) for a in (0, 4, 5)] +
              [F._case("split", 65536 + 37, 128), F._case("grouped", 12 * 5463, 128, R=5463, add_groups=11)])


def _run(case, dt, form=None, prec=torch.float64, **defect):
    ops = F.make_operands(case, dt, "cpu")
    outs = F.alloc_outputs(ops, "cpu", form)
    F.emulate(ops, outs, prec, **defect)
    return ops, outs


def _failures(ops, outs):
    out = []
    for fn in (F.check_canaries, F.check_bits, lambda o, u: F.assert_values(F.value_report(o, u))):
        try:
            fn(ops, outs)
        except AssertionError as e:
            out.append(str(e)[:120])
    return out


def _misses(case, dt, kind, form="full", **defect):
    """the defect's error on the rows of `kind` (None: of the kind that sees it best) is at least MARGIN x their bound"""
    ops, outs = _run(case, dt, form, **defect)
    rep = F.value_report(ops, outs)
    r = rep[kind] if kind else max(rep.values(), key=lambda q: q["err"] / q["bound"])
    assert r["err"] > MARGIN * r["bound"], (case["name"], dt, kind, defect, r)
    return r["err"] / r["bound"]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", [c["name"] for c in HOST_CASES])
def test_fp32_restatement_passes_every_check(name, dt):
    """What the bounds are taken from is inside them: the fp32 two-pass evaluation passes the value bounds of every row kind (benign: 1e-5, 16-bit: 2u), the bit
    relations and the canaries, through the form's own outputs and through all six."""
    case = next(c for c in HOST_CASES if c["name"] == name)
    for form in (None, "full"):
        ops, outs = _run(case, dt, form, prec=torch.float32)
        assert _failures(ops, outs) == []
        rep = F.value_report(ops, outs)
        if form == "full":
            assert set(rep) >= {"benign", "mean40", "spike", "lowvar", "const"} or case["M"] < 5, rep.keys()
    # and an exact (fp64) evaluation, rounded once, is inside them too
    ops, outs = _run(case, dt, "full")
    assert _failures(ops, outs) == []


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wrong_statistics_miss_the_bounds(dt):
    seen = {}
    plain, fb = F._case("split", 1000, 768), F._case("feedback", 1000, 768)
    # eps: the blocks' 1e-6 against feedback_norm's 1e-5, either way, through the fp32 output and through the 16-bit output alone
    seen["eps_1e-5_for_1e-6"] = _misses(plain, dt, "lowvar", eps=1e-5)
    seen["eps_1e-6_for_1e-5"] = _misses(fb, dt, "lowvar", eps=1e-6)
    seen["eps_1e-6_for_1e-5/out16"] = _misses(fb, dt, "lowvar", form=None, eps=1e-6)
    seen["eps_1e-5_for_1e-6/out16"] = _misses(F._case("plain16", 1000, 768), dt, "lowvar", form=None, eps=1e-5)
    # one-pass variance, evaluated in fp32
    seen["onepass_fp32"] = _misses(plain, dt, "mean40", prec=torch.float32, onepass=True)
    for C in (768, 1024, 200):
        seen[f"div_C-1/{C}"] = _misses(F._case("split", 1000, C), dt, "benign", div=C - 1)
    for C, NV in ((200, 3), (772, 4)):
        seen[f"div_padded/{C}"] = _misses(F._case("split", 1000, C), dt, "benign", div=256 * NV)
    for C in (768, 772, 200):
        seen[f"last_chunk/{C}"] = _misses(F._case("split", 1000, C), dt, "benign", drop_last_chunk=True)
        _misses(F._case("split", 1000, C), dt, "spike", drop_last_chunk=True)
    print(dt, {k: round(v, 1) for k, v in seen.items()})


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wrong_groups_miss_the_bounds(dt):
    small = [F._case("grouped", 35, 200, R=7, add_groups=a) for a in (0, 4, 5)]
    big = F._case("grouped", 12 * 5463, 128, R=5463, add_groups=11)
    for shift in (1, -1):
        for c in small + [big]:
            _misses(c, dt, None, resolve_kw=dict(group_shift=shift))     # one row per group, whatever its kind
            assert _failures(*_run(c, dt, None, resolve_kw=dict(group_shift=shift)))          # through the 16-bit output of the form itself
    for c in (small[1], big):      # add_groups = G - 1
        _misses(c, dt, "benign", resolve_kw=dict(add_groups=c["G"]))
        _misses(c, dt, "benign", resolve_kw=dict(add_groups=c["G"] - 2))
        assert _failures(*_run(c, dt, None, resolve_kw=dict(add_groups=c["G"])))
    _misses(small[0], dt, "benign", resolve_kw=dict(add_groups=1))       # add_groups = 0: nothing is added
    for c in (small[1], small[2], big):
        _misses(c, dt, "benign", resolve_kw=dict(add_wrong_row=True))
        # copy32 pins the row of add bit for bit
        ops, outs = _run(c, dt, "full", resolve_kw=dict(add_wrong_row=True))
        with pytest.raises(AssertionError, match="copy32"):
            F.check_bits(ops, outs)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wrong_walks_are_rejected(dt):
    """The row walker's own state: a stale prefetch (row r shows row r - 8192) and a last, ragged sweep that is skipped."""
    c = F._case("split", 65536 + 37, 128)
    stale = lambda r: torch.where(r >= F.NWALK, r - F.NWALK, r)   # noqa: E731
    _misses(c, dt, "benign", rows_from=stale)
    assert _failures(*_run(c, dt, None, rows_from=stale))
    g = F._case("grouped", 12 * 5463, 128, R=5463, add_groups=11)
    _misses(g, dt, "benign", rows_from=stale)
    ops, outs = _run(c, dt, None, skip_rows_from=(c["M"] // F.NWALK) * F.NWALK)
    with pytest.raises(AssertionError, match="not written"):
        F.check_canaries(ops, outs)
    with pytest.raises(AssertionError):
        F.assert_values(F.value_report(ops, outs))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wrong_outputs_break_the_bit_relations(dt):
    head = F._case("head", 1000, 768)
    ops, outs = _run(head, dt, None, lo_from_y=True)
    with pytest.raises(AssertionError, match="out16_lo"):
        F.check_bits(ops, outs)
    for c in (head, F._case("head_wide", 37, 772)):
        ops, outs = _run(c, dt, None, dup_stride_c=True)
        with pytest.raises(AssertionError, match="out16"):      # the misplaced copy runs over the other column blocks too
            F.check_bits(ops, outs)
        with pytest.raises(AssertionError):
            F.check_canaries(ops, outs)
    ops, outs = _run(F._case("mem_raw", 1000, 768), dt, None, raw_after_mean=True)
    with pytest.raises(AssertionError, match="raw16"):
        F.check_bits(ops, outs)


def test_raw16_saturates_in_fp16_only():
    """The rule the kernels are held to: fp16 stores +-1e5 as +-65504, bf16 keeps its rounding; an unsaturated fp16 store (inf) is rejected."""
    c = F._case("mem_raw", 1000, 768)
    for dt in ("bf16", "fp16"):
        ops, outs = _run(c, dt, None, prec=torch.float32)
        raw = F.as16(outs["view"]["raw16"].contiguous(), dt).float()
        big = ops["kinds"] == F.BIG
        assert int(big.sum()) > 3 and torch.isfinite(raw).all()
        want = 65504.0 if dt == "fp16" else float(torch.tensor(1e5).bfloat16())
        assert (raw[big][:, 0] == want).all() and (raw[big][:, -1] == -want).all()
    ops, outs = _run(c, "fp16", None, prec=torch.float32)
    s, _ = F.evaluate(ops, torch.arange(c["M"]), torch.float32)
    outs["view"]["raw16"][:] = s.half().view(torch.int16)     # the non-saturating conversion
    with pytest.raises(AssertionError, match="raw16"):
        F.check_bits(ops, outs)


def test_case_table_reaches_every_kernel_form_and_edge():
    """The GPU file's table: every form on both sides of the dispatch, both walker widths, every listed M and C, grouped with add_groups in {0, G - 1, G}, and every
    row kind in every case of 5 rows or more -- first rows, last rows and group boundaries among the stress rows."""
    hit = {(c["form"], F.kernel_name(c["M"], c["C"])) for c in F.CASES}
    for f in F.FORMS:
        assert (f, "ln") in hit and ((f, "ln_rows/3") in hit or (f, "ln_rows/4") in hit), f
    assert {k for _, k in hit} == {"ln", "ln_rows/3", "ln_rows/4"}
    Ms, Cs = {c["M"] for c in F.CASES}, {c["C"] for c in F.CASES}
    assert {1, 3, 4, 5, 1000, 65535, 65536, 65537, 8192 * 9 - 1, 65536 + 37, 307200, 35, 12 * 21504, 12 * 5463} <= Ms
    assert {768, 1024, 128, 200, 260, 772} <= Cs
    for R, G in ((7, 5), (5463, 12)):
        assert {c["add_groups"] for c in F.CASES if c["R"] == R and c["G"] == G} >= {0, G - 1, G}
    for c in F.CASES:
        if c["M"] > 400000 or c["M"] < 5:
            continue
        n = c["R"] or c["M"]
        k = F.row_kinds(n, F.FORMS[c["form"]].get("big", False), "cpu")
        assert set(k.tolist()) >= {0, 1, 2, 3, 4}, c["name"]
        assert (k[:4] > 0).all() and (k[-3:] > 0).any(), c["name"]
