"""No GPU: the host side of the bf16 training attention core -- the additive ABI 21 switch ``must3r_hip_train_attention_mode`` of the library as built here, the
three context managers over it (``attention_precision``, ``current_attention_precision``, ``amp``), and the reference arithmetic that
tests/test_attn16_gpu.py holds the kernels to (tests/attn16_ref.py).

The reference: with its five roundings removed it is tests/attn_grad_ref.py (rtol 1e-12 in fp64).  Then the parity rule of the GPU test,
``e <= 4 e_ref + 32 2^-24 m`` against the unrounded fp64 yardstick with ``e_ref`` the fp32 run of the reference, is applied to a stand-in for the GPU: the fp32
run of the same arithmetic in the kernel's own order (``tiled=True``: key tiles of 64, a running maximum, p rounded relative to it), clean and with each
planted defect of ``attn16_ref.DEFECTS``.  The clean stand-in passes on all seven cases.  A defect is exposed where its worst ratio over the cases and tensors
is above 1; the ratios are printed, and what the rule does not expose at these shapes is listed in ``NOT_EXPOSED`` and asserted to be exactly that list, so
that neither a sharper nor a blunter rule goes unnoticed.  The rule is a rule on the size of the bf16 rounding error: it measures against the UNROUNDED fp64
result and allows four times the error of a correct bf16 run, so a defect that changes the result by less than a few roundings of an operand cannot show in it;
the exact single-key checks of the GPU test are what sees a truncated operand.  Measured here (seeds fixed), worst ratio over the cases: clean 0.259;
operands truncated 1.069 (exposed, barely: truncation doubles the operand error and biases it); P and dS truncated 0.445, l from the rounded p 0.366, delta from
the rounded dO 0.259, P unrounded in dV 0.279, dP from the unrounded dO 0.283, dS unrounded in dQ 0.259, V unrounded in the forward 0.319 (not exposed); s
dropped on dK 437.5 (profiles/attn16_parity.txt, section "host").  That assertion stays: it is why there are two rules.

The second rule, ``grad_parity.compare_rounded``, is what sees a wrong rounding point.  Its yardstick is the fp64 run of the SAME rounded arithmetic in the
kernel's tile order (``core(float64, tiled=True)``; tests/attn16_ref.py states why that is where the kernel rounds), so only the fp32 accumulation is left in
the comparison, a few units of 2^-24 m instead of 10^5 -- except in the few places where a p or a dS lies so near a bf16 boundary that fp32 and fp64 round it
to different neighbours.  So the unit is the (row, head) segment of the written rows, a segment's error its max |. - y64|, and the rule
``q(e) <= 4 q(e_ref) + 32 2^-24 m`` on the 0.9 quantile q over the segments, ``e_ref`` from the fp32 run of the reference; the tenth it steps over is a
condition, not a measurement.  lse has no flip (l sums the unrounded p) and is held entry by entry:
``|lse - lse64| <= 4 max|lse32 - lse64| + 32 2^-24 max(1, max|lse64|)``.  The stand-in for the GPU is the fp32 run in the kernel's own form
(``exp2=True``: s log2 e as one fp32 constant after the product, exp2, O = acc (1 / l), lse = lse2 ln 2), on the seven cases and the key-mask case.  Measured
here: clean, worst ratio 0.093, worst share of segments above the bound 0.0145 (asserted <= 0.05: the inputs keep a correct run well inside the tenth), lse
0.072 of its bound.  All nine planted defects fail the rule in EVERY case, in every tensor they can reach and in no other (``ACTS``, asserted: the table is
the signature by which a failing GPU run names its rounding point); the smallest over the cases of the largest ratio over the tensors: operands truncated
2886, P and dS truncated 764, l from the rounded p 134 (and lse at 24 to 228 times its bound, the only defect besides the truncated operands that moves lse),
delta from the rounded dO 267, P unrounded in dV 233 -- these five asserted >= 50 --, s dropped on dK 1.2e6, dP from the unrounded dO 550, dS unrounded in
dQ 265, V unrounded in the forward 350.  NOT exposed by the rounded rule: none (``NOT_EXPOSED_ROUNDED``).  profiles/attn16_parity.txt, section "host, rounded".
"""
import ctypes as C
import functools
import os
import re
import threading

import pytest
import torch

import attn16_ref as R16
import attn_grad_ref as AR
import grad_parity as GP
from conftest import ROOT
from must3r_amd import _lib, _train_common as TCM, train_attention as TA, train_block as TB

# the planted defects the parity rule against the UNROUNDED yardstick does not expose at the seven shapes (worst ratio <= 1); see the module docstring
NOT_EXPOSED = ("truncate_p", "l_rounded", "delta_rounded", "dv_unrounded_p", "dp_unrounded_do", "ds_unrounded_dq", "v_unrounded")


@pytest.fixture(autouse=True)
def _default_mode():
    lib = _lib.load()
    lib.must3r_hip_train_attention_mode(0)
    lib.must3r_hip_train_linear_mode(0)
    yield
    lib.must3r_hip_train_attention_mode(0)
    lib.must3r_hip_train_linear_mode(0)


def test_symbol_and_abi():
    lib = _lib.load()
    assert "must3r_hip_train_attention_mode" in _lib.EXPORTS and _lib.PROTOTYPES["must3r_hip_train_attention_mode"] == (C.c_int, [C.c_int])
    fn = lib.must3r_hip_train_attention_mode
    assert fn.restype is C.c_int and fn.argtypes == [C.c_int]
    assert lib.must3r_hip_abi_version() == 21 and _lib.ABI_VERSION == 21
    h = open(f"{ROOT}/include/must3r_hip.h").read()
    assert "#define MUST3R_HIP_ABI_VERSION 21" in h and "int must3r_hip_train_attention_mode(int mode);" in h
    assert re.search(r"#define MUST3R_TRAIN_ATTENTION_F32\s+0\b", h) and re.search(r"#define MUST3R_TRAIN_ATTENTION_BF16\s+1\b", h)
    assert (_lib.TRAIN_ATTENTION_F32, _lib.TRAIN_ATTENTION_BF16) == (0, 1)
    # the Linears' switch is what it was: two modes, 2 refused
    assert lib.must3r_hip_train_linear_mode(2) == -1 and lib.must3r_hip_train_linear_mode(-1) == 0


def test_default_set_query_and_refusals():
    lib = _lib.load()
    fn = lib.must3r_hip_train_attention_mode
    assert fn(-1) == 0
    assert fn(1) == 0 and fn(-1) == 1          # returns the previous mode
    assert fn(1) == 1 and fn(0) == 1 and fn(-1) == 0
    for start in (0, 1):
        fn(start)
        for bad in (2, -2, 1 << 20):
            fn(-1)
            assert fn(bad) == -1
            assert lib.must3r_hip_last_error().decode() and "train_attention_mode" in lib.must3r_hip_last_error().decode()
            assert fn(-1) == start


def test_mode_is_per_thread():
    lib = _lib.load()
    fn = lib.must3r_hip_train_attention_mode
    seen = {}

    def worker(name, set_to):
        seen[name + "_start"] = fn(-1)
        if set_to is not None:
            fn(set_to)
        seen[name + "_end"] = fn(-1)

    fn(1)
    t = threading.Thread(target=worker, args=("a", None))
    t.start(); t.join()
    assert seen["a_start"] == 0 and seen["a_end"] == 0          # a new thread starts at F32 whatever its parent's mode
    fn(0)
    t = threading.Thread(target=worker, args=("b", 1))
    t.start(); t.join()
    assert seen["b_start"] == 0 and seen["b_end"] == 1 and fn(-1) == 0          # and what it sets is its own


def test_the_two_modes_are_independent():
    lib = _lib.load()
    lin, att = lib.must3r_hip_train_linear_mode, lib.must3r_hip_train_attention_mode
    for a in (0, 1):
        for b in (0, 1):
            lin(a), att(b)
            assert (lin(-1), att(-1)) == (a, b)
            att(1 - b)
            assert lin(-1) == a
            lin(1 - a)
            assert att(-1) == 1 - b
    lin(0), att(0)
    with TB.linear_precision("bf16"):
        assert (TB.current_precision(), TB.current_attention_precision()) == ("bf16", "fp32")
        with TB.attention_precision("bf16"):
            assert (TB.current_precision(), TB.current_attention_precision()) == ("bf16", "bf16")
            with TB.linear_precision("fp32"):
                assert (TB.current_precision(), TB.current_attention_precision()) == ("fp32", "bf16")
        assert (TB.current_precision(), TB.current_attention_precision()) == ("bf16", "fp32")
    with TB.attention_precision("bf16"):
        assert (TB.current_precision(), TB.current_attention_precision()) == ("fp32", "bf16")
    assert (TB.current_precision(), TB.current_attention_precision()) == ("fp32", "fp32")


def test_attention_precision_context():
    assert TB.attention_precision is TCM.attention_precision and TB.current_attention_precision is TCM.current_attention_precision and TB.amp is TCM.amp
    assert TA.attention_precision is TCM.attention_precision
    cur = TB.current_attention_precision
    assert cur() == "fp32"
    with TB.attention_precision("bf16"):
        assert cur() == "bf16"
        with TB.attention_precision("fp32"):
            assert cur() == "fp32"
            with TB.attention_precision("bf16"):
                assert cur() == "bf16"
                with TB.attention_precision(None):
                    assert cur() == "bf16"
            assert cur() == "fp32"
        assert cur() == "bf16"
    assert cur() == "fp32"
    with pytest.raises(KeyError):
        with TB.attention_precision("bf16"):
            raise KeyError("x")
    assert cur() == "fp32"
    with TB.attention_precision(None):
        assert cur() == "fp32"
    for bad in ("fp16", "BF16", 1, ""):
        with TB.attention_precision("bf16"):
            with pytest.raises(ValueError, match="attention_precision"):
                with TB.attention_precision(bad):
                    pass
            assert cur() == "bf16"
    assert cur() == "fp32"


def test_amp_context():
    both = lambda: (TB.current_precision(), TB.current_attention_precision())
    assert both() == ("fp32", "fp32")
    with TB.amp("bf16"):
        assert both() == ("bf16", "bf16")
        with TB.amp("fp32"):
            assert both() == ("fp32", "fp32")
            with TB.amp(None):
                assert both() == ("fp32", "fp32")
        assert both() == ("bf16", "bf16")
        with TB.attention_precision("fp32"):
            assert both() == ("bf16", "fp32")
    assert both() == ("fp32", "fp32")
    with pytest.raises(KeyError):
        with TB.amp("bf16"):
            raise KeyError("x")
    assert both() == ("fp32", "fp32")
    for bad in ("fp16", "BF16", 1, ""):
        with TB.linear_precision("bf16"):
            with pytest.raises(ValueError, match="amp"):
                with TB.amp(bad):
                    pass
            assert both() == ("bf16", "fp32")
    assert both() == ("fp32", "fp32")


def test_package_does_not_re_export_the_switches():
    import must3r_amd
    for name in ("attention_precision", "current_attention_precision", "amp"):
        assert not hasattr(must3r_amd, name), name


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name):
    """(case, unrounded fp64 autograd, fp32 run of attn16_ref): computed once, shared, never modified."""
    case = AR.make_case(name)
    return case, AR.grads(case, torch.float64), R16.core(case, torch.float32)


def test_rounding_helpers():
    f = lambda bits: torch.tensor([bits], dtype=torch.int32).view(torch.float32)
    assert float(R16.rnd(f(0x3F808000))) == 1.0 and float(R16.rnd(f(0x3F818000))) == float(f(0x3F820000))     # ties to even, both ways
    assert float(R16.rnd(f(0x3F808001))) == float(f(0x3F810000)) and float(R16.chop(f(0x3F80FFFF))) == 1.0
    t = R16.rnd(torch.tensor([float("inf"), float("-inf"), float("nan")]))
    assert float(t[0]) == float("inf") and float(t[1]) == float("-inf") and bool(torch.isnan(t[2]))
    assert R16.rnd(torch.tensor([1.00390625], dtype=torch.float64)).dtype == torch.float64


@pytest.mark.parametrize("name", AR.CASES)
def test_without_roundings_it_is_the_yardstick(name):
    case, g64, _ = _reference(name)
    for tiled in (False, True):
        got = R16.core(case, torch.float64, rounding=False, tiled=tiled)
        for k in AR.NAMES:
            assert torch.allclose(got[k], g64[k], rtol=1e-12, atol=1e-12 * float(g64[k].abs().max())), (name, tiled, k)


def _worst(rows):
    return max(r[5] for r in rows)


def test_parity_rule_on_the_emulation_and_the_planted_defects():
    """The rule of tests/test_attn16_gpu.py with the fp32 tiled emulation in place of the GPU; every row is printed by ``compare`` before it is asserted."""
    clean = []
    for name in AR.CASES:
        case, g64, g32 = _reference(name)
        GP.compare(clean, f"host {name}", R16.core(case, torch.float32, tiled=True), g64, {k: g32[k] for k in AR.NAMES})
    print(f"clean emulation: worst ratio {_worst(clean):.3f}")
    assert _worst(clean) <= 1.0
    ratios = {}
    for d in R16.DEFECTS:
        rows = []
        for name in AR.CASES:
            case, g64, g32 = _reference(name)
            try:
                GP.compare(rows, f"host {d} {name}", R16.core(case, torch.float32, tiled=True, defect=d), g64, {k: g32[k] for k in AR.NAMES})
            except AssertionError:
                pass          # a defect is meant to fail the rule; its rows are in ``rows``
        ratios[d] = _worst(rows)
        print(f"defect {d}: worst ratio {ratios[d]:.3f} ({'exposed' if ratios[d] > 1 else 'NOT exposed'})")
    assert tuple(d for d in R16.DEFECTS if not ratios[d] > 1.0) == NOT_EXPOSED, ratios


# ---------------------------------------------------------------------------------------------------------------------------------
# the rounded rule: against the fp64 run of the same rounded arithmetic, on a quantile of (row, head) segments
# ---------------------------------------------------------------------------------------------------------------------------------
ROUNDED_CASES = AR.CASES + ("cross_shared key mask",)
# the tensors a defect can reach: delta enters dS alone; the dV product reads P and dO^ alone; dP enters dS alone; V is read by the forward (O, and through
# delta dQ and dK) but dV = P^T^ dO^ holds P = exp(S - lse), which never saw V
ACTS = {"truncate_operand": AR.NAMES, "truncate_p": AR.NAMES, "l_rounded": AR.NAMES, "delta_rounded": ("dQ", "dK"), "dk_no_scale": ("dK",),
        "dv_unrounded_p": ("dV",), "dp_unrounded_do": ("dQ", "dK"), "ds_unrounded_dq": ("dQ",), "v_unrounded": ("O", "dQ", "dK")}
AT_LEAST_50 = ("truncate_operand", "truncate_p", "l_rounded", "delta_rounded", "dv_unrounded_p")
NOT_EXPOSED_ROUNDED = ()          # the planted defects the rounded rule does not expose in every case: none


@functools.lru_cache(maxsize=None)
def _rounded_reference(name):
    """(case, keeps, fp64 and fp32 tiled runs of the rounded arithmetic, counted rows, the exp2 stand-in for the GPU): computed once, shared, never modified."""
    if name == "cross_shared key mask":
        case, keep = R16.key_mask_case()
        keeps = list(keep)
    else:
        case, keeps = _reference(name)[0], None
    run = lambda dtype, **kw: R16.core(case, dtype, tiled=True, keep=keeps, **kw)
    return case, keeps, run(torch.float64), run(torch.float32), R16.written_rows(case, keeps), run(torch.float32, exp2=True)


def _rounded(rows, tag, name, got):
    case, _, y64, r32, counted, _ = _rounded_reference(name)
    GP.compare_rounded(rows, tag, got, {k: y64[k] for k in AR.NAMES}, r32, case["heads"], counted=counted)


@pytest.mark.parametrize("name", AR.CASES)
def test_the_rounded_yardstick_without_roundings_and_the_exp2_form(name):
    """``tiled`` and ``exp2`` change the order and the form, not the arithmetic: without roundings the exp2 stand-in is the fp32 run to fp32 accuracy."""
    case, g64, _ = _reference(name)
    a, b = R16.core(case, torch.float32, rounding=False, tiled=True, exp2=True), R16.core(case, torch.float32, rounding=False, tiled=True)
    for k in AR.NAMES:
        m = float(g64[k].abs().max())
        assert float((a[k].double() - g64[k]).abs().max()) <= 4 * float((b[k].double() - g64[k]).abs().max()) + 32 * GP.U * m, (name, k)
    with pytest.raises(AssertionError):
        R16.core(case, torch.float64, tiled=True, exp2=True)


def test_written_rows_are_the_nonzero_rows():
    for name in ROUNDED_CASES:
        case, _, y64, _, counted, _ = _rounded_reference(name)
        for k in AR.NAMES:
            assert not bool(y64[k][~counted[k]].any()), (name, k)
            assert bool(counted[k].any()), (name, k)
    _, _, _, _, counted, _ = _rounded_reference("degenerate")
    assert int(counted["O"].sum()) == 40 and int(counted["dK"].sum()) == 70


def test_compare_rounded_steps_over_a_capped_share_only():
    """The rule itself on made-up errors: segments are (row, head); a whole-ulp error in under a tenth of them passes and is reported as the share; in more
    than a tenth it fails; rows not counted do not dilute."""
    heads, R = 2, 50
    y = {"x": torch.ones((R, heads * 64), dtype=torch.float64)}
    r32 = {"x": y["x"].float() + 2.0 ** -24}
    got = y["x"].float().clone()
    got[:4, 0] += 2.0 ** -8          # 4 of 100 segments
    rows = []
    GP.compare_rounded(rows, "toy", {"x": got}, y, r32, heads)
    assert rows[0][6] == pytest.approx(0.04) and rows[0][5] <= 1.0
    got[:12, 70] += 2.0 ** -8        # and 12 more, in the other head
    with pytest.raises(AssertionError):
        GP.compare_rounded(rows, "toy", {"x": got}, y, r32, heads)
    assert rows[1][6] == pytest.approx(0.16) and rows[1][5] > 1.0
    counted = torch.zeros(R, dtype=torch.bool)
    counted[:10] = True              # 4 + 10 of 20 counted segments
    with pytest.raises(AssertionError):
        GP.compare_rounded(rows, "toy", {"x": got}, y, r32, heads, counted={"x": counted})
    assert rows[2][6] == pytest.approx(0.7)


def test_rounded_rule_on_the_stand_in_and_the_planted_defects():
    """``compare_rounded`` with the fp32 exp2 stand-in in place of the GPU, clean and with each of the nine planted defects, per case and tensor; every row is
    printed before it is asserted, and the table goes to the file M3R_ATTN16_HOST_TABLE names (kept in profiles/attn16_parity.txt, section "host, rounded")."""
    lines = []

    def say(text):
        print(text)
        lines.append("# " + text)

    clean = []
    for name in ROUNDED_CASES:
        _rounded(clean, f"host rounded {name}", name, _rounded_reference(name)[5])
    print(f"host rounded, clean stand-in: worst ratio {_worst(clean):.3f}, worst share above the bound {max(r[6] for r in clean):.4f}")
    assert _worst(clean) <= 1.0
    assert all(r[6] <= 0.05 for r in clean), [r for r in clean if r[6] > 0.05]          # the inputs keep a correct run well inside the 0.1 the rule steps over
    lse_ratio = {}
    for name in ROUNDED_CASES:
        _, _, y64, r32, _, got = _rounded_reference(name)
        fin, bound = R16.lse_rounded_bound(y64["lse"], r32["lse"])
        assert bool((torch.isfinite(got["lse"]) == fin).all())
        lse_ratio[name] = float((got["lse"][fin].double() - y64["lse"][fin]).abs().max()) / bound
    say(f"host rounded, clean stand-in: worst lse error / bound {max(lse_ratio.values()):.3f}")
    assert max(lse_ratio.values()) <= 1.0
    smallest = {}
    for d in R16.DEFECTS:
        for name in ROUNDED_CASES:
            case, keeps, y64, r32, _, _ = _rounded_reference(name)
            got, rows = R16.core(case, torch.float32, tiled=True, keep=keeps, exp2=True, defect=d), []
            try:
                _rounded(rows, f"host rounded {d} {name}", name, got)
            except AssertionError:
                pass          # a defect is meant to fail the rule; its rows are in ``rows``
            ratio = {r[1]: r[5] for r in rows}
            fin, bound = R16.lse_rounded_bound(y64["lse"], r32["lse"])
            lse = float((got["lse"][fin].double() - y64["lse"][fin]).abs().max()) / bound
            say(f"host rounded defect {d:<17}{name:<23}" + "".join(f"{k} {ratio[k]:>10.1f}  " for k in AR.NAMES) + f"lse {lse:>8.2f}")
            # the signature: above the bound in every tensor the defect can reach, inside it in every other
            assert d in NOT_EXPOSED_ROUNDED or all(ratio[k] > 1.0 for k in ACTS[d]), (d, name, ratio)
            assert all(ratio[k] <= 1.0 for k in AR.NAMES if k not in ACTS[d]), (d, name, ratio)
            smallest[d] = min(smallest.get(d, float("inf")), max(ratio.values()))
            if d == "l_rounded":
                assert lse > 1.0, (name, lse)          # the one defect that reaches lse without touching an operand
        say(f"host rounded defect {d}: smallest over the cases of the largest ratio over the tensors {smallest[d]:.1f} "
            f"({'exposed in every case' if smallest[d] > 1 else 'NOT exposed'})")
    assert tuple(d for d in R16.DEFECTS if not smallest[d] > 1.0) == NOT_EXPOSED_ROUNDED, smallest
    assert all(smallest[d] >= 50.0 for d in AT_LEAST_50), smallest
    path = os.environ.get("M3R_ATTN16_HOST_TABLE")
    if path:
        GP.append_rounded_table(path, ["#", "# host, rounded: tests/test_attn16_host.py, the rounded rule with the fp32 exp2 stand-in (attn16_ref.core(tiled=True, exp2=True))"
                                       " in place of the GPU"], clean, (38, 56))
        with open(path, "a") as f:
            f.writelines(line + "\n" for line in lines)
