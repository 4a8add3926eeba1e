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
the rounded dO 0.259, P unrounded in dV 0.279 (not exposed); s dropped on dK 437.5 (profiles/attn16_parity.txt, section "host").
"""
import ctypes as C
import functools
import re
import threading

import pytest
import torch

import attn16_ref as R16
import attn_grad_ref as AR
import grad_parity as GP
from conftest import ROOT
from must3r_amd import _lib, _train_common as TCM, train_attention as TA, train_block as TB

# the planted defects the parity rule does not expose at the seven shapes (worst ratio <= 1); see the module docstring
NOT_EXPOSED = ("truncate_p", "l_rounded", "delta_rounded", "dv_unrounded_p")


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
