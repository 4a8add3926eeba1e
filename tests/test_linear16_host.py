"""No GPU: the host side of the bf16 training Linears -- the additive ABI 21 switch ``must3r_hip_train_linear_mode`` of the library as built here, the context
manager over it, and the reference arithmetic that tests/test_linear16_gpu.py holds the kernels to (tests/linear16_ref.py).

The reference is checked against the unrounded fp64 product: within 2^-7 + 2^-16 of sum |a| |w| per element for every input (two operand roundings of 2^-8),
and within 2^-8 + 2^-18 where the contraction has 34 terms or more (test_reference_gap_where_the_contraction_has_many_terms derives the 34).  Four
planted defects show what the operator bound ``(K_c + 4) 2^-24 (sum |a^| |w^| + ...)`` sees.  The factor by which a defect's worst element exceeds the bound
is printed for every shape.  A defect is seen where the factor is above 1; it is asked to be above WIDE = 4 (the margin the project's parity rule leaves a
result: a defect 4 times past a bound that a correct kernel meets with room cannot hide in that room).

The inputs are the GPU test's own (``linear16_ref.inputs`` and ``wgrad_inputs``, the same seeds' generators and the same rows scaled by 2^+-20), since it is
that test's bound on that test's data whose sight is in question.  Factors measured here (seeds fixed): truncation 32 ... 40000, one operand unrounded
9.8 ... 10400, a dropped half step 1.2e5 ... 7.8e5, db from a rounded dZ 30 ... 6500; at the 2056-row weight gradient 125, 29 and 30.  The bound is per element,
and the elements that show a defect there are those of the row scaled by 2^20, where one product carries the sum.  (On plain randn rows the bound, one
rounding per addition in the worst case, grows like K_c^2 and a rounding defect like sqrt(K_c): at 2056 plain rows one unrounded operand is 2.1 and a rounded
db 0.9 times the bound.  The scaled rows of the test's inputs are what keeps the check sharp at that length.)
"""
import ctypes as C
import re
import threading

import pytest
import torch

import linear16_ref as LR
from conftest import ROOT
from must3r_amd import _lib, _train_common as TCM, train_block as TB

WIDE = 4.0
# M, N, K of the forward (dgrad contracts over N where N % 16 == 0); the GPU test's shapes
FORWARD = [(1, 4, 16), (19, 68, 48), (70, 128, 64), (129, 192, 768), (300, 68, 16), (300, 192, 48)]
# rows, O, K of the weight gradient
WGRAD = [(1, 4, 16), (127, 68, 48), (129, 128, 64), (2056, 192, 128)]


@pytest.fixture(autouse=True)
def _default_mode():
    lib = _lib.load()
    lib.must3r_hip_train_linear_mode(0)
    yield
    lib.must3r_hip_train_linear_mode(0)


def test_symbol_and_abi():
    lib = _lib.load()
    assert "must3r_hip_train_linear_mode" in _lib.EXPORTS and _lib.PROTOTYPES["must3r_hip_train_linear_mode"] == (C.c_int, [C.c_int])
    fn = lib.must3r_hip_train_linear_mode
    assert fn.restype is C.c_int and fn.argtypes == [C.c_int]
    assert lib.must3r_hip_abi_version() == 21 and _lib.ABI_VERSION == 21
    h = open(f"{ROOT}/include/must3r_hip.h").read()
    assert "#define MUST3R_HIP_ABI_VERSION 21" in h and "int must3r_hip_train_linear_mode(int mode);" in h
    assert re.search(r"#define MUST3R_TRAIN_LINEAR_F32\s+0\b", h) and re.search(r"#define MUST3R_TRAIN_LINEAR_BF16\s+1\b", h)
    assert (_lib.TRAIN_LINEAR_F32, _lib.TRAIN_LINEAR_BF16) == (0, 1)


def test_default_set_query_and_refusals():
    lib = _lib.load()
    fn = lib.must3r_hip_train_linear_mode
    assert fn(-1) == 0
    assert fn(1) == 0 and fn(-1) == 1          # returns the previous mode
    assert fn(1) == 1 and fn(0) == 1 and fn(-1) == 0
    for start in (0, 1):
        fn(start)
        for bad in (2, -2, 1 << 20):
            fn(-1)
            assert fn(bad) == -1
            assert lib.must3r_hip_last_error().decode() and "train_linear_mode" in lib.must3r_hip_last_error().decode()
            assert fn(-1) == start


def test_mode_is_per_thread():
    lib = _lib.load()
    fn = lib.must3r_hip_train_linear_mode
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


def test_linear_precision_context():
    assert TB.linear_precision is TCM.linear_precision and TB.current_precision is TCM.current_precision
    assert TB.current_precision() == "fp32"
    with TB.linear_precision("bf16"):
        assert TB.current_precision() == "bf16"
        with TB.linear_precision("fp32"):
            assert TB.current_precision() == "fp32"
            with TB.linear_precision("bf16"):
                assert TB.current_precision() == "bf16"
                with TB.linear_precision(None):
                    assert TB.current_precision() == "bf16"
            assert TB.current_precision() == "fp32"
        assert TB.current_precision() == "bf16"
    assert TB.current_precision() == "fp32"
    with pytest.raises(KeyError):
        with TB.linear_precision("bf16"):
            raise KeyError("x")
    assert TB.current_precision() == "fp32"
    with TB.linear_precision(None):
        assert TB.current_precision() == "fp32"
    for bad in ("fp16", "BF16", 1, ""):
        with TB.linear_precision("bf16"):
            with pytest.raises(ValueError, match="linear_precision"):
                with TB.linear_precision(bad):
                    pass
            assert TB.current_precision() == "bf16"
    assert TB.current_precision() == "fp32"


def test_package_does_not_re_export_the_switch():
    import must3r_amd
    assert not hasattr(must3r_amd, "linear_precision")


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rounding_is_nearest_even_and_keeps_nan_and_inf():
    f = lambda bits: torch.tensor([bits], dtype=torch.int32).view(torch.float32)
    assert float(LR.rnd(f(0x3F808000))) == 1.0                          # a tie goes to the even neighbour ...
    assert float(LR.rnd(f(0x3F818000))) == float(f(0x3F820000))         # ... in both directions
    assert float(LR.rnd(f(0x3F808001))) == float(f(0x3F810000))
    assert float(LR.rnd(f(0x7F7FFFFF))) == float("inf")                 # the largest fp32 rounds past the largest bf16
    t = LR.rnd(torch.tensor([float("inf"), float("-inf"), float("nan")]))
    assert float(t[0]) == float("inf") and float(t[1]) == float("-inf") and bool(torch.isnan(t[2]))
    assert float(LR._chop(f(0x3F80FFFF))) == 1.0


def _gaps(M, N, K, scaled_rows=True):
    """{contraction length: worst |a^ w^ - a w| / sum |a| |w|} of the three products of a shape: forward (over K), dgrad (over N), wgrad (over the M rows)"""
    a, w, _, res = LR.inputs(M, N, K, 11, scaled_rows=scaled_rows)
    out = {}
    for Kc, g in [(K, LR.unrounded_gap(a, w.t())), (M, LR.unrounded_gap(res.t(), a))] + ([(N, LR.unrounded_gap(res, w))] if N % 16 == 0 else []):
        out[Kc] = max(out.get(Kc, 0.0), g)
    return out


@pytest.mark.parametrize("M,N,K", FORWARD)
def test_reference_is_within_two_roundings_of_the_unrounded_product(M, N, K):
    """The bound that holds for every input: bf16 keeps 8 significant bits, rounding to nearest moves a value by at most 2^-8 of itself, so a product of two
    rounded operands is within (1 + 2^-8)^2 - 1 = 2^-7 + 2^-16 of the exact one, and so is every element relative to sum |a| |w|.  A contraction of one row (the
    1-row weight gradient) or one dominated by a row scaled by 2^20 comes close to it: 1.6 to 1.9 x 2^-8 here."""
    gap = max(_gaps(M, N, K).values())
    print(f"{M}x{N}x{K}: |a^ w^ - a w| / sum |a| |w| = {gap / 2 ** -8:.3f} x 2^-8")
    assert gap <= 2.0 ** -7 + 2.0 ** -16


MANY_TERMS = 34


@pytest.mark.parametrize("M,N,K", FORWARD)
def test_reference_gap_where_the_contraction_has_many_terms(M, N, K):
    """|a^ w^ - a w| <= (2^-8 + 2^-18) sum |a| |w|: half of the bound above.  It is no bound for every input (one product alone can err by 2^-7), but it
    holds on randn operands once the contraction has enough comparable terms: the error of one product has a standard deviation of at most
    sqrt(2 / 3) 2^-8 of it (two roundings, each uniform in +-2^-8 at worst), the errors of the K_c products are independent, and for products of Gaussians
    sqrt(sum t^2) / sum |t| = (pi / 2) / sqrt(K_c); so the gap of an element is about 1.3 / sqrt(K_c) x 2^-8 at one sigma, and the worst of some 1e4 ... 1e5
    elements (4.5 sigma) stays below 2^-8 from K_c = 5.8^2 = 34 on.  Held from MANY_TERMS = 34 on; of the contraction lengths of the tests that is 48 and more.
    This is a statistical argument, not a bound: it says what randn operands give with overwhelming probability, and the test runs it on fixed seeds.  Measured over 8 seeds: 0.15 ... 0.63 of the figure there,
    0.73 ... 0.84 at 19 terms, 0.86 ... 0.97 at 16, 0.9 ... 1.7 at one.  Rows are not scaled here: a row of 2^20 among the rows of a weight gradient is a
    contraction of one term."""
    gaps = {Kc: g for Kc, g in _gaps(M, N, K, scaled_rows=False).items() if Kc >= MANY_TERMS}
    for Kc, g in gaps.items():
        print(f"{M}x{N}x{K}, {Kc} terms: {g / (2.0 ** -8 + 2.0 ** -18):.3f} of 2^-8 + 2^-18")
    assert all(g <= 2.0 ** -8 + 2.0 ** -18 for g in gaps.values()), gaps


def test_the_figure_is_held_at_every_shape_with_many_terms():
    held = {Kc for s in FORWARD for Kc in _gaps(*s, scaled_rows=False) if Kc >= MANY_TERMS}
    assert {48, 64, 768} <= held and 16 not in held


def _factor(got, ref, bound):
    return float(((got - ref).abs() / bound).max())


@pytest.mark.parametrize("M,N,K", FORWARD)
def test_planted_defects_exceed_the_bound_forward_and_dgrad(M, N, K):
    a, w, b, res = LR.inputs(M, N, K, 12)
    forms = [("forward", lambda d: LR.forward(a, w, b, res, defect=d), K)]
    if N % 16 == 0:
        forms.append(("dgrad", lambda d: LR.dgrad(res, w, defect=d), N))
    for name, fn, Kc in forms:
        ref, scale = fn(None)
        bound = LR.bound(Kc, scale)
        for d in ("truncate", "one_operand") + (("drop_tail",) if Kc % 32 == 16 else ()):
            f = _factor(fn(d)[0], ref, bound)
            print(f"{name} {M}x{N}x{K} K_c {Kc} {d}: {f:.1f} x the bound")
            assert f >= WIDE, (name, d, f)


@pytest.mark.parametrize("R,O,K", WGRAD)
def test_planted_defects_exceed_the_bound_wgrad(R, O, K):
    dz, a = LR.wgrad_inputs(R, O, K, 23)          # the GPU test's inputs: one row of dz scaled by 2^20, one of a by 2^-20
    dW, sW, db, sb = LR.wgrad(dz, a)
    for d in ("truncate", "one_operand", "db_rounded") + (("drop_tail",) if R > 16 and R % 32 == 16 else ()):
        got = LR.wgrad(dz, a, defect=d)
        f = _factor(got[2], db, LR.bound(R, sb)) if d == "db_rounded" else _factor(got[0], dW, LR.bound(R, sW))
        print(f"wgrad {R}x{O}x{K} {d}: {f:.2f} x the bound")
        assert f >= WIDE, (d, f)
    # a correct emulation with another summation order (fp32 partial sums of 128 rows, added in fp32) is inside the bound
    parts = [(LR.rnd(dz[r:r + 128]).t() @ LR.rnd(a[r:r + 128])).float() for r in range(0, R, 128)]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    assert _factor(acc.double(), dW, LR.bound(R, sW)) <= 1.0
