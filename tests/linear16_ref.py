"""The reference arithmetic of the bf16 training Linears (csrc/train_lin16.hip): operands rounded with ``.to(torch.bfloat16)`` and every product and sum
formed in fp64.  A product of two bf16 values is exact in fp32 (8-bit significands: 16 bits), so against this reference the only error of a correct kernel is
its fp32 summation and the additions of its epilogue:

    |got - ref64| <= (K_c + 4) 2^-24 (sum_k |a^_k| |w^_k| + |bias| + |res|)           ``bound``

with K_c the contraction length -- one rounding per addition in the worst case, whatever the order in which the MFMA and the K loop add.

``defect`` plants what a wrong kernel could do, for the CPU test that shows the bound sees it: ``"truncate"`` (operands chopped to bf16 instead of rounded to
nearest even), ``"one_operand"`` (the second operand of the product left unrounded), ``"drop_tail"`` (the last 16 contraction indices dropped: the half
step of K % 32 == 16), ``"db_rounded"`` (the bias gradient summed from the rounded dZ).  Shared by tests/test_linear16_host.py and tests/test_linear16_gpu.py.
"""
import torch

U = 2.0 ** -24
DEFECTS = ("truncate", "one_operand", "drop_tail", "db_rounded")


def rnd(t):
    """fp32 -> bf16 (nearest even) -> fp64"""
    return t.to(torch.bfloat16).double()


def _chop(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def _operands(a, b, defect):
    """fp64 images of the two operands as the (possibly defective) kernel multiplies them; a is contracted along dim 1, b along dim 0"""
    if defect == "truncate":
        a64, b64 = _chop(a), _chop(b)
    elif defect == "one_operand":
        a64, b64 = rnd(a), b.double()
    else:
        a64, b64 = rnd(a), rnd(b)
    if defect == "drop_tail":
        a64, b64 = a64[:, :-16], b64[:-16]
    return a64, b64


def _product(a, b, defect=None):
    """(a^ b^ in fp64, sum |a^| |b^| of the correct product): a [P, Kc], b [Kc, Q]"""
    a64, b64 = _operands(a, b, defect)
    return a64 @ b64, rnd(a).abs() @ rnd(b).abs()


def forward(a, w, bias=None, res=None, defect=None):
    """out = a w^T + bias (+ res): (ref64, scale); a [M, K], w [N, K]"""
    ref, scale = _product(a, w.t(), defect)
    for t in (bias, res):
        if t is not None:
            ref, scale = ref + t.double(), scale + t.double().abs()
    return ref, scale


def dgrad(dz, w, defect=None):
    """dX = dZ W: (ref64, scale); dz [M, O], w [O, K]"""
    return _product(dz, w, defect)


def wgrad(dz, a, defect=None):
    """dW = dZ^T A and db = column sums of the unrounded dZ: (dW64, scale_dW, db64, scale_db); dz [R, O], a [R, K]"""
    dW, scale = _product(dz.t(), a, defect)
    src = rnd(dz) if defect == "db_rounded" else dz.double()
    return dW, scale, src.sum(0), dz.double().abs().sum(0)


def bound(Kc, scale):
    return (Kc + 4) * U * scale


def unrounded_gap(a, b):
    """max over the elements of |a^ b^ - a b| / sum |a| |b|, both products in fp64: at most 2^-7 + 2^-16 for any input (bf16 keeps 8 significant bits: two
    relative roundings of at most 2^-8 each and their product); on randn operands with many comparable terms it is well below 2^-8 (tests/test_linear16_host.py)"""
    got, _ = _product(a, b)
    exact, scale = a.double() @ b.double(), a.double().abs() @ b.double().abs()
    return float(((got - exact).abs() / scale).max())


def inputs(M, N, K, seed, ld=None, scaled_rows=True):
    """randn operands of a forward: a [M, ld or K] (the first K columns are the operand), w [N, K] / sqrt K, bias [N], res [M, N]; a few rows of a scaled by 2^+-20"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((M, ld or K), generator=g)
    if scaled_rows and M > 2:
        a[1] *= 2.0 ** 20
        a[M // 2] *= 2.0 ** -20
    return a, torch.randn((N, K), generator=g) * K ** -0.5, torch.randn(N, generator=g), torch.randn((M, N), generator=g)


def wgrad_inputs(R, O, K, seed):
    """randn operands of a weight gradient: dz [R, O], a [R, K]; with more than two rows, one row of dz scaled by 2^20 and one of a by 2^-20"""
    g = torch.Generator().manual_seed(seed)
    dz, a = torch.randn((R, O), generator=g), torch.randn((R, K), generator=g)
    if R > 2:
        dz[1] *= 2.0 ** 20
        a[R // 2] *= 2.0 ** -20
    return dz, a
