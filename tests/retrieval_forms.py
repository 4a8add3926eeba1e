"""Shared by tests/test_retrieval_forms_gpu.py (every entry point of csrc/retrieval.hip through the C ABI, against fp64) and tests/test_retrieval_forms_host.py
(the checks discriminate): the case tables, the operands, the fp64 references computed from the fp32 inputs the kernels read, the per-element bounds, the
canary-filled destinations, the checks, an emulation of topk_kernel's bitonic network that takes the comparator as a parameter, and an fp32 emulation of
what each kernel writes (with the defects the host file plants).  Nothing here needs a GPU.

Bounds (u = 2^-24; every one per element, none moves to fit a run):
  affine   out = fp32((A - sub) B + bias) + resid; s = sum_k |a_k - sub_k| |b_k| + |bias|, v64 the fp64 value before the residual.
           fp32:  |got - ref| <= (K + 4) u (s + |resid|): one rounding per operation in any order, fused or not (the derivation of linear16_ref.bound).
           fp64:  |got - ref| <= u |v64| + u |v64 + resid| + (K + 4) 2^-53 (s + |resid|): the two fp32 roundings the kernel makes plus fp64 accumulation,
                  i.e. the Whitener within half an fp32 ulp of the fp64 result.
  row_norm |got - ref| <= (C/2 + 2) u ref: C squares and C - 1 additions move the sum by at most (C + 1) u relatively, the root halves that and rounds once.
  spoc     t_c = sum_n |a_n f_nc|, ds_c = (N + 1) u t_c, n = max(|s64|_2, 1e-12): ds_c / n + |ref_c| |ds|_2 / n + (C/2 + 4) u |ref_c|
           (the sum's own error, the norm's share of it, and row_norm's budget plus the reciprocal and the product).
  l2       (L/2 + 4) u |ref|; an all-zero vector gives exact zeros; below 1e-12 the reference divides by 1e-12 as F.normalize does.
  ln       no closed bound (the error follows the row's conditioning): grad_parity.compare per row kind, e_gpu <= 4 e_ref + 32 u m with e_ref the error of
           fp32 F.layer_norm (+ F.gelu) on the CPU over the same rows.  Constant rows and C = 1 give beta exactly; with GELU the fp32 GELU of beta within
           (2 z^2 + 32) u |z| Phi(z) (tests/test_block_grad_gpu.py).
  top-k    no tolerance: indices equal torch.sort(attn, descending=True, stable=True) on the CPU truncated to k (NaN first), out_attn and out_feat are the
           bits of attn[idx] and feat[idx]."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import grad_parity

U = 2.0 ** -24
U64 = 2.0 ** -53
LEAD, PAD = 64, 96                      # canary elements in front of / behind every destination
CANARY32 = 0x7FC5A5A5                   # a NaN whose payload no arithmetic of these cases produces
CANARY64 = -0x5A5A5A5A5A5A5A5B          # the same idea for the int64 indices
PAD_IDX = 0x7FFFFFFF                    # topk_kernel's padding index


# ---- destinations
class Guarded:
    """A destination of `shape` inside a larger canary-filled buffer: `view` is what the kernel is given."""

    def __init__(self, shape, device, dtype=torch.float32):
        n = int(np.prod(shape)) if len(shape) else 1
        self.idt, self.canary = (torch.int32, CANARY32) if dtype == torch.float32 else (torch.int64, CANARY64)
        self.buf = torch.full((LEAD + n + PAD,), self.canary, dtype=self.idt, device=device)
        self.bits = self.buf[LEAD:LEAD + n]
        self.view = self.bits.view(dtype).view(shape)

    def fill(self, t):
        self.view.copy_(t)
        return self

    def failures(self, name):
        out = []
        if not bool((self.buf[:LEAD] == self.canary).all()):
            out.append(f"{name}: written in front of the destination")
        if not bool((self.buf[LEAD + self.bits.numel():] == self.canary).all()):
            out.append(f"{name}: written behind the destination")
        if bool((self.bits == self.canary).any()):
            out.append(f"{name}: elements of the destination not written")
        return out


def _ratio(e, bound):
    """max e / bound; an element with bound 0 must be exact; NaN anywhere -> inf"""
    r = torch.where(bound > 0, e / bound, torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def bits(t):
    return t.contiguous().view(torch.int32)


def _row_scales(M, lo=-10, hi=10):
    """2^e per row, e walking through [lo, hi] in steps of 7: rows of very different norms in every tile"""
    return torch.tensor([2.0 ** (lo + (7 * r) % (hi - lo + 1)) for r in range(M)], dtype=torch.float32)


def wave_rowsum(v):
    """[M, C] -> [M] as a wave adds a row: lane l adds columns l, l + 64, ... in order, then the 64 partial sums are added pairwise"""
    M, C = v.shape
    Cp = -(-C // 64) * 64
    p = torch.zeros((M, Cp), dtype=v.dtype)
    p[:, :C] = v
    p = p.view(M, Cp // 64, 64)
    s = torch.zeros((M, 64), dtype=v.dtype)
    for j in range(Cp // 64):
        s = s + p[:, j]
    w = 64
    while w > 1:
        w //= 2
        s = s[:, :w] + s[:, w:2 * w]
    return s[:, 0]


# =====================================================================================================================================================
# affine
AFFINE_SHAPES = [(1, 1, 1), (5, 3, 2), (63, 65, 15), (64, 64, 16), (65, 63, 17), (70, 33, 100), (129, 130, 50), (300, 96, 96)]
AFFINE_OPTS = {"none": (0, 0, 0, 0), "all": (1, 1, 1, 0), "sub": (1, 0, 0, 0), "bias": (0, 1, 0, 0), "resid": (0, 0, 1, 0), "alias": (1, 1, 1, 1)}   # sub, bias, resid, resid aliases out
AFFINE_INPUTS = ("scaled", "bigmean")
AFFINE_DEFECTS = ("drop_tail", "sub_tail", "dlayout", "acc32", "bias_after_cast", "b_stride")


def affine_cases():
    return [dict(M=M, N=N, K=K, double=d, bt=bt, opt=o, kind=kd, name=f"{'f64' if d else 'f32'}-bt{bt}-{M}x{N}x{K}-{o}-{kd}")
            for d in (1, 0) for bt in (0, 1) for (M, N, K) in AFFINE_SHAPES for o in AFFINE_OPTS for kd in AFFINE_INPUTS]


def affine_operands(case, device="cpu"):
    """A [M, K] fp32: rows scaled 2^+-10 (`scaled`) or 1000 + 1e-3 randn (`bigmean`, sub = 1000); sub [K], B and bias in the compute type; B as the kernel reads it
    ([K, N], or [N, K] with b_transposed) and `Bl`, the logical [K, N]; resid [M, N] fp32."""
    M, N, K = case["M"], case["N"], case["K"]
    td = torch.float64 if case["double"] else torch.float32
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N)
    if case["kind"] == "scaled":
        A = torch.randn((M, K), generator=g) * _row_scales(M)[:, None]
        sub = torch.randn((K,), generator=g).to(td)
    else:
        A = 1000.0 + 1e-3 * torch.randn((M, K), generator=g)
        sub = torch.full((K,), 1000.0, dtype=td)
    Bl = (torch.randn((K, N), generator=g, dtype=torch.float64) * K ** -0.5).to(td)
    bias = torch.randn((N,), generator=g, dtype=torch.float64).to(td)
    resid = torch.randn((M, N), generator=g)
    use_sub, use_bias, use_resid, alias = AFFINE_OPTS[case["opt"]]
    ops = dict(case=case, A=A, sub=sub if use_sub else None, Bl=Bl, B=(Bl.t().contiguous() if case["bt"] else Bl.contiguous()),
               bias=bias if use_bias else None, resid=resid if use_resid else None, alias=bool(alias))
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}


def affine_ref(ops):
    """(ref64, bound) [M, N] on the CPU"""
    c = ops["case"]
    A = ops["A"].cpu().double()
    if ops["sub"] is not None:
        A = A - ops["sub"].cpu().double()
    Bl = ops["Bl"].cpu().double()
    v, s = A @ Bl, A.abs() @ Bl.abs()
    if ops["bias"] is not None:
        v, s = v + ops["bias"].cpu().double(), s + ops["bias"].cpu().double().abs()
    r = ops["resid"].cpu().double() if ops["resid"] is not None else torch.zeros_like(v)
    ref = v + r
    if c["double"]:
        bound = U * v.abs() + U * ref.abs() + (c["K"] + 4) * U64 * (s + r.abs())
    else:
        bound = (c["K"] + 4) * U * (s + r.abs())
    return ref, bound


def affine_dest(ops, device):
    c = ops["case"]
    d = Guarded((c["M"], c["N"]), device)
    if ops["alias"]:
        d.fill(ops["resid"])
    return d


def affine_check(ops, dest, ref_bound=None):
    """(worst |got - ref| / bound, failures)"""
    ref, bound = ref_bound or affine_ref(ops)
    got = dest.view.cpu().double()
    r = _ratio((got - ref).abs(), bound)
    fails = dest.failures("out")
    if not r <= 1.0:
        fails.append(f"out: |got - ref| / bound = {r:.3g}")
    return r, fails


def affine_emulate(ops, dest, defect=None):
    """What gemmx_kernel writes, in the compute type on the CPU: 16-wide K tiles through zero-padded 16-row blocks, bias, the fp32 cast, the residual.
    Defects: drop_tail (the K tile of K % 16 dropped), sub_tail (sub not applied in that tile), dlayout (the other type's D-layout row formula), acc32 (the fp64 path
    accumulated in fp32), bias_after_cast, b_stride (b_transposed read with the other stride)."""
    c = ops["case"]
    M, N, K = c["M"], c["N"], c["K"]
    td = torch.float64 if c["double"] and defect != "acc32" else torch.float32
    K16, Mp = 16 * (K // 16), -(-M // 16) * 16
    A = ops["A"].cpu().to(td)
    if ops["sub"] is not None:
        sub = ops["sub"].cpu().to(td).expand(M, K).clone()
        if defect == "sub_tail":
            sub[:, K16:] = 0
        A = A - sub
    if defect == "drop_tail":
        A = A.clone()
        A[:, K16:] = 0
    Ap = torch.zeros((Mp, K), dtype=td)
    Ap[:M] = A
    Bm = ops["B"].cpu()
    if defect == "b_stride":
        Bu = Bm.reshape(-1).view(K, N) if c["bt"] else Bm.reshape(-1).view(N, K).t()
    else:
        Bu = ops["Bl"].cpu()
    Bu = Bu.to(td)
    acc = torch.zeros((Mp, N), dtype=td)
    for k0 in range(0, K, 16):
        acc = acc + Ap[:, k0:k0 + 16] @ Bu[k0:k0 + 16]
    bias = ops["bias"].cpu() if ops["bias"] is not None else None
    if bias is None:
        o = acc.float()
    elif defect == "bias_after_cast":
        o = acc.float() + bias.float()
    else:
        o = (acc + bias.to(td)).float()
    if defect == "dlayout":     # accumulator element (lane / 16 = a, r = b) holds row 4 b + a of its 16-row block (f64) or 4 a + b (f32); the other formula swaps a and b
        i = torch.arange(Mp)
        o = o[(i // 16) * 16 + 4 * (i % 4) + (i % 16) // 4]
    o = o[:M]
    if ops["resid"] is not None:
        o = o + (dest.view.cpu().clone() if ops["alias"] else ops["resid"].cpu())
    dest.view.copy_(o)


def affine_reaches(defect, case):
    """the cases in which a defect changes what is written by more than the bound allows (tests/test_retrieval_forms_host.py asserts every one of them)"""
    M, N, K = case["M"], case["N"], case["K"]
    sub, bias, resid, _ = AFFINE_OPTS[case["opt"]]
    if defect == "drop_tail":
        return K % 16 != 0
    if defect == "sub_tail":          # scaled: sub ~ randn next to a row scaled down to 2^-10; bigmean: the whole mean comes back
        return K % 16 != 0 and bool(sub)
    if defect == "dlayout":           # row 4 a + b <-> row 4 b + a of every 16-row block: row 1 shows row 4 (zeros + bias where M <= 4).  Not where the rows are all but equal
        return M > 1 and (bool(case["double"]) or bool(sub) or case["kind"] == "scaled")   # under a loose bound: fp32, 1000 + 1e-3 noise, no sub: (K + 4) u 1000 K |b| >> 1e-3 |b|
    if defect == "b_stride":          # the same memory under the other stride is another matrix unless one of its sides is 1
        return N > 1 and K > 1
    if defect == "acc32":             # fp32 sums of >= 15 terms against half an fp32 ulp of the result; it takes a few thousand elements for one to cancel enough
        return bool(case["double"]) and K >= 15 and M * N >= 4000
    if defect == "bias_after_cast":   # two more fp32 roundings (of the sum and of the bias) where the sum and the bias cancel; the fp32 path is unchanged by it.  With the residual
        return bool(case["double"]) and bool(bias) and not resid and M * N >= 4000 and case["kind"] == "scaled"   # the bound grows by u |v + r| and hides it
    raise KeyError(defect)


# =====================================================================================================================================================
# row_norm
ROWNORM_CASES = [dict(M=M, C=C, kind="scaled", name=f"M{M}-C{C}") for C in (1, 3, 63, 64, 65, 100, 1024) for M in (1, 5, 37)] + \
                [dict(M=5, C=C, kind="lastcol", name=f"M5-C{C}-lastcol") for C in (65, 100, 1024)]


def rownorm_operands(case, device="cpu"):
    M, C = case["M"], case["C"]
    g = torch.Generator().manual_seed(77 * M + C)
    x = torch.randn((M, C), generator=g) * _row_scales(M)[:, None]
    if case["kind"] == "lastcol":     # the only non-zero of every row in the last column
        x[:, :-1] = 0
    return dict(case=case, x=x.to(device))


def rownorm_ref(ops):
    ref = ops["x"].cpu().double().square().sum(1).sqrt()
    return ref, (ops["case"]["C"] / 2 + 2) * U * ref


def rownorm_emulate(ops, dest, defect=None):
    """defect drop_cols: the columns c >= 64 floor(C / 64) are not summed"""
    x = ops["x"].cpu()
    if defect == "drop_cols":
        x = x[:, :64 * (x.shape[1] // 64)]
    dest.view.copy_(torch.sqrt(wave_rowsum(x * x)) if x.shape[1] else torch.zeros(x.shape[0]))


def value_check(dest, ref, bound, name="out"):
    got = dest.view.cpu().double()
    r = _ratio((got - ref.view(got.shape)).abs(), bound.view(got.shape))
    fails = dest.failures(name)
    if not r <= 1.0:
        fails.append(f"{name}: |got - ref| / bound = {r:.3g}")
    return r, fails


# =====================================================================================================================================================
# l2_normalize
L2_CASES = [dict(outer=o, L=L, inner=i, name=f"{o}x{L}x{i}") for (o, L, i) in ((5, 65, 1), (1, 1, 1), (3, 7, 5), (2, 100, 257), (1, 3, 70000))]


def l2_operands(case, device="cpu"):
    """[outer, L, inner]; vector t = o * inner + i: t % 5 == 1 all zero, t % 5 == 3 of norm about 1e-13 (the eps branch), the others randn scaled by 2^e, e walking
    through [-40, 40] from 0 (fp32 squares stay normal)"""
    o, L, i = case["outer"], case["L"], case["inner"]
    g = torch.Generator().manual_seed(31 * L + i)
    x = torch.randn((o, L, i), generator=g)
    t = (torch.arange(o)[:, None] * i + torch.arange(i)[None, :])
    e = (t * 13 + 40) % 81 - 40
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())
    scale = torch.where(t % 5 == 1, torch.zeros_like(scale), scale)
    scale = torch.where(t % 5 == 3, torch.full_like(scale, 1e-13 / math.sqrt(L)), scale)
    x = (x.double() * scale[:, None, :]).float()
    return dict(case=case, x=x.to(device), zero=(t % 5 == 1))


def l2_ref(x):
    """F.normalize(x, dim=1) of [outer, L, inner] in fp64 -> (ref, bound)"""
    x = x.cpu().double()
    n = x.square().sum(1, keepdim=True).sqrt().clamp_min(1e-12)
    ref = x / n
    return ref, (x.shape[1] / 2 + 4) * U * ref.abs()


def l2_emulate(x, dest, defect=None):
    """inner == 1: the wave-per-row kernel (defect drop_cols as in row_norm); otherwise a thread per vector adds its squares in index order"""
    x = x.cpu()
    o, L, i = x.shape
    if i == 1:
        xs = x.view(o, L)
        if defect == "drop_cols":
            xs = xs[:, :64 * (L // 64)]
        s = wave_rowsum(xs * xs).view(o, 1, 1) if xs.shape[1] else torch.zeros((o, 1, 1))
    else:
        s = torch.zeros((o, i))
        for l in range(L):
            s = s + x[:, l] * x[:, l]
        s = s.view(o, 1, i)
    inv = 1.0 / torch.sqrt(s).clamp_min(torch.tensor(1e-12, dtype=torch.float32))
    dest.view.copy_(x * inv)


def l2_check(ops, dest, x=None):
    x = ops["x"] if x is None else x
    ref, bound = l2_ref(x)
    r, fails = value_check(dest, ref, bound)
    z = ops["zero"][:, None, :].expand(ref.shape)
    if bool(z.any()) and not bool((dest.view.cpu()[z] == 0).all()):
        fails.append("out: an all-zero vector does not give exact zeros")
    return r, fails


# =====================================================================================================================================================
# weighted_spoc
SPOC_CASES = [dict(N=N, C=C, name=f"N{N}-C{C}") for (N, C) in ((1, 4), (7, 255), (100, 257), (300, 1024))]
SPOC_IMAGES = ("ordinary", "zero weights", "norm below 1e-12")


def spoc_operands(case, device="cpu"):
    """three images: ordinary (weights |randn| over four octaves), all weights zero, weights so small that the pooled vector has norm about 1e-13"""
    N, C = case["N"], case["C"]
    g = torch.Generator().manual_seed(5 * N + C)
    feat = torch.randn((3, N, C), generator=g)
    attn = torch.randn((3, N), generator=g).abs() * torch.tensor([2.0 ** ((3 * n) % 5 - 2) for n in range(N)])
    attn[1] = 0
    attn[2] *= 1e-13 / math.sqrt(N * C)
    return dict(case=case, feat=feat.to(device), attn=attn.to(device))


def spoc_ref(ops):
    f, a = ops["feat"].cpu().double(), ops["attn"].cpu().double()
    N, C = ops["case"]["N"], ops["case"]["C"]
    p = f * a[:, :, None]
    s, t = p.sum(1), p.abs().sum(1)
    ds = (N + 1) * U * t
    n = s.square().sum(1, keepdim=True).sqrt().clamp_min(1e-12)
    ref = s / n
    return ref, ds / n + ref.abs() * ds.square().sum(1, keepdim=True).sqrt() / n + (C / 2 + 4) * U * ref.abs()


def spoc_emulate(ops, dest, defect=None):
    """fp32 sums in token order, then the wave-per-row normalisation.  Defects: drop_token (the last token), cols256 (columns >= 256 of the sums never written: the
    normalisation reads what the destination held)"""
    f, a = ops["feat"].cpu(), ops["attn"].cpu()
    Bn, N, C = f.shape
    s = torch.zeros((Bn, C))
    for n in range(N - 1 if defect == "drop_token" else N):
        s = s + f[:, n] * a[:, n, None]
    if defect == "cols256":
        s[:, 256:] = dest.view.cpu()[:, 256:]
    inv = 1.0 / torch.sqrt(wave_rowsum(s * s)).clamp_min(torch.tensor(1e-12, dtype=torch.float32))
    dest.view.copy_(s * inv[:, None])


def spoc_check(ops, dest):
    ref, bound = spoc_ref(ops)
    r, fails = value_check(dest, ref, bound)
    if not bool((dest.view.cpu()[1] == 0).all()):
        fails.append("out: zero weights do not give exact zeros")
    return r, fails


# =====================================================================================================================================================
# layernorm_act_f32
ORDINARY, BIGMEAN, CONST = range(3)
LN_KINDS = ("ordinary", "bigmean", "const")
LN_EPS = 1e-5
LN_CASES = [dict(M=M, C=C, affine=af, gelu=ge, first=fk, name=f"M{M}-C{C}-{'wb' if af else 'null'}-gelu{ge}" + (f"-k{fk}" if M < 3 else ""))
            for C in (1, 63, 64, 65, 320) for M in (1, 5, 70) for af in (1, 0) for ge in (0, 1) for fk in ((0, 1, 2) if M < 3 else (0,))]


def ln_operands(case, device="cpu"):
    """row r is of kind (r + first) % 3: ordinary randn * 3 + 0.5; bigmean 1024 s + s randn (mean = 2^10 x spread), s in {1, 2^-6, 2^6}; const 1.75 (every sum and
    the mean are exact).  With C = 1 every row is constant, whatever it holds."""
    M, C = case["M"], case["C"]
    g = torch.Generator().manual_seed(13 * M + C)
    kinds = (torch.arange(M) + case["first"]) % 3
    x = torch.randn((M, C), generator=g) * 3 + 0.5
    s = torch.tensor([2.0 ** (6 * ((r // 3) % 3 - 1)) for r in range(M)])[:, None]
    x = torch.where((kinds == BIGMEAN)[:, None], 1024.0 * s + s * torch.randn((M, C), generator=g), x)
    x = torch.where((kinds == CONST)[:, None], torch.full_like(x, 1.75), x)
    if C == 1:
        kinds = torch.full_like(kinds, CONST)
    w, b = torch.randn((C,), generator=g), torch.randn((C,), generator=g)
    return dict(case=case, x=x.to(device), kinds=kinds, w=w.to(device) if case["affine"] else None, b=b.to(device) if case["affine"] else None)


def _gelu64(z):
    return z * 0.5 * torch.erfc(-z / math.sqrt(2))


def ln_eval(ops, prec):
    x = ops["x"].cpu().to(prec)
    w = None if ops["w"] is None else ops["w"].cpu().to(prec)
    b = None if ops["b"] is None else ops["b"].cpu().to(prec)
    y = F.layer_norm(x, (x.shape[1],), w, b, LN_EPS)
    if ops["case"]["gelu"]:
        y = _gelu64(y) if prec == torch.float64 else F.gelu(y)
    return y


def ln_emulate(ops, dest, defect=None):
    """the kernel's two passes in fp32 (the second also sums the residuals and corrects the mean by theirs).  Defects: onepass (variance = E[x^2] - mean^2), mean_padded (mean and variance divided by 64 ceil(C / 64))"""
    x = ops["x"].cpu()
    M, C = x.shape
    div = torch.tensor(float(-(-C // 64) * 64 if defect == "mean_padded" else C))
    mu = (wave_rowsum(x) / div)[:, None]
    if defect == "onepass":
        var = wave_rowsum(x * x) / div - mu[:, 0] * mu[:, 0]
    else:
        d = x - mu
        dm = wave_rowsum(d) / div        # the corrected second pass: mean = mu + dm
        var = (wave_rowsum(d * d) / div - dm * dm).clamp_min(0)
        mu = None
        d = d - dm[:, None]
    rstd = (1.0 / torch.sqrt(var + torch.tensor(LN_EPS)))[:, None]
    v = (d if mu is None else x - mu) * rstd
    v = v * (ops["w"].cpu() if ops["w"] is not None else 1.0) + (ops["b"].cpu() if ops["b"] is not None else 0.0)
    if ops["case"]["gelu"]:
        v = v * (0.5 * torch.erfc(v * torch.tensor(-0.70710678118654752440)))
    dest.view.copy_(v)


def ln_reaches(defect, ops):
    """onepass: E[x^2] - mean^2 loses the variance of a row whose mean is 2^10 x its spread.  mean_padded: every C that is no multiple of 64 -- but not C = 1 under GELU,
    where the wrong row is +-8 gamma + beta and a negative one is flushed to 0 by the activation, which is what a constant row without beta gives anyway."""
    c = ops["case"]
    if defect == "onepass":
        return c["C"] > 1 and bool((ops["kinds"] == BIGMEAN).any())
    if defect == "mean_padded":
        return c["C"] % 64 != 0 and not (c["C"] == 1 and c["gelu"])
    raise KeyError(defect)


def ln_check(ops, dest, rows=None, tag=""):
    """grad_parity.compare per row kind (its rows go to `rows`), then the exact relations of the constant rows.  Returns the failures."""
    c = ops["case"]
    fails = dest.failures("out")
    got = dest.view.cpu()
    y64, y32 = ln_eval(ops, torch.float64), ln_eval(ops, torch.float32)
    rows = [] if rows is None else rows
    for k, kn in enumerate(LN_KINDS):
        m = ops["kinds"] == k
        if not bool(m.any()):
            continue
        try:
            grad_parity.compare(rows, tag or c["name"], {kn: got[m]}, {kn: y64[m]}, {kn: y32[m]})
        except AssertionError as e:
            fails.append(f"{kn}: {str(e)[:200]}")
    m = ops["kinds"] == CONST
    if bool(m.any()):
        beta = ops["b"].cpu() if ops["b"] is not None else torch.zeros(c["C"])
        beta = beta.expand(int(m.sum()), c["C"])
        if not c["gelu"]:
            if not torch.equal(bits(got[m]), bits(beta)):
                fails.append("const: out != beta bit for bit")
        else:
            z = beta.double()
            want = _gelu64(z)
            r = _ratio((got[m].double() - want).abs(), (2 * z * z + 32) * U * want.abs())
            if not r <= 1.0:
                fails.append(f"const: |out - gelu(beta)| / ((2 z^2 + 32) u |z| Phi(z)) = {r:.3g}")
    return fails


# =====================================================================================================================================================
# top-k
TOPK_N = (1, 2, 3, 63, 64, 65, 100, 768, 1000, 4095, 4096)
TOPK_C = (4, 12, 64)
TOPK_IMAGES = (1, 3)
TOPK_KEYS = ("distinct", "quant", "equal", "inf")
TOPK_NAN_KEYS = ("nan1", "nan3", "nanfrac", "nanall")       # only ever run on the kernel with the total order


def topk_ks(N):
    return sorted({1, N // 2 + 1, N})


def topk_keys(kind, Bn, N, seed=0):
    """[Bn, N] fp32 keys.  distinct: a permutation of N equally spaced values around 0; quant: 4 values (heavy ties); equal: one value; inf: distinct with +inf and -inf
    at the ends (and at 1 and N / 2 from N = 5); nan1 / nan3: distinct with that many NaNs; nanfrac: quant with N // 10 + 1 NaNs; nanall."""
    g = torch.Generator().manual_seed(97 * N + 7 * Bn + seed)
    out = torch.empty((Bn, N))
    for b in range(Bn):
        distinct = (torch.randperm(N, generator=g).float() - N // 2) * 0.375
        quant = torch.randint(0, 4, (N,), generator=g).float() - 1.5
        if kind in ("distinct", "inf", "nan1", "nan3"):
            k = distinct
        elif kind in ("quant", "nanfrac"):
            k = quant
        else:
            k = torch.full((N,), 0.75)
        if kind == "inf":
            k[0] = -math.inf
            if N >= 2:
                k[N - 1] = math.inf
            if N >= 5:
                k[1], k[N // 2] = math.inf, -math.inf
        cnt = {"nan1": 1, "nan3": 3, "nanfrac": N // 10 + 1, "nanall": N}.get(kind, 0)
        if cnt:
            k[torch.randperm(N, generator=g)[:min(cnt, N)]] = math.nan
        out[b] = k
    return out


def topk_feat(Bn, N, C, device="cpu"):
    """[Bn, N, C]: every element names its place, so a row gathered from anywhere else cannot pass"""
    return torch.arange(Bn * N * C, dtype=torch.float32, device=device).view(Bn, N, C) * 0.5 + 1.0


def cmp_old(ka, kb, ia, ib):
    """the comparator before the fix: not an order once a key is NaN"""
    return (ka > kb) | ((ka == kb) & (ia < ib))


def cmp_total(ka, kb, ia, ib):
    """NaN first, then descending, ties (and NaNs among themselves) by lower index: a total order"""
    na, nb = ka != ka, kb != kb
    return (na & ~nb) | ((na == nb) & ((ka > kb) | (((ka == kb) | na) & (ia < ib))))


def cmp_high(ka, kb, ia, ib):
    """the total order with ties by HIGHER index"""
    na, nb = ka != ka, kb != kb
    return (na & ~nb) | ((na == nb) & ((ka > kb) | (((ka == kb) | na) & (ia > ib))))


def bitonic(keys, comparator=cmp_total, pad_key=-math.inf):
    """topk_kernel's network on one image's keys (numpy fp32 [N]): P, lo / hi / desc exactly as in the kernel -> (keys [P], indices [P]) after the last stage"""
    N = len(keys)
    P = 1
    while P < N:
        P <<= 1
    key = np.full((P,), pad_key, dtype=np.float32)
    key[:N] = keys
    idx = np.full((P,), PAD_IDX, dtype=np.int64)
    idx[:N] = np.arange(N)
    i = np.arange(P // 2)
    size = 2
    with np.errstate(invalid="ignore"):
        while size <= P:
            stride = size >> 1
            while stride > 0:
                lo = 2 * i - (i & (stride - 1))
                hi = lo + stride
                desc = (lo & size) == 0
                ka, kb, ia, ib = key[lo], key[hi], idx[lo], idx[hi]
                swap = comparator(ka, kb, ia, ib) != desc
                key[lo], key[hi] = np.where(swap, kb, ka), np.where(swap, ka, kb)
                idx[lo], idx[hi] = np.where(swap, ib, ia), np.where(swap, ia, ib)
                stride >>= 1
            size <<= 1
    return key, idx


def topk_dests(Bn, k, C, device):
    return dict(feat=Guarded((Bn, k, C), device), attn=Guarded((Bn, k), device), idx=Guarded((Bn, k), device, torch.int64))


def topk_network(attn, comparator=cmp_total, pad_key=-math.inf):
    """the sorted (keys, indices) of every image: depends on neither k nor C"""
    a = attn.cpu().numpy()
    return [bitonic(a[b], comparator, pad_key) for b in range(a.shape[0])]


def topk_emulate(feat, attn, k, dests, comparator=cmp_total, pad_key=-math.inf, net=None):
    """what topk_kernel writes with that comparator and padding key; a row gathered from outside the tensor is emulated as zeros"""
    Bn, N, C = feat.shape
    net = net or topk_network(attn, comparator, pad_key)
    for b in range(Bn):
        key, idx = net[b]
        ix = torch.from_numpy(idx[:k].copy())
        dests["idx"].view[b] = ix
        dests["attn"].view[b] = torch.from_numpy(key[:k].copy())
        inside = ix < N
        dests["feat"].view[b] = torch.where(inside[:, None], feat[b].cpu()[ix.clamp_max(N - 1)], torch.zeros(()))


def topk_expected(attn, k):
    """the contract: a stable descending sort on the CPU, NaN first"""
    return torch.sort(attn.cpu(), dim=1, descending=True, stable=True).indices[:, :k]


def topk_check(feat, attn, k, dests):
    """failures; no tolerance anywhere"""
    fails = []
    for n, d in dests.items():
        fails += d.failures(n)
    dev = dests["idx"].view.device
    want = topk_expected(attn, k).to(dev)
    got = dests["idx"].view
    if not torch.equal(got, want):
        fails.append(f"idx: {int((got != want).sum())} of {want.numel()} indices differ from the stable descending sort")
        return fails
    if not torch.equal(bits(dests["attn"].view), bits(torch.gather(attn, 1, want))):
        fails.append("attn: not the bits of attn[idx]")
    if not torch.equal(bits(dests["feat"].view), bits(torch.gather(feat, 1, want[:, :, None].expand(-1, -1, feat.shape[2])))):
        fails.append("feat: not the bits of the gathered rows")
    return fails


def _same_key(a):
    """[N, N] bool: keys that tie (equal, or both NaN)"""
    return (a[:, None] == a[None, :]) | (torch.isnan(a)[:, None] & torch.isnan(a)[None, :])


def topk_reaches(defect, attn, k):
    """does the defect change the first k of some image?  From the keys alone, not from any emulation.
    high_index: one of the first k of the stable order has a tie partner of higher index (the padding is one, for a real -inf, when N is no power of two).  pad_zero: N is no power of two and fewer than k keys rank before (0, padding),
    i.e. are NaN or >= 0.  old_cmp: see the host file (a NaN key is the condition; whether the network then misorders is a property of the data)."""
    a = attn.cpu()
    Bn, N = a.shape
    if defect == "high_index":
        for b in range(Bn):
            first = topk_expected(a[b:b + 1], k)[0]
            tie = _same_key(a[b])
            if bool((tie[first] & (torch.arange(N)[None, :] > first[:, None])).any()):
                return True
            if (N & (N - 1)) != 0 and bool((a[b][first] == -math.inf).any()):
                return True
        return False
    if defect == "pad_zero":
        return (N & (N - 1)) != 0 and bool(((torch.isnan(a) | (a >= 0)).sum(1) < k).any())
    raise KeyError(defect)
