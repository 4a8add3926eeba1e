"""Shared by tests/test_lnfold_forms_gpu.py (every GEMM launch form of the LN fold of a one-view update, through must3r_hip_op_gemm_lnfold_ex, against fp64) and
tests/test_lnfold_forms_host.py (the checks discriminate): the dispatch restated, the case table, the row kinds, the operands, the fp64 reference, the bounds, the
canary-filled destinations, the checks, an fp32 emulation of what the kernels write (with the defects the host file plants), and the chain of three decoder blocks
driven through a back end (the GPU entry point, or the emulation).  Nothing here needs a GPU.

The fold (csrc/model.hip decode_impl, `lnf`): a residual GEMM ("producer") stores the new fp32 rows x, their copy, y = x - shift[m] rounded to fp16 (x16) and the
(sum, sum of squares) of y per 16-column fragment; the Linear that follows ("consumer") computes epi(rstd (x16 W'^T - mu s) + c) with W' = gamma (.) W, s_n = sum_k W'_nk,
c = W beta + b, (mu, rstd) of y from the fragment sums, and leaves shift + mu = the row mean for the next producer.

Forms (call sites): producers embed (EPI_F32, plain weights, bias2, no shift, copy32), proj (EPI_RESID_F32, split, shift), fc2 (split and plain, K = 3072, shift, copy32),
fc2_last (no fold outputs: the default dispatch); consumers qkv (EPI_QKV_ROPE, split; `first`: ln_shift_init = 1 on unshifted rows, block 0's qkv), projq (EPI_STORE16,
split, scale), fc1 (EPI_STORE16_GELU, split and plain).  M in {12, 196, 700, 768, 1024}: 196 leaves 4 rows in the last 48- / 64- / 96-row tile, 700 leaves 28 / 60 / 28,
768 none, 1024 leaves 16 / 0 / 64.

Row kinds (kind = m % 13, so every tile holds several): benign rows with an exact and with a stale shift; a common offset of 10 and of 40 sigma with an exact shift, a
shift 5 % off, and none; two token-constant massive channels (3e3); three token-dependent ones (x 300); sigma = 1e-3 around 5; a constant row; a row with |y| > 65504.

Consumer reference: fp64 epi(LN0(x) W'^T + c) over the fp32 rows x and the weights the kernel multiplies (W_hi + W_lo, or the fp16 W'); s and c as finalize_weights derives
them (fp64 sums of the fp32 W').  Bound, per element (u = 2^-11):
    |out - ref| <= C_R u |ref| + g(C_A u kappa_m ||W'_n||_2 + C_V 2^-24 kappa_m^2 |pre - c_n|)
pre = the value in front of the epilogue, kappa_m = sqrt(1 + mean(y_m)^2 / (var(y_m) + eps)) in fp64 from the rows the consumer reads (y = x - shift), g = the epilogue's
Lipschitz factor on an error of pre: 1, GELU_SLOPE, the RoPE pair norm sqrt(B_n^2 + B_partner^2), and out_scale on the scaled columns.  The first term is the rounding of
the stored value, the second the fp16 rounding of y (and of a plain W' against s) that the product amplifies by kappa, the third the cancellation in E[y^2] - mu^2.
C_R, C_V = 1 (their floor: one rounding of the output is u/2 = half of C_R = 1), C_A = 16 = the smallest power of two for which the emulation below stays at ratio <= 0.5 on
every case (tests/test_lnfold_forms_host.py asserts that, and that C_A / 2 does not: the rows with three token-dependent massive channels set it -- their rounding error
sits in three terms of the product and does not average; the benign and the offset rows alone would take C_A = 8).  On rows with kappa <= 2 the bound stays inside twice
the unfolded 16-bit bounds of gemm_forms.py (2u / 2u, with RoPE 2u / 4u): the weights are drawn at W_SCALE / sqrt(K) for that, and the host file asserts it.  Rows with
kappa > 300 are outside any contract: finite, and row-wise inside the kappa^2 term, max_n |out - ref| <= g C_V_OUT 2^-24 kappa^2 max_n ||W'_n||_2 (||W'_n||_2 = the scale
of |pre - c_n|, which itself is 0 on a constant row; C_V_OUT = 8 by the same rule).  The saturated row (its x16 no longer holds x) must be finite.
Producer bounds: out against fp64 1e-5 / 1e-4 (plain) and 2e-6 / 8e-6 (split) as in gemm_forms.py; copy32 == out and x16 == fp16_sat(out - shift) bit for bit; each
fragment sum against the fp64 sum of the fp32 terms within (n - 1) 2^-24 sum |term|, n = 16 (squares: n, their products are rounded too)."""
import math

import torch

import gemm_forms as G

D = 768
SLOTS = D // 16
U = 2.0 ** -11
U32 = 2.0 ** -24
EPS = 1e-6
W_SCALE = 0.125
GELU_SLOPE = 1.13          # max |gelu'| = 1.1290
C_R, C_A, C_V = 1.0, 16.0, 1.0
C_V_OUT = 8.0              # rows with kappa > 300: the row-wise kappa^2 check (the product's kappa term is not in it)
KAPPA_CONTRACT = 300.0
EPI_STORE16, EPI_STORE16_GELU, EPI_QKV_ROPE, EPI_RESID_F32, EPI_F32 = G.EPI_STORE16, G.EPI_STORE16_GELU, G.EPI_QKV_ROPE, G.EPI_RESID_F32, G.EPI_F32
LEAD, PAD = 2, 3           # canary rows in front of and behind every destination
MS = (12, 196, 700, 768, 1024)
KINDS = ("benign_exact", "benign_stale", "off10_exact", "off10_5pct", "off10_none", "off40_exact", "off40_5pct", "off40_none", "massive_const", "massive_token",
         "tiny_sigma", "constant", "saturate")
NK = len(KINDS)
BIG_CH, TOK_CH, SAT_CH = (3, 90), (5, 77, 200), 7


# ---- csrc/gemm_route.hpp gemm_route restated for the fold's launches (default options; bk128: M3R_BK128); tests/test_gemm_route_host.py holds both against the rule
def consumer_kernel(epi, weights, bk128=1):
    if weights == "plain":
        return f"g64/e{epi}/w1/n64"
    if epi == EPI_STORE16_GELU:
        return f"g96/e{epi}/w2/n96"
    if epi == EPI_STORE16:
        return f"{'g48k128' if bk128 else 'g48'}/e{epi}/w2/n48"
    return f"g64/e{epi}/w2/n64"


def producer_kernel(epi, M, K, weights, fold_outputs=True):
    """a launch with x16_out / copy32_out / stats_out never takes the 256-row, g128 or sparse kernels (`lnp`); N = 768"""
    ws = 1 if weights == "plain" else 2
    if not fold_outputs:
        return G.dispatch(epi, M, D, K, 0 if weights == "plain" else 2)
    t96 = ((M + 95) // 96) * (D // 96)
    t48 = ((M + 47) // 48) * (D // 48)
    if ws == 2 and 224 <= t96 <= 256:
        return f"g96/e{epi}/w2/n96"
    if 192 <= t48 <= 256:
        return f"{'g48k128' if K % 128 == 0 and K >= 256 else 'g48'}/e{epi}/w{ws}/n48"
    return f"{'g64p' if ((M + 63) // 64) * (D // 64) <= 256 else 'g64'}/e{epi}/w{ws}/n64"


# ---- the case tables
def _pcases():
    out = []
    for M in MS:
        for K in (256, 1024):
            out.append(dict(role="producer", form="embed", name=f"embed-K{K}-M{M}", epi=EPI_F32, weights="plain", K=K, M=M, shift=False, copy=True, fold=True, bias2=True))
        out.append(dict(role="producer", form="proj", name=f"proj-split-M{M}", epi=EPI_RESID_F32, weights="split", K=D, M=M, shift=True, copy=False, fold=True, bias2=False))
        for w in ("split", "plain"):
            out.append(dict(role="producer", form="fc2", name=f"fc2-{w}-M{M}", epi=EPI_RESID_F32, weights=w, K=3072, M=M, shift=True, copy=True, fold=True, bias2=False))
            out.append(dict(role="producer", form="fc2_last", name=f"fc2_last-{w}-M{M}", epi=EPI_RESID_F32, weights=w, K=3072, M=M, shift=False, copy=False, fold=False,
                            bias2=False))
    return out


def _ccases():
    out = []
    for M in MS:
        for first in (1, 0):
            out.append(dict(role="consumer", form="qkv", name=f"qkv-split-M{M}" + ("-first" if first else ""), epi=EPI_QKV_ROPE, weights="split", N=3 * D, M=M, init=first,
                            rope_cols=2 * D, scale_cols=D))
        out.append(dict(role="consumer", form="projq", name=f"projq-split-M{M}", epi=EPI_STORE16, weights="split", N=D, M=M, init=0, rope_cols=0, scale_cols=D))
        for w in ("split", "plain"):
            out.append(dict(role="consumer", form="fc1", name=f"fc1-{w}-M{M}", epi=EPI_STORE16_GELU, weights=w, N=4 * D, M=M, init=0, rope_cols=0, scale_cols=0))
    return out


PCASES, CCASES = _pcases(), _ccases()
CASE = {c["name"]: c for c in PCASES + CCASES}
assert len(CASE) == len(PCASES) + len(CCASES)


def kernel_of(case):
    if case["role"] == "consumer":
        return consumer_kernel(case["epi"], case["weights"])
    return producer_kernel(case["epi"], case["M"], case["K"], case["weights"], case["fold"])


# ---- rows of every kind: kind of row m = KINDS[m % NK]
def make_rows(M, seed, unshifted=False):
    """x fp32 [M, 768] and shift fp32 [M], row m of kind KINDS[m % NK].  unshifted: every shift 0 (the rows of the embed producer, which has none)"""
    g = torch.Generator().manual_seed(4001 + seed)
    z = torch.randn((M, D), generator=g)
    s = 1.0 + 3.0 * torch.rand((M, 1), generator=g)
    x = s * z + 0.7 * torch.randn((M, 1), generator=g)
    stale = 0.2 * s[:, 0] * torch.randn((M,), generator=g)
    tok = 300.0 * torch.randn((M, len(TOK_CH)), generator=g)
    k = torch.arange(M) % NK
    K = {n: i for i, n in enumerate(KINDS)}
    for name, off in (("off10", 10.0), ("off40", 40.0)):
        sel = (k == K[name + "_exact"]) | (k == K[name + "_5pct"]) | (k == K[name + "_none"])
        x[sel] = (s * z + off * s)[sel]
    sel = k == K["massive_const"]
    x[sel] = z[sel]
    for ch in BIG_CH:
        x[sel, ch] = 3.0e3
    sel = k == K["massive_token"]
    x[sel] = z[sel]
    for i, ch in enumerate(TOK_CH):
        x[sel, ch] = tok[sel, i]
    sel = k == K["tiny_sigma"]
    x[sel] = 5.0 + 1.0e-3 * z[sel]
    x[k == K["constant"]] = 5.0
    sel = k == K["saturate"]
    x[sel] = z[sel]
    x[sel, SAT_CH] = 1.0e5
    mean = x.double().mean(1).float()
    shift = mean.clone()
    shift[k == K["benign_stale"]] += stale[k == K["benign_stale"]]
    for name in ("off10", "off40"):
        shift[k == K[name + "_5pct"]] *= 0.95
        shift[k == K[name + "_none"]] = 0.0
    if unshifted:
        shift = torch.zeros_like(shift)
    return x.contiguous(), shift.contiguous()


def fragment_sums(y):
    """what ln_fold_emit leaves: (sum, sum of squares) of the fp32 y per 16-column fragment, in fp32 -- a lane adds its 4 columns pairwise, the 4 lanes of a row's
    fragment (columns 4 fg ..) are added pairwise (quad_row_sum)"""
    M = y.shape[0]
    y = y.float().view(M, -1, 4, 4)
    a = (y[..., 0] + y[..., 1]) + (y[..., 2] + y[..., 3])
    q = (y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1]) + (y[..., 2] * y[..., 2] + y[..., 3] * y[..., 3])
    s1 = (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
    s2 = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    return torch.stack((s1, s2), -1).contiguous()


def round16(v):
    return G.round16(v, "fp16")


def kappa(y):
    """sqrt(1 + mean^2 / (var + eps)) of the rows y the consumer reads, in fp64"""
    y = y.double()
    m = y.mean(1)
    return torch.sqrt(1.0 + m * m / (y.var(1, unbiased=False) + EPS))


def _weights(Wf, weights):
    """W as the kernel takes it, and the parts it multiplies (hi before lo)"""
    if weights == "plain":
        w = Wf.half().contiguous()
        return w, (w,)
    hi = Wf.half()
    lo = (Wf - hi.float()).half()
    return torch.cat((hi, lo), dim=1).contiguous(), (hi, lo)


def _matmul(a, parts, prec):
    v = None
    for p in parts:
        t = a.to(prec) @ p.to(prec).t()
        v = t if v is None else v + t
    return v


# ---- producers
def make_producer(case, device="cpu", seed=0):
    M, K = case["M"], case["K"]
    g = torch.Generator().manual_seed(7001 + seed + 13 * M + K)
    A = torch.randn((M, K), generator=g).half()
    Wf = torch.randn((D, K), generator=g) / math.sqrt(K)
    bias = torch.round(torch.randn((D,), generator=g) * 1024.0) / 1024.0       # multiples of 2^-10: the constant row comes out exactly constant
    ops = dict(case=case, kernel=kernel_of(case), bias2=None, x_old=None, shift=None)
    if case["form"] == "embed":
        if K == 256:
            bias[SAT_CH] = 1.0e5       # every row beyond the fp16 range in one column
        ops["bias2"] = torch.randn((D,), generator=g)
        A = (A.float() * (0.25 + 2.0 * torch.rand((M, 1), generator=g))).half()
    W, parts = _weights(Wf, case["weights"])
    if case["epi"] == EPI_RESID_F32:
        x, shift = make_rows(M, seed + K)
        A[torch.arange(M) % NK == KINDS.index("constant")] = 0
        lin = _matmul(A, parts, torch.float64) + bias.double()
        ops["x_old"] = (x.double() - lin).float()
        if case["shift"]:
            ops["shift"] = shift
    ops.update(A=A.contiguous(), W=W, parts=parts, bias=bias)
    for k_, v in list(ops.items()):
        if isinstance(v, torch.Tensor):
            ops[k_] = v.to(device)
    ops["parts"] = tuple(p.to(device) for p in parts)
    return ops


def alloc_producer(ops, device="cpu"):
    """every destination inside a canary-filled buffer; out holds the old residual rows (EPI_RESID_F32)"""
    case = ops["case"]
    M, rows = case["M"], LEAD + case["M"] + PAD
    nan = float("nan")
    outs = dict(out=torch.full((rows, D), nan, device=device))
    if ops["x_old"] is not None:
        outs["out"][LEAD:LEAD + M] = ops["x_old"]
    if case["fold"]:
        outs["x16"] = torch.full((rows, D), G.CANARY16, dtype=torch.int16, device=device)
        outs["stats"] = torch.full((rows, SLOTS, 2), nan, device=device)
        if case["copy"]:
            outs["copy"] = torch.full((rows, D), nan, device=device)
    if ops["shift"] is not None:
        outs["shift"] = torch.full((rows,), nan, device=device)
        outs["shift"][LEAD:LEAD + M] = ops["shift"]
    return outs


def producer_op(ops, outs):
    """the launch: what the entry point (or the emulation) is given.  Destinations are windows of the canary-filled buffers."""
    case = ops["case"]
    M = case["M"]

    def win(k):
        return outs[k][LEAD:LEAD + M] if k in outs else None
    return dict(role="producer", epi=case["epi"], M=M, N=D, K=case["K"], A=ops["A"], W=ops["W"], parts=ops["parts"], wsplit=0 if case["weights"] == "plain" else 2,
                bias=ops["bias"], bias2=ops["bias2"], row_start2=0, out=win("out"), x16=win("x16"), copy=win("copy"), stats=win("stats"), shift=win("shift"))


def emulate_producer(op, prec=torch.float32, x16_unshifted=False):
    """what a producer launch writes, in fp32.  Defect: x16 rounded from x where x - shift belongs"""
    v = _matmul(op["A"], op["parts"], prec) + op["bias"].to(prec)
    if op["bias2"] is not None:
        rows = torch.arange(op["M"], device=v.device)
        v = v + (rows >= op["row_start2"]).to(prec)[:, None] * op["bias2"].to(prec)
    x = (op["out"].to(prec) + v if op["epi"] == EPI_RESID_F32 else v).float()
    op["out"][:] = x
    if op["copy"] is not None:
        op["copy"][:] = x
    sh = op["shift"][:, None] if op["shift"] is not None else 0.0
    y = x - sh
    if op["x16"] is not None:
        op["x16"][:] = round16(x if x16_unshifted else y).view(torch.int16)
    if op["stats"] is not None:
        op["stats"][:] = fragment_sums(y)


def producer_bound(case):
    return (1e-5, 1e-4) if case["weights"] == "plain" else (2e-6, 8e-6)


def _nan_outside(buf, M):
    return bool(torch.isnan(buf[:LEAD]).all()) and bool(torch.isnan(buf[LEAD + M:]).all())


def check_producer(ops, outs, strict=True):
    """raises AssertionError with the relation that failed (strict = False: the exact relations only, the ratios are reported); returns dict(err: out against fp64 as a ratio of the bound, s1 / s2: the fragment sums as ratios of theirs)"""
    case = ops["case"]
    M = case["M"]
    out = outs["out"][LEAD:LEAD + M]
    assert _nan_outside(outs["out"], M), "canaries around out overwritten"
    assert bool(torch.isfinite(out).all()), "out: elements not written, or not finite"
    ref = _matmul(ops["A"], ops["parts"], torch.float64) + ops["bias"].double()
    if ops["bias2"] is not None:
        ref = ref + ops["bias2"].double()
    if ops["x_old"] is not None:
        ref = ref + ops["x_old"].double()
    rtol, atol = producer_bound(case)
    rep = dict(err=G.ratio(out, ref, rtol, atol), rtol=rtol, atol=atol, s1=0.0, s2=0.0)
    assert not strict or rep["err"] <= 1.0, ("out against fp64", rep)
    if "shift" in outs:
        sh = outs["shift"]
        assert _nan_outside(sh, M) and torch.equal(sh[LEAD:LEAD + M], ops["shift"]), "a producer must not write ln_shift"
    if not case["fold"]:
        return rep
    if "copy" in outs:
        assert _nan_outside(outs["copy"], M), "canaries around copy32 overwritten"
        assert torch.equal(outs["copy"][LEAD:LEAD + M].view(torch.int32), out.view(torch.int32)), "copy32 != out"
    y = out - (ops["shift"][:, None] if ops["shift"] is not None else 0.0)
    x16 = outs["x16"]
    assert bool((x16[:LEAD] == G.CANARY16).all()) and bool((x16[LEAD + M:] == G.CANARY16).all()), "canaries around x16 overwritten"
    assert torch.equal(x16[LEAD:LEAD + M], round16(y).view(torch.int16)), "x16 != fp16_sat(out - shift)"
    st = outs["stats"]
    assert _nan_outside(st, M), "canaries around the fragment sums overwritten"
    st = st[LEAD:LEAD + M].double()
    assert bool(torch.isfinite(st).all()), "fragment sums not written"
    fr = y.double().view(M, SLOTS, 16)
    a1, a2 = fr.abs().sum(-1), (fr * fr).sum(-1)
    tiny = 1e-30
    rep["s1"] = float(((st[..., 0] - fr.sum(-1)).abs() / (15 * U32 * a1 + tiny)).max())
    rep["s2"] = float(((st[..., 1] - a2).abs() / (16 * U32 * a2 + tiny)).max())
    assert not strict or (rep["s1"] <= 1.0 and rep["s2"] <= 1.0), ("fragment sums against fp64", rep)
    return rep


# ---- consumers
def positions(M):
    m = torch.arange(M)
    return torch.stack(((m // 32) % G.NPOS, m % 32), -1).contiguous()


def fold_weights(Wf, gam, bet, b, weights):
    """the derived operands of finalize_weights (csrc/model.hip derive_ln_fold): W' = gamma (.) W in fp32, s and c from fp64 sums"""
    Wg = (Wf * gam).float()
    s_n = Wg.double().sum(1).float()
    c_n = (Wf.double() @ bet.double() + b.double()).float()
    W, parts = _weights(Wg, weights)
    return W, parts, s_n, c_n


def make_consumer(case, device="cpu", seed=0):
    """the rows a producer left (x, shift -> x16 and fragment sums, by the emulation of the producer's epilogue) and the consumer's own operands"""
    M, N = case["M"], case["N"]
    g = torch.Generator().manual_seed(9001 + seed + 13 * M + N)
    x, shift = make_rows(M, seed + N, unshifted=bool(case["init"]))
    y = x - shift[:, None]
    Wf = torch.randn((N, D), generator=g) * (W_SCALE / math.sqrt(D))
    gam = 1.0 + 0.3 * torch.randn((D,), generator=g)
    bet = 0.2 * torch.randn((D,), generator=g)
    b = W_SCALE * torch.randn((N,), generator=g)
    W, parts, s_n, c_n = fold_weights(Wf, gam, bet, b, case["weights"])
    ops = dict(case=case, kernel=kernel_of(case), x=x, shift=shift, y=y, x16=round16(y).contiguous(), stats=fragment_sums(y), W=W, s_n=s_n, c_n=c_n,
               pos=positions(M) if case["epi"] == EPI_QKV_ROPE else None)
    for k_, v in list(ops.items()):
        if isinstance(v, torch.Tensor):
            ops[k_] = v.to(device)
    ops["parts"] = tuple(p.to(device) for p in parts)
    return ops


def alloc_consumer(ops, device="cpu"):
    case = ops["case"]
    M, rows = case["M"], LEAD + case["M"] + PAD
    outs = dict(out=torch.full((rows, case["N"]), G.CANARY16, dtype=torch.int16, device=device), shift=torch.full((rows,), float("nan"), device=device))
    if not case["init"]:
        outs["shift"][LEAD:LEAD + M] = ops["shift"]      # (init: the buffer holds nothing -- NaN)
    return outs


def consumer_op(ops, outs):
    case = ops["case"]
    M = case["M"]
    return dict(role="consumer", epi=case["epi"], M=M, N=case["N"], K=D, A=ops["x16"], stats=ops["stats"], W=ops["W"], parts=ops["parts"],
                wsplit=0 if case["weights"] == "plain" else 2, s_n=ops["s_n"], bias=ops["c_n"], eps=EPS, shift=outs["shift"][LEAD:LEAD + M], init=case["init"],
                pos=ops["pos"], rope_cols=case["rope_cols"], scale_cols=case["scale_cols"], out=outs["out"][LEAD:LEAD + M])


def epilogue(v, epi, pos, rope_cols, scale_cols):
    """the epilogue's arithmetic on the value in front of it, in v's precision, before the rounding to fp16"""
    if epi == EPI_QKV_ROPE:
        v = G._rope(v, pos, rope_cols)
    if scale_cols > 0:
        v = torch.cat((v[:, :scale_cols] * G.OUT_SCALE, v[:, scale_cols:]), dim=1)
    if epi == EPI_STORE16_GELU:
        v = torch.nn.functional.gelu(v)
    return v


def row_stats(stats, eps, frags=SLOTS, no_eps=False):
    """(mu, rstd) as ln_fold_rows computes them from the fragment sums: 12 threads of a row add 4 fragments each in order, one adds the 12 partial sums in order
    (gemm48; the other tiles split 8 x 6, 4 x 12: the same bound); E[y^2] - mu^2 clamped at 0.  Defects: frags < 48 fragments; eps dropped"""
    st = stats.float().clone()
    st[:, frags:] = 0.0
    st = st.view(st.shape[0], 12, 4, 2)
    part = torch.zeros_like(st[:, :, 0])
    for i in range(4):
        part = part + st[:, :, i]
    tot = torch.zeros_like(part[:, 0])
    for t in range(12):
        tot = tot + part[:, t]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(D), dtype=torch.float32)
    mu = tot[:, 0] * inv
    var = (tot[:, 1] * inv - mu * mu).clamp_min(0.0)
    return mu, torch.rsqrt(var + (0.0 if no_eps else eps))


def emulate_consumer(op, prec=torch.float32, frags47=False, tail_stats=0, drop_s_tile=False, shift_twice=False, ignore_init=False, no_eps=False):
    """what a consumer launch writes.  Defects: frags47: mu and the variance from 47 of the 48 fragments; tail_stats = BM: the rows of the last (ragged) BM-row tile all
    read row M - 1's statistics; drop_s_tile: s_n = 0 in the second 64-column tile; shift_twice: a second column block adds mu to ln_shift again; ignore_init:
    ln_shift_init treated as 0; no_eps: rstd = 1 / sqrt(var)"""
    M = op["M"]
    mu, rstd = row_stats(op["stats"], op["eps"], 47 if frags47 else SLOTS, no_eps)
    if tail_stats and M % tail_stats:
        t0 = M // tail_stats * tail_stats
        mu[t0:], rstd[t0:] = mu[M - 1].clone(), rstd[M - 1].clone()
    s_n = op["s_n"].clone()
    if drop_s_tile:
        s_n[64:128] = 0.0
    acc = _matmul(op["A"], op["parts"], prec)
    v = (acc - s_n.to(prec) * mu.to(prec)[:, None]) * rstd.to(prec)[:, None] + op["bias"].to(prec)
    v = epilogue(v, op["epi"], op["pos"], op["rope_cols"], op["scale_cols"]).float()
    op["out"][:] = round16(v).view(torch.int16)
    old = op["shift"].clone() if (not op["init"] or ignore_init) else torch.zeros_like(op["shift"])
    op["shift"][:] = old + mu * (2.0 if shift_twice else 1.0)


def _partner(n_cols, rope_cols, device):
    n = torch.arange(n_cols, device=device)
    p = torch.where(n % 32 < 16, n + 16, n - 16)
    return torch.where(n < rope_cols, p, n)


def consumer_reference(ops):
    """dict(ref: fp64 epi(LN0(x) W'^T + c), bound: the per-element bound, kappa [M], rowterm: the row-wise kappa^2 term of rows outside the contract)"""
    case = ops["case"]
    x = ops["x"].double()
    ln0 = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + EPS)
    w = sum(p.double() for p in ops["parts"])
    lin = ln0 @ w.t()
    pre = lin + ops["c_n"].double()
    ref = epilogue(pre, case["epi"], ops["pos"], case["rope_cols"], case["scale_cols"])
    kap = kappa(ops["y"])
    b_pre = C_A * U * kap[:, None] * w.norm(dim=1)[None, :] + C_V * U32 * (kap * kap)[:, None] * lin.abs()
    gmax = 1.0
    if case["epi"] == EPI_QKV_ROPE:
        bp = b_pre[:, _partner(case["N"], case["rope_cols"], b_pre.device)]
        rot = torch.arange(case["N"], device=b_pre.device) < case["rope_cols"]
        b_pre = torch.where(rot[None, :], torch.sqrt(b_pre * b_pre + bp * bp), b_pre)
        gmax = math.sqrt(2.0)
    if case["scale_cols"] > 0:
        b_pre = torch.cat((b_pre[:, :case["scale_cols"]] * G.OUT_SCALE, b_pre[:, case["scale_cols"]:]), dim=1)
    if case["epi"] == EPI_STORE16_GELU:
        b_pre = b_pre * GELU_SLOPE
        gmax = GELU_SLOPE
    rowterm = gmax * U32 * kap * kap * w.norm(dim=1).max()
    return dict(ref=ref, bound=C_R * U * ref.abs() + b_pre, kappa=kap, rowterm=rowterm)


def unfolded_bound(case, ref):
    """twice the 16-bit bounds of gemm_forms.py for the unfolded launch: 2 (atol + rtol |ref|), 2u / 2u, with RoPE 2u / 4u"""
    return 2.0 * ((4 * U if case["epi"] == EPI_QKV_ROPE else 2 * U) + 2 * U * ref.abs())


def check_consumer(ops, outs, R=None, strict=True):
    """raises AssertionError with the relation that failed (strict = False: the ratios are reported, not asserted); returns dict(err: worst |out - ref| / bound over the rows inside the contract, kinds: the same per row
    kind, out_of_contract: worst row-wise ratio of the rows with kappa > 300 against C_V_OUT x their kappa^2 term, shift: worst ratio of the shift bookkeeping)"""
    case = ops["case"]
    M = case["M"]
    R = consumer_reference(ops) if R is None else R
    buf = outs["out"]
    assert bool((buf[:LEAD] == G.CANARY16).all()) and bool((buf[LEAD + M:] == G.CANARY16).all()), "canaries around out overwritten"
    got16 = buf[LEAD:LEAD + M].contiguous()
    assert not bool((got16 == G.CANARY16).any()), "elements of out not written (or NaN)"
    got = got16.view(torch.float16).double()
    assert bool(torch.isfinite(got).all()), "out not finite"
    kinds = torch.arange(M, device=got.device) % NK
    sat = kinds == KINDS.index("saturate")
    outc = (R["kappa"] > KAPPA_CONTRACT) & ~sat
    inc = ~(outc | sat)
    q = (got - R["ref"]).abs() / R["bound"]
    rep = dict(err=float(q[inc].max()), kinds={}, out_of_contract=0.0, kappa_max=float(R["kappa"][inc].max()))
    for i, name in enumerate(KINDS):
        sel = inc & (kinds == i)
        if bool(sel.any()):
            rep["kinds"][name] = round(float(q[sel].max()), 3)
    if bool(outc.any()):
        rep["out_of_contract"] = float(((got - R["ref"]).abs().max(1).values[outc] / (C_V_OUT * R["rowterm"][outc])).max())
    # the shift: old + mu = the mean of x, once.  mu is a sum of 768 fp32 values of size <= |y| in 4 stages (16 + 4 + 12 terms and the product with 1 / K)
    sh = outs["shift"]
    assert _nan_outside(sh, M), "ln_shift written outside its M rows"
    new = sh[LEAD:LEAD + M].double()
    assert bool(torch.isfinite(new).all()), "ln_shift not finite"
    y = ops["y"].double()
    tol = (15 + 3 + 11 + 2) * U32 * y.abs().mean(1) + 2 * U32 * ops["x"].double().mean(1).abs() + 1e-30
    rep["shift"] = float(((new - ops["x"].double().mean(1)).abs() / tol)[~sat].max())
    if strict:
        assert rep["shift"] <= 1.0, ("ln_shift != (init ? 0 : old) + mu", rep)
        assert rep["err"] <= 1.0, ("out against fp64 epi(LN(x) W^T + b)", rep)
        assert rep["out_of_contract"] <= 1.0, ("rows with kappa > 300 against the kappa^2 term", rep)
    return rep


# ---- the chain: three decoder blocks of a folding call, driven through the launches alone
CHAIN_L, CHAIN_M, CHAIN_C = 3, 196, 256


def make_chain(precision, device="cpu", seed=0):
    """weights of 3 blocks (fp16w2: every Linear split; fp16wa: the MLP's plain, the others split; the embed plain in both), the encoder tokens, and the fixed fp16
    attention outputs that feed the two proj Linears"""
    g = torch.Generator().manual_seed(12001 + seed)
    M = CHAIN_M
    mlp = "plain" if precision == "fp16wa" else "split"

    def lin(N, K, scale=1.0):
        return torch.randn((N, K), generator=g) * (scale / math.sqrt(K)), 0.1 * torch.randn((N,), generator=g)

    def norm():
        return 1.0 + 0.3 * torch.randn((D,), generator=g), 0.2 * torch.randn((D,), generator=g)
    ch = dict(precision=precision, M=M, tokens=torch.randn((M, CHAIN_C), generator=g).half(), pos=positions(M), layers=[])
    We, be = lin(D, CHAIN_C)
    ch["embed"] = dict(zip(("W", "parts"), _weights(We, "plain")), bias=be, bias2=0.1 * torch.randn((D,), generator=g))
    for _ in range(CHAIN_L):
        ly = {}
        for name, N, w in (("qkv", 3 * D, "split"), ("projq", D, "split"), ("fc1", 4 * D, mlp)):
            Wf, b = lin(N, D, W_SCALE)
            gam, bet = norm()
            W, parts, s_n, c_n = fold_weights(Wf, gam, bet, b, w)
            ly[name] = dict(W=W, parts=parts, s_n=s_n, c_n=c_n, weights=w)
        for name, K, w in (("proj", D, "split"), ("cproj", D, "split"), ("fc2", 4 * D, mlp)):
            Wf, b = lin(D, K, 0.5)
            W, parts = _weights(Wf, w)
            ly[name] = dict(W=W, parts=parts, bias=b, weights=w)
        ly["attn"] = (torch.randn((M, D), generator=g).half(), torch.randn((M, D), generator=g).half())
        ch["layers"].append(ly)

    def mv(o):
        if isinstance(o, torch.Tensor):
            return o.to(device)
        if isinstance(o, dict):
            return {k: mv(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return type(o)(mv(v) for v in o)
        return o
    return mv(ch)


def run_chain(ch, run, device="cpu"):
    """embed -> 3 x (qkv, proj, projq, proj, fc1, fc2) as decode_impl launches them; run(op) executes one launch.  After every consumer: its shift against the fp64 mean of
    the current x, the kappa of the rows it read (<= 2: a condition on the inputs), and its output inside the bound of that kappa.  Returns the list of reports."""
    M = ch["M"]
    nan = float("nan")
    x = torch.full((M, D), nan, device=device)
    x16 = torch.full((M, D), G.CANARY16, dtype=torch.int16, device=device)
    stats = torch.full((M, SLOTS, 2), nan, device=device)
    copy = torch.full((M, D), nan, device=device)
    shift = torch.full((M,), nan, device=device)
    reports = []

    def producer(epi, A, w, K, shifted, copied, fold=True, bias2=None):
        run(dict(role="producer", epi=epi, M=M, N=D, K=K, A=A, W=w["W"], parts=w["parts"], wsplit=0 if len(w["parts"]) == 1 else 2, bias=w["bias"], bias2=bias2,
                 row_start2=0, out=x, x16=x16 if fold else None, copy=copy if copied else None, stats=stats if fold else None, shift=shift if shifted else None))
        if copied:
            assert torch.equal(copy.view(torch.int32), x.view(torch.int32)), "copy32 != out"

    def consumer(name, epi, w, first, rope_cols, scale_cols):
        N = w["W"].shape[0]
        old = torch.zeros_like(shift) if first else shift.clone()
        y = x - old[:, None]
        assert torch.equal(x16, round16(y).view(torch.int16)), (name, "x16 != fp16_sat(x - shift)")
        out = torch.full((M, N), G.CANARY16, dtype=torch.int16, device=device)
        run(dict(role="consumer", epi=epi, M=M, N=N, K=D, A=x16.view(torch.float16), stats=stats, W=w["W"], parts=w["parts"], wsplit=0 if len(w["parts"]) == 1 else 2,
                 s_n=w["s_n"], bias=w["c_n"], eps=EPS, shift=shift, init=1 if first else 0, pos=ch["pos"], rope_cols=rope_cols, scale_cols=scale_cols, out=out))
        case = dict(M=M, N=N, epi=epi, rope_cols=rope_cols, scale_cols=scale_cols, init=1 if first else 0)
        ops = dict(case=case, x=x.clone(), y=y, parts=w["parts"], c_n=w["c_n"], pos=ch["pos"], shift=old)
        R = consumer_reference(ops)
        got = out.view(torch.float16).double()
        assert bool(torch.isfinite(got).all()), (name, "out not finite")
        xm = x.double().mean(1)
        tol = 31 * U32 * y.double().abs().mean(1) + 2 * U32 * xm.abs() + 1e-30
        rep = dict(consumer=name, err=float(((got - R["ref"]).abs() / R["bound"]).max()), kappa=float(R["kappa"].max()),
                   shift=float(((shift.double() - xm).abs() / tol).max()))
        reports.append(rep)
        return out

    producer(EPI_F32, ch["tokens"], ch["embed"], CHAIN_C, False, True, bias2=ch["embed"]["bias2"])
    for l, ly in enumerate(ch["layers"]):
        consumer(f"l{l}.qkv", EPI_QKV_ROPE, ly["qkv"], l == 0, 2 * D, D)
        producer(EPI_RESID_F32, ly["attn"][0], ly["proj"], D, True, False)
        consumer(f"l{l}.projq", EPI_STORE16, ly["projq"], False, 0, D)
        producer(EPI_RESID_F32, ly["attn"][1], ly["cproj"], D, True, False)
        g16 = consumer(f"l{l}.fc1", EPI_STORE16_GELU, ly["fc1"], False, 0, 0)
        last = l + 1 == len(ch["layers"])
        producer(EPI_RESID_F32, g16.view(torch.float16), ly["fc2"], 4 * D, not last, not last, fold=not last)
    return reports


def emulate(op, **defect):
    """the emulation as a back end of run_chain and of the host checks"""
    if op["role"] == "producer":
        emulate_producer(op, **defect)
    else:
        emulate_consumer(op, **defect)
