"""Shared by tests/test_resid_forms_gpu.py (the fp32 residual epilogue EPI_RESID_F32 and the exact-erf GELU epilogue EPI_STORE16_GELU of csrc/gemm.hip, in every kernel
the default dispatch reaches from the six Linears of csrc/model.hip that use them, through must3r_hip_op_gemm_ex, against fp64) and tests/test_resid_forms_host.py (the
table is complete, the bounds leave room, the checks discriminate).  Dispatch, DT, round16, bound, the canary constants and the 2:4 rule come from tests/gemm_forms.py.
Nothing here needs a GPU.

Case table.  Sites: encoder proj (RESID, N 1024, K 1024), fc1 (GELU, 4096, 1024), fc2 (RESID, 1024, 4096); decoder proj and cross proj (RESID, 768, 768), fc1 and
feedback fc1 (GELU, 3072, 768), fc2 (RESID, 768, 3072).  Weights: plain (bf16 and fp16), split and sparse-split (fp16).  Per (site, weights), M = 4, 8 .. 40000 goes
through the restated dispatch; every distinct kernel name gets the smallest M that reaches it (on a grid of 4: a few rows behind a tile boundary, the ragged last row
block of epilogue_row) and the next whole multiple of the family's tile height with the same name (the whole-tile paths of epilogue_tile).  K enters the dispatch by
divisibility only: the whole-tile case keeps the site's K; the ragged case takes the smallest K the family's rule admits on the proj sites and the decoder's fc1
(one K-tile; g48k128: 256) and the next one on the fc2 sites and the encoder's fc1 (two K-tiles; g48k128: 384), the other way round with sparse weights, so that every family meets both with each epilogue.

Relations, under the default options.  v32 = the EPI_F32 twin of the launch (same operands, own canary-framed buffer), held to fp64 by gemm_forms.bound unchanged.
  RESID, exact: out == fl32(x0 + v32) bit for bit.  The epilogue computes x_old + (acc + bias) (epilogue_row, and the straight-line and batched paths of epilogue_tile),
      the library is built without contraction and every tile shape accumulates in one order (gemm_forms relies on the same for projq).  x0 is not randn: blocks of
      24 rows x 40 columns (they cross every tile and wave-tile boundary) of +0, -0, fp32 subnormals, 2^-20 r, r and 2^12 r, r ~ N(0, 1) with a full mantissa, so that a
      lost low bit, a stale or doubled row or a reordered bias changes bits somewhere.  No family needed the weaker form (LEGIT_ORDER is empty).
  RESID against fp64: |out - (x0 + p64)| <= bound(p64) + 2^-24 |out|, p64 = the fp64 product plus bias; recorded as a ratio for every case.
  GELU against the twin: |out - gelu64(v32)| <= u |g| + 1.3e-6 + h: one 16-bit rounding, the figure common.hpp documents for gelu_erf, half the format's smallest
      subnormal step; fp16 saturated at +-65504 (cvt4_sat).
  GELU against fp64: 2u / 2u, 2u / 8u with a sparse low part (test_gemm_store_gelu_resid_f32, test_gemm_sparse_low_part).
  Canaries in front of and behind every destination (the residual's are finite, so that a read-modify-write of a row past M changes them), the inputs bit-identical
  after the launch, a second launch the same bits.

GELU over its domain: with A = 0 the accumulator is exactly +0 and the stored value is T(gelu_erf(bias[n])).  DOMAIN holds every finite fp16 value, both signs of 0 and of
fp32 subnormals, a dense run across |x| = 4.3 sqrt 2 (the end of the fitted interval), a run from there to where the erfc term underflows, 1e4, values beyond 65504 and
1e30; NaN and +-inf behind them.  Held: the bound above; the sign rule (no positive output for a negative input, no negative one for a positive input); out == T(x) for
x >= 1 wherever fp64 puts the erfc term below h (for tiny x the term x / 2 is below h as well, but there T(x / 2) != T(x) is right); NaN in, NaN out.  +-inf is recorded:
gelu_erf is defined on finite pre-activations and gives NaN for both.  The same launches with EPI_STORE16 hold the store itself over the same
inputs: T(x) bit for bit, fp16 saturated at +-65504 with +-inf included, NaN kept (cvt4_sat: a clamp in fp32 stored -65504 for a NaN until this file found it)."""
import math

import torch

import gemm_forms as F
from gemm_forms import DT, EPI_F32, EPI_RESID_F32, EPI_STORE16_GELU, F16_MAX, LEAD, PAD, bound, dispatch, round16
from test_ops_gpu import _prune24

RESID, GELU = EPI_RESID_F32, EPI_STORE16_GELU
SITES = (("enc_proj", RESID, 1024, 1024), ("enc_fc1", GELU, 4096, 1024), ("enc_fc2", RESID, 1024, 4096),
         ("dec_proj", RESID, 768, 768), ("dec_fc1", GELU, 3072, 768), ("dec_fc2", RESID, 768, 3072))
WEIGHTS = ("plain", "split", "sparse")
M_STEP, M_MAX = 4, 40000
TWO_K_TILES = ("enc_fc1", "enc_fc2", "dec_fc2")     # sites whose ragged cases run two K-tiles (sparse weights: one)
TILE_M = {"g64p": 64, "g64": 64, "g48": 48, "g48k128": 48, "g96": 96, "g128": 128, "g256": 256, "g256p": 256, "g256ps": 256, "g256s": 256, "g256o2": 256, "g256k": 256}
CANARY_X = 1.2345678        # the residual stream's canary rows: finite, so that x += v on a row past M changes them
GELU_ABS = 1.3e-6           # common.hpp: |GELU error| of gelu_erf in fp32 arithmetic
HALF_STEP = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -134}     # half the smallest subnormal step
LEGIT_ORDER = ()            # families whose RESID and F32 instantiations accumulate in different orders (none: the exact relation holds everywhere)
ERFC_Q = (1.1510913372039795, 0.4592546820640564, 0.052561257034540176, -0.007397521752864122, 0.0005204606568440795)   # common.hpp kErfcQ0..4


def site_dispatch(site, weights, M, K=None):
    _, epi, N, K0 = site
    return dispatch(epi, M, N, K0 if K is None else K, 0 if weights == "plain" else 2, 1, weights == "sparse")


def sweep_names(site, weights):
    """{kernel name: the smallest M of the sweep that reaches it}, in order of appearance"""
    first = {}
    for M in range(M_STEP, M_MAX + 1, M_STEP):
        first.setdefault(site_dispatch(site, weights, M), M)
    return first


def _small_k(fam, second):
    k0 = 256 if fam == "g48k128" else 64     # launch_48: the 128-deep K-tiles need K % 128 == 0 and K >= 256
    return k0 + (128 if fam == "g48k128" else 64) * (1 if second else 0)


def _cases():
    out = []
    for site in SITES:
        tag, epi, N, K0 = site
        for w in WEIGHTS:
            for kern, m0 in sweep_names(site, w).items():
                fam = kern.split("/")[0]
                T = TILE_M[fam]
                m1 = next(m for m in range((m0 // T + 1) * T, M_MAX + 4 * T, T) if site_dispatch(site, w, m) == kern)
                for kind, M, K in (("ragged", m0, _small_k(fam, (tag in TWO_K_TILES) != (w == "sparse"))), ("whole", m1, K0)):
                    assert site_dispatch(site, w, M, K) == kern, (tag, w, kern, M, K)
                    c = F._case("resid" if epi == RESID else "gelu", f"{tag}-{w}-{kern.replace('/', '_')}-{kind}-M{M}-K{K}", epi, N, K, M)
                    c.update(site=tag, weights=w, kernel=kern, rows=kind, tile=T)
                    out.append(c)
    return out


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)
COMBOS = [(c["name"], dt) for c in CASES for dt in (("bf16", "fp16") if c["weights"] == "plain" else ("fp16",))]


# ---- operands and references
def make_operands(case, dt, device):
    ops = F.make_operands(case, dt, case["weights"], device, seed=len(case["name"]))
    assert ops["kernel"] == case["kernel"]
    return ops


def twin_ops(ops):
    """the EPI_F32 launch of the same operands: with the packed low part exactly where the kernel under test multiplies it (a GELU launch of sparse weights that the
    dispatch gives to g256o2, g96 or the small tiles multiplies the dense low part)"""
    case = dict(ops["case"], epi=EPI_F32)
    weights = ops["weights"] if ops["weights"] != "sparse" or ops["w3"] else "split"
    kern = dispatch(EPI_F32, case["M"], case["N"], case["K"], 0 if weights == "plain" else 2, 1, weights == "sparse")
    assert (kern.split("/")[2] == "w3") == ops["w3"], (ops["kernel"], kern)
    return dict(ops, case=case, weights=weights, kernel=kern)


def make_x0(M, N, device, seed=0):
    """the old residual stream: blocks of 24 rows x 40 columns of +0, -0, subnormals, 2^-20 r, r, 2^12 r (r ~ N(0, 1), never 0)"""
    g = torch.Generator(device=device).manual_seed(4177 + seed)
    r = torch.randn((M, N), device=device, generator=g)
    r = torch.where(r == 0, torch.ones_like(r), r)
    kind = ((torch.arange(M, device=device) // 24)[:, None] + (torch.arange(N, device=device) // 40)[None, :]) % 6
    sub = torch.copysign(torch.full_like(r, 2.0 ** -140), r) * (1 + (r.abs() * 977).floor() % 512)      # 2^-140 .. 2^-131
    x = torch.where(kind == 0, torch.zeros_like(r), r)
    x = torch.where(kind == 1, -torch.zeros_like(r), x)
    x = torch.where(kind == 2, sub, x)
    x = torch.where(kind == 3, r * 2.0 ** -20, x)
    x = torch.where(kind == 5, r * 2.0 ** 12, x)
    return x.contiguous()


def gelu64(v):
    """exact-erf GELU in fp64, the negative tail as a product: x / 2 erfc(-x / sqrt 2)"""
    v = v.double()
    return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))


def erfc_term64(x):
    """|x| / 2 erfc(|x| / sqrt 2): what GELU subtracts from max(x, 0)"""
    a = x.double().abs()
    return 0.5 * a * torch.special.erfc(a / math.sqrt(2.0))


def sat(g, dt):
    return g.clamp(-F16_MAX, F16_MAX) if dt == "fp16" else g


def gelu_kernel(v, tanh=False, no_max=False):
    """common.hpp gelu_erf on fp32 values: max(x, 0) - a 2^(-a Q(a) - 1), evaluated in fp64 and rounded to fp32 once.  Defects: the tanh form; max(x, 0) dropped"""
    x = v.double()
    if tanh:
        return (0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))).float()
    a = x.abs()
    q = torch.full_like(a, ERFC_Q[4])
    for c in ERFC_Q[3::-1]:
        q = q * a + c
    e = torch.exp2((-a * q - 1.0).clamp(min=-1100.0))
    e = torch.where(e < 2.0 ** -126, torch.zeros_like(e), e)      # v_exp_f32 flushes a subnormal result
    return ((0.0 if no_max else x.clamp(min=0)) - a * e).float()


def f32_bound(case, dt, kernel):
    return bound(dict(case, epi=EPI_F32), dt, kernel)


def gelu_bound64(case, dt, kernel):
    u = DT[dt][2]
    return 2 * u, (8 * u if kernel.split("/")[2] == "w3" else 2 * u)


# ---- destinations
def frame(inner, fill):
    """[LEAD + M + PAD, N] filled with `fill`, `inner` (or nothing) in rows LEAD .. LEAD + M; returns (buffer, the [M, N] window)"""
    M, N = inner.shape
    buf = torch.full((LEAD + M + PAD, N), fill, dtype=inner.dtype, device=inner.device)
    buf[LEAD:LEAD + M] = inner
    return buf, buf[LEAD:LEAD + M]


def frame_like(case, dtype, device, fill):
    return frame(torch.full((case["M"], case["N"]), fill, dtype=dtype, device=device), fill)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_frame(buf, fill, M, what):
    """nothing in front of row 0 or behind row M - 1 changed, bit for bit; every element of the window written (twin and GELU: no canary left inside)"""
    ref = torch.full((1,), fill, dtype=buf.dtype, device=buf.device)
    edge = torch.cat((buf[:LEAD], buf[LEAD + M:]))
    assert bool((bits(edge) == bits(ref)).all()), f"{what}: canary rows in front of row 0 or behind row M - 1 changed"


def check_written(view, fill, what):
    left = torch.isnan(view).any() if view.dtype == torch.float32 else (view == fill).any()
    assert not bool(left), f"{what}: elements of the destination not written (or NaN)"


# ---- the checks.  Each returns a ratio or raises AssertionError naming the relation
def check_resid_exact(out, x0, v32, what=""):
    want = x0 + v32
    bad = bits(out) != bits(want)
    n = int(bad.sum())
    if n:
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"exact relation out == fl32(x0 + v32) fails on {n} elements, first at {i}: out {out[i[0], i[1]].item()!r}, want {want[i[0], i[1]].item()!r}, "
                             f"x0 {x0[i[0], i[1]].item()!r}, v32 {v32[i[0], i[1]].item()!r} {what}")


def resid_ratio64(out, x0, p64, rtol, atol, room=False):
    """max |out - (x0 + p64)| / (atol + rtol |p64| + 2^-24 |out|).  room: max (|out - (x0 + p64)| - 2^-24 |out|) / (atol + rtol |p64|): the share of the product's
    allowance that is used once the one rounding of the sum, which a correct result reaches in full, is taken off"""
    o = out.double()
    err, rnd, tol = (o - (x0.double() + p64)).abs(), 2.0 ** -24 * o.abs(), atol + rtol * p64.abs()
    r = (((err - rnd).clamp(min=0) / tol) if room else (err / (tol + rnd))).max().item()
    return float("inf") if r != r else r


def gelu_ratio(out, x, dt, room=False):
    """max |out - gelu64(x)| / (u |g| + 1.3e-6 + h), g saturated as the fp16 store saturates.  room: max (|out - g| - u |g| - h) / 1.3e-6: the share of gelu_erf's
    documented error that is used once the 16-bit rounding, which a correct result reaches in full, is taken off"""
    g = sat(gelu64(x), dt)
    err, rnd = (out.double() - g).abs(), DT[dt][2] * g.abs() + HALF_STEP[dt]
    r = (((err - rnd).clamp(min=0) / GELU_ABS) if room else (err / (rnd + GELU_ABS))).max().item()
    return float("inf") if r != r else r


def check_sign(out, x):
    o = out.double()
    assert not bool(((x < 0) & (o > 0)).any()), "sign rule: a positive output for a negative input"
    assert not bool(((x > 0) & (o < 0)).any()), "sign rule: a negative output for a positive input"


def check_identity_tail(out, x, dt):
    """out == T(x) for x >= 1 wherever the erfc term is below h in fp64"""
    sel = (x >= 1) & (erfc_term64(x) < HALF_STEP[dt])
    assert bool(sel.any())
    assert bool((bits(out[sel]) == bits(round16(x[sel], dt))).all()), "out != T(x) where the erfc term is below half a subnormal step"


# ---- GELU over its domain
def domain():
    """(x fp32 [n], n a multiple of 256; finite: the first `nf` entries; then NaN, +inf, -inf and zero padding)"""
    h = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16).float()      # every finite fp16 >= 0
    edge = 4.3 * math.sqrt(2.0)
    ulp = 2.0 ** -21                                                                                # of fp32 at 6.08
    parts = [h,
             torch.tensor([2.0 ** -149, 2.0 ** -140, 3e-41, 6e-41, 1e-39, 2.0 ** -127, 2.0 ** -126]),
             torch.tensor(edge, dtype=torch.float64).float() + torch.arange(-1024, 1025) * ulp,       # every fp32 value around the end of the fit
             torch.linspace(6.0, 6.2, 1025), torch.linspace(5.0, 15.0, 4001),
             torch.tensor([20.0, 100.0, 1e4, 65504.0, 65519.0, 65520.0, 7e4, 1e5, 1e10, 1e30, 3e38])]
    pos = torch.cat(parts)
    fin = torch.cat((pos, -pos))
    tail = torch.tensor([float("nan"), float("inf"), float("-inf")])
    n = fin.numel() + 3
    x = torch.cat((fin, tail, torch.zeros((-n) % 256)))
    return x.contiguous(), fin.numel()


DOMAIN_RUNS = [   # (tag, dt, weights, M): M = 4 the per-row store path, M = 64 the whole-fragment path that trades rows between lanes, then chip-filling families
    ("row", "bf16", "plain", 4), ("row", "fp16", "plain", 4), ("row", "fp16", "split", 4),
    ("frag", "bf16", "plain", 64), ("frag", "fp16", "plain", 64), ("frag", "fp16", "split", 64),
    ("chip", "bf16", "plain", 768), ("chip", "fp16", "plain", 772), ("chip", "fp16", "split", 260),
]


def domain_kernel(weights, M, N, epi=GELU):
    return dispatch(epi, M, N, 64, 0 if weights == "plain" else 2, 1, False)


def check_store_domain(out, x, nf, dt):
    """EPI_STORE16 of the same launches stores T(+0 + x): round to nearest even, fp16 saturated at +-65504 (+-inf included), NaN kept"""
    want = round16(torch.zeros_like(x) + x, dt)
    fin = torch.ones_like(x, dtype=torch.bool)
    fin[nf] = False
    assert bool((bits(out[fin]) == bits(want[fin])).all()), "16-bit store: out != T(x), saturated"
    assert bool(torch.isnan(out[nf].float())), "NaN in, no NaN out"


def check_domain(out, x, nf, dt):
    """out: the stored row [n] for the inputs x; returns the ratio of the bound over the finite inputs"""
    o, xf = out[:nf], x[:nf]
    r = gelu_ratio(o, xf, dt)
    assert r <= 1.0, f"GELU bound u |g| + 1.3e-6 + h: ratio {r}"
    check_sign(o, xf)
    check_identity_tail(o, xf, dt)
    assert bool(torch.isnan(out[nf].float())), "NaN in, no NaN out"
    return r


# ---- the sparse pack's position halfwords (the layout stated above misc.hip::sparse24_pack_kernel)
def decode_idx(idx, rows, K):
    """idx [K/64][rows/32][64] dwords -> positions [rows][K/64][4 g][4 q][2] of the two kept entries of group k = 64 t + 16 g + 4 q + e"""
    hw = idx.contiguous().view(torch.int16).reshape(K // 64, rows // 32, 64, 2).to(torch.int32) & 0xFFFF
    n = torch.arange(rows, device=idx.device)
    g = torch.arange(4, device=idx.device)
    b = hw[:, (n // 32)[:, None], ((n % 16)[:, None] + 16 * g[None, :]), ((n % 32) // 16)[:, None]]      # [t][n][g]
    q = torch.arange(4, device=idx.device)
    first, second = (b[..., None] >> (4 * q)) & 3, (b[..., None] >> (4 * q + 2)) & 3
    return torch.stack((first, second), -1).permute(1, 0, 2, 3, 4)


def encode_idx(pos):
    """the inverse of decode_idx (host round trip)"""
    rows, T = pos.shape[:2]
    q = torch.arange(4)
    b = ((pos[..., 0] | (pos[..., 1] << 2)) << (4 * q)).sum(-1)      # [n][t][g]
    hw = torch.zeros((T, rows // 32, 64, 2), dtype=torch.int32)
    n = torch.arange(rows)
    for g in range(4):
        hw[:, n // 32, n % 16 + 16 * g, (n % 32) // 16] = b[:, :, g].t().to(torch.int32)
    d = hw[..., 0].to(torch.int64) | (hw[..., 1].to(torch.int64) << 16)
    return torch.where(d >= 2 ** 31, d - 2 ** 32, d).to(torch.int32)


def pruned_positions(lo):
    """_prune24's kept positions [rows][K/64][4][4][2] in k order, and where a group has two non-zero kept entries (else "which zero" is ambiguous)"""
    rows, K = lo.shape
    kept = _prune24(lo).reshape(rows, K // 64, 4, 4, 4)
    nz = torch.argsort((kept == 0).to(torch.int8), dim=-1, stable=True)[..., :2].sort(dim=-1).values
    return nz.to(torch.int32), (kept != 0).sum(-1) == 2


def check_positions(idx, lo):
    rows, K = lo.shape
    want, two = pruned_positions(lo)
    got = decode_idx(idx, rows, K)
    assert bool(two.any()) and bool((got[two] == want[two].to(got.device)).all()), "sparse pack: position halfwords differ from the 2:4 rule"


# ---- fp32 emulation of what the kernels write, with the defects the host file plants
def emulate_resid(ops, x0, rows, trunc24=False, double_ragged=False, bias_last=False):
    """rows `rows` of the new residual stream (x0: the old values of those rows) and of the twin.  Defects: the old residual kept in its top 24 bits; the old row added twice in the ragged last row
    block; (x0 + acc) + bias"""
    case = ops["case"]
    acc = F.linear(dict(ops, bias=torch.zeros_like(ops["bias"])), 0, rows, torch.float32).float()
    b = ops["bias"][0]
    v32 = acc + b
    x = x0
    if trunc24:
        x = (x.view(torch.int32) & ~0xFF).view(torch.float32)
    if bias_last:
        out = (x + acc) + b
    else:
        out = x + v32
    if double_ragged:
        rag = rows >= case["M"] // case["tile"] * case["tile"]
        out = torch.where(rag[:, None], out + x, out)
    return out, v32


def emulate_gelu(ops, rows, **defect):
    v32 = F.linear(ops, 0, rows, torch.float32).float()
    return round16(gelu_kernel(v32, **defect), ops["dt"]), v32


def edge_rows(case, n=6):
    """the first and last n rows and both sides of the last tile boundary"""
    M, T = case["M"], case["tile"]
    last = (M - 1) // T * T
    r = set(range(min(n, M))) | set(range(max(0, M - n), M)) | {m for m in (last - 1, last, last + 1) if 0 <= m < M}
    return torch.tensor(sorted(r))
