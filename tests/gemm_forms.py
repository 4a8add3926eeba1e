"""Shared by tests/test_gemm_forms_gpu.py (the grouped and per-scene argument forms in which the batched decoder launches its GEMMs, through must3r_hip_op_gemm_ex,
against fp64) and tests/test_gemm_forms_host.py (the checks discriminate): the default dispatch restated, the case table, the operands (every weight group its own
weights and bias), the fp64 reference, the bounds, the canary-filled destinations, the checks, and an fp32 emulation of what the kernels write (with the defects the host
file plants).  Nothing here needs a GPU.

Forms (call sites in csrc/model.hip): kv_scene (kv_project: one problem per scene, shared weights, out_table), kv_all (projkv_all: problem g = l S + b uses layer g / S's
weights, bias and rows of the packed sparse low part; run with the model's 16-bit store and with an fp32 twin of the same launch, whose bound resolves the low part),
embed (enc->dec embed: bias2 on the rows with m % row_period2 >= row_start2), q_scaled (projq, decoder qkv, encoder qkv: out_scale on the columns < scale_cols before
rounding, after RoPE), head_scenes (EPI_HEAD: scenes head_scene_skip floats further apart than contiguous).

Reference: fp64 over exactly the operands the kernel multiplies (the convention of test_ops_gpu.py): 16-bit-rounded A; plain weights: the 16-bit-rounded W; dense split:
W_hi + W_lo; sparse: W_hi + P(W_lo) (test_ops_gpu._prune24) where the dispatch reaches a sparse kernel (w3), W_hi + W_lo where it falls back to the dense ones.

Error measure: ratio = max |out - ref| / (atol + rtol |ref|), so allclose(out, ref, rtol, atol) <=> ratio <= 1.  Bounds (u = unit round-off), each from the test named:
16-bit stores 2u / 2u (test_gemm_store_gelu_resid_f32), with RoPE 2u / 4u (test_gemm_qkv_rope), with a sparse low part 2u / 8u (test_gemm_sparse_low_part); fp32 outputs
1e-5 / 1e-4 with plain weights (test_gemm_store_gelu_resid_f32), 2e-6 / 8e-6 with split or sparse weights (test_gemm_sparse_low_part); EPI_HEAD as fp32 plain.  The fp32
emulation on the CPU stays within half of each (tests/test_gemm_forms_host.py, on the boundary rows of the large cases; over ALL rows of the largest fp32 split cases,
embed-r700-S26 and kv_all-L3-S2-r768-f32, it measures 0.37 - 0.38), so no form needed a wider figure.

Exact relations: canaries in front of, behind and between all destinations; and for projq (scale without RoPE) out16 == T(v32 * out_scale) bit for bit, v32 = the fp32 twin
of the same launch (EPI_F32, no scale): every tile shape accumulates in the same order and the library is built without contraction, and a scale applied after the
rounding stays inside 2u, so only the bits can tell."""
import math
import struct

import torch

from test_ops_gpu import _prune24   # the 2:4 rule of misc.hip::sparse24_pack_kernel, restated once

DT = {"bf16": (0, torch.bfloat16, 2.0 ** -8), "fp16": (1, torch.float16, 2.0 ** -11)}   # id, torch dtype, unit round-off
EPI_STORE16, EPI_STORE16_GELU, EPI_QKV_ROPE, EPI_RESID_F32, EPI_F32, EPI_HEAD = range(6)
LEAD, GAP, PAD = 2, 1, 3      # canary rows in front of the first destination, between two destinations, behind the last
LEAD_E, PAD_E = 64, 96        # EPI_HEAD: canary floats in front of scene 0 and behind the last scene
CANARY16 = 0x7E55             # fp16: a NaN; bf16: 7e37.  No output of these cases
F16_MAX = 65504.0
OUT_SCALE = struct.unpack("f", struct.pack("f", 0.125 * math.log2(math.e)))[0]   # the fp32 value the kernel multiplies with
NPOS = 64


# ---- csrc/gemm_route.hpp gemm_route restated for the table defaults of options.hpp (GEMM256 = G256K = G256P = G256P_SPLIT = SPARSE_256 = SPARSE_LO = BK128 = 1,
# PERSIST = 0), without the LN fold: an independent restatement, held against the rule itself point for point without a GPU (tests/test_gemm_route_host.py).
# sparse: the caller passes the packed low part.  Returns gemm_last_kernel()'s "<family>/e<EPI>/w<WS>/n<BN>".
def _fill(t):
    return t * 100 // (((t + 255) // 256) * 256)


def dispatch(epi, M, N, K, wsplit, batch=1, sparse=False):
    nb = batch if batch > 1 else 1
    rope, head = epi == EPI_QKV_ROPE, epi == EPI_HEAD
    rb256 = ((M + 255) // 256) * nb
    t48 = ((M + 47) // 48) * (N // 48) * nb
    use48 = N % 48 == 0 and K % 64 == 0 and not rope and not head and 192 <= t48 <= 256
    fam48 = "g48k128" if K % 128 == 0 and K >= 256 else "g48"
    small8 = ((M + 63) // 64) * (N // 64) * nb <= 256

    def name(fam, ws, bn):
        return f"{fam}/e{epi}/w{ws}/n{bn}"
    if wsplit == 2:
        t96 = ((M + 95) // 96) * (N // 96) * nb
        use96 = N % 96 == 0 and K % 64 == 0 and not head and 224 <= t96 <= 256
        tiles = ((M + 127) // 128) * (N // 64) * nb
        t256, t192, t128 = rb256 * (N // 256), rb256 * (N // 192), rb256 * (N // 128)
        ok256, ok128 = N % 256 == 0 and K % 32 == 0, N % 128 == 0 and K % 32 == 0
        ok192 = N % 192 == 0 and K % 32 == 0 and not rope
        pick, best = 0, -1
        for bn, t, ok in ((256, t256, ok256), (192, t192, ok192), (128, t128, ok128)):   # cost ~ rounds x tile width; ties -> the wider tile
            if not ok or t < 200 or _fill(t) < 80:
                continue
            cost = ((t + 255) // 256) * bn
            if best < 0 or cost < best:
                best, pick = cost, bn
        if epi == EPI_STORE16_GELU and ok128 and t128 >= 1024:
            return name("g256o2", 2, 128)
        if use96:
            return name("g96", 2, 96)
        if use48:
            return name(fam48, 2, 48)
        if sparse and ok128 and K % 64 == 0 and t128 >= 200 and (_fill(t128) >= 80 or pick != 0):
            if ok256 and t256 >= 200 and _fill(t256) + 12 >= _fill(t128):
                return name("g256s", 3, 256)
            return name("g256ps", 3, 128)
        if pick != 0 and ok128 and K % 64 == 0 and (pick == 128 or (pick == 192 and t128 >= 200 and _fill(t128) >= _fill(t192) and _fill(t128) >= 90)):
            return name("g256p", 2, 128)
        if pick:
            return name("g256", 2, pick)
        if tiles >= 384:
            return name("g128", 2, 64)
        return name("g64p" if small8 else "g64", 2, 64)
    t256 = rb256 * (N // 256)
    ok256 = N % 256 == 0 and K % 32 == 0
    if use48:
        return name(fam48, 1, 48)
    if ok256 and t256 >= 200 and _fill(t256) >= 80:
        return name("g256p" if K % 64 == 0 and not rope else "g256k", 1, 256)
    if N % 128 == 0 and ((M + 127) // 128) * (N // 128) * nb >= 192:
        return name("g128", 1, 128)
    return name("g64p" if small8 else "g64", 1, 64)


# ---- the case table
def _case(kind, name, epi, N, K, M, P=1, S=1, L=1, **kw):
    """P problems of M rows each; S scenes, L weight groups (kv forms: P = L S).  The other fields by kind."""
    c = dict(kind=kind, name=name, epi=epi, N=N, K=K, M=M, P=P, S=S, L=L, ldc=0 if epi == EPI_HEAD else N, scale_cols=0, rope_cols=0, row_start2=0, row_period2=0,
             bias2=False, hv=0, skip=0)
    c.update(kw)
    return c


def _cases():
    out = []
    for rows, S in ((12, 2), (12, 6), (12, 12), (12, 16), (12, 24), (12, 28), (12, 36), (700, 6), (768, 2), (196, 12), (1000, 3), (700, 28), (768, 28)):
        out.append(_case("kv_scene", f"kv_scene-r{rows}-S{S}", EPI_STORE16, 1536, 768, rows, P=S, S=S))
    for L, S, rows in ((3, 4, 12), (4, 7, 12), (12, 3, 12), (12, 1, 768), (3, 2, 768), (5, 4, 196)):
        assert L != S
        out.append(_case("kv_all", f"kv_all-L{L}-S{S}-r{rows}", EPI_STORE16, 1536, 768, rows, P=L * S, S=S, L=L))
        out.append(_case("kv_all", f"kv_all-L{L}-S{S}-r{rows}-f32", EPI_F32, 1536, 768, rows, P=L * S, S=S, L=L))
    for rows, S, rs2, per in ((392, 1, 196, 0), (600, 1, 0, 0), (1536, 1, 768, 0), (392, 5, 196, 392), (1536, 3, 768, 1536), (700, 13, 196, 700), (700, 19, 196, 700),
                              (700, 26, 196, 700), (700, 26, 0, 700)):
        out.append(_case("embed", f"embed-r{rows}-S{S}-s{rs2}-p{per}", EPI_F32, 768, 1024, rows * S, S=S, R=rows, bias2=True, row_start2=rs2, row_period2=per))
    for M in (12, 600, 1400, 2700, 4100, 9000, 13300, 17600):
        out.append(_case("projq", f"projq-M{M}", EPI_STORE16, 768, 768, M, scale_cols=768))
    for V, gh, gw in ((1, 3, 4), (3, 14, 14), (5, 14, 14), (8, 14, 14), (16, 14, 14), (30, 14, 14)):
        out.append(_case("dec_qkv", f"dec_qkv-M{V * gh * gw}", EPI_QKV_ROPE, 2304, 768, V * gh * gw, V=V, gh=gh, gw=gw, rope_cols=1536, scale_cols=768))
    for V in (2, 5, 23):
        out.append(_case("enc_qkv", f"enc_qkv-M{V * 196}", EPI_QKV_ROPE, 3072, 1024, V * 196, V=V, gh=14, gw=14, rope_cols=2048, scale_cols=1024))
    for S, V, gh, gw in ((5, 3, 3, 4), (4, 2, 14, 14), (20, 2, 14, 14)):
        # contig: the form the model launches when the scenes are contiguous (head_views = 0); views0: the scene fields set with nothing between the scenes
        for tag, hv, skip in (("contig", 0, 0), ("views0", V, 0), ("skip4", V, 4), ("skip448", V, 7 * 64)):
            out.append(_case("head", f"head-S{S}-V{V}-{gh}x{gw}-{tag}", EPI_HEAD, 1792, 2304, S * V * gh * gw, S=S, V=V, gh=gh, gw=gw, hv=hv, skip=skip))
    return out


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)
GROUPED = ("kv_scene", "kv_all")


def weight_modes(case, dt):
    """fp16 runs plain, dense-split and sparse-split weights, bf16 plain only (split weights are fp16-only); the head runs plain weights"""
    return ("plain",) if dt == "bf16" or case["kind"] == "head" else ("plain", "split", "sparse")


COMBOS = [(c["name"], dt, w) for c in CASES for dt in ("bf16", "fp16") for w in weight_modes(c, dt)]


def kernel_of(case, weights):
    return dispatch(case["epi"], case["M"], case["N"], case["K"], 0 if weights == "plain" else 2, case["P"], weights == "sparse")


def bound(case, dt, kernel):
    """(rtol, atol) of the form's output, by output type, epilogue and the weights the kernel multiplies (module docstring)"""
    u = DT[dt][2]
    ws = kernel.split("/")[2]
    if case["epi"] in (EPI_STORE16, EPI_QKV_ROPE):
        return 2 * u, (8 * u if ws == "w3" else 4 * u if case["epi"] == EPI_QKV_ROPE else 2 * u)
    if case["epi"] == EPI_F32 and ws != "w1":
        return 2e-6, 8e-6
    return 1e-5, 1e-4


# ---- operands
def make_operands(case, dt, weights, device, seed=0):
    """A [P M, K] 16-bit (problem g: rows g M ...); Wf [L, N, K] / sqrt(K) and bias [L, N]: every weight group its own; W as the kernel takes it ([L, N, K] 16-bit, or
    [L, N, 2K] = [hi | lo] fp16), lo_p = P(lo) for the sparse mode; bias2 [N]; pos [M, 2] = (y, x) of views of gh x gw positions."""
    tdt = DT[dt][1]
    g = torch.Generator(device=device).manual_seed(977 + seed)

    def rn(*shape):
        return torch.randn(shape, device=device, generator=g)
    P, M, N, K, L = case["P"], case["M"], case["N"], case["K"], case["L"]
    kernel = kernel_of(case, weights)
    ops = dict(case=case, dt=dt, weights=weights, kernel=kernel, w3=kernel.split("/")[2] == "w3", A=rn(P * M, K).to(tdt))
    Wf = rn(L, N, K) / math.sqrt(K)
    ops["bias"] = rn(L, N)
    if weights == "plain":
        ops["W"] = Wf.to(tdt).contiguous()
    else:
        assert dt == "fp16"
        hi = Wf.half()
        lo = (Wf - hi.float()).half()
        ops["hi"], ops["lo"], ops["W"] = hi, lo, torch.cat((hi, lo), dim=2).contiguous()
        if weights == "sparse":
            ops["Wf"] = Wf.contiguous()      # what must3r_hip_op_sparse24_pack packs: all L N rows of the parameter
            ops["lo_p"] = _prune24(lo.reshape(L * N, K)).reshape(L, N, K)
    ops["bias2"] = rn(N) if case["bias2"] else None
    if case["epi"] == EPI_QKV_ROPE:
        ys, xs = torch.meshgrid(torch.arange(case["gh"]), torch.arange(case["gw"]), indexing="ij")
        ops["pos"] = torch.stack((ys.reshape(-1), xs.reshape(-1)), -1).repeat(case["V"], 1).contiguous().to(device)
    return ops


def weight_group(case, g):
    return g // case["S"] if case["L"] > 1 else 0


def _parts(ops, wg, wg_lo):
    if ops["weights"] == "plain":
        return (ops["W"][wg],)
    return ops["hi"][wg], (ops["lo_p"] if ops["w3"] else ops["lo"])[wg_lo]


def round16(v, dt):
    """what the 16-bit stores write: round to nearest even, fp16 saturated at +-65504 (common.hpp cvt4_sat)"""
    v = v.float()
    return (v.clamp(-F16_MAX, F16_MAX) if dt == "fp16" else v).to(DT[dt][1])


def _rope(v, pos, rope_cols):
    """oracle.must3r_ref.rope2d on the heads of the columns < rope_cols, in v's precision (its tables live on the CPU)"""
    from oracle import must3r_ref as R
    n = v.shape[0]
    t = v[:, :rope_cols].cpu().reshape(1, n, rope_cols // 64, 64).permute(0, 2, 1, 3)
    r = R.rope2d(t, pos.cpu()[None]).permute(0, 2, 1, 3).reshape(n, rope_cols).to(v.dtype)
    return torch.cat((r.to(v.device), v[:, rope_cols:]), dim=1)


def linear(ops, g, rows, prec, w_mod_L=False, bias_unstrided=False, sp_row0_zero=False):
    """acc + bias of rows `rows` of problem g in `prec`: what an EPI_F32 launch of the same operands stores.  Defects: the weights of group g % L; the bias of group 0;
    the sparse low part of group 0."""
    case = ops["case"]
    wg = g % case["L"] if w_mod_L else weight_group(case, g)
    a = ops["A"][g * case["M"] + rows].to(prec)
    v = None
    for p in _parts(ops, wg, 0 if sp_row0_zero and ops["w3"] else wg):     # hi before lo, as the kernels accumulate
        t = a @ p.to(prec).t()
        v = t if v is None else v + t
    return v + ops["bias"][0 if bias_unstrided else wg].to(prec)


def finish(ops, v, rows, prec, no_period=False, start2_off=0, scale_cols_off=0):
    """the epilogue's arithmetic on acc + bias, before any rounding to 16 bits.  Defects: row_period2 ignored; row_start2 moved; scale_cols moved"""
    case = ops["case"]
    if ops["bias2"] is not None:
        per = 0 if no_period else case["row_period2"]
        m = rows % per if per > 0 else rows
        v = v + (m >= case["row_start2"] + start2_off).to(prec)[:, None] * ops["bias2"].to(prec)
    if case["epi"] == EPI_QKV_ROPE:
        v = _rope(v, ops["pos"][rows], case["rope_cols"])
    sc = case["scale_cols"] + scale_cols_off
    if sc > 0:
        v = torch.cat((v[:, :sc] * OUT_SCALE, v[:, sc:]), dim=1)
    return v


def all_rows(ops):
    return torch.arange(ops["case"]["M"], device=ops["A"].device)


def reference(ops, g, rows=None):
    rows = all_rows(ops) if rows is None else rows
    return finish(ops, linear(ops, g, rows, torch.float64), rows, torch.float64)


def emulated(ops, g, rows, prec=torch.float32):
    """the clean emulation of rows `rows` of problem g, in the output's type"""
    v = finish(ops, linear(ops, g, rows, prec), rows, prec).float()
    return v if ops["case"]["epi"] in (EPI_F32, EPI_HEAD) else round16(v, ops["dt"])


def ratio(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|); inf when anything is NaN"""
    ref = ref.double()
    r = ((got.double() - ref).abs() / (atol + rtol * ref.abs())).max().item()
    return float("inf") if r != r else r


def boundary_rows(case, n=6):
    """host subset of a problem's rows: the first and last n, and both sides of every scene boundary and of every row_start2"""
    M = case["M"]
    r = set(range(min(n, M))) | set(range(max(0, M - n), M))
    R = case.get("R") or (case["gh"] * case["gw"] if "gh" in case else 0)
    if R:
        for s0 in range(0, M, R):
            for d in (-1, 0, 1, case["row_start2"] - 1, case["row_start2"], case["row_start2"] + 1, R - 1):
                if 0 <= s0 + d < M:
                    r.add(s0 + d)
    return torch.tensor(sorted(r))


# ---- destinations.  Every one is a row-offset pointer into a larger buffer with canaries in front, behind and between; the problems' slots are in permuted order
def slot_of(case, g):
    """slot of problem g's destination: a permutation of the P slots (scene b's rows do not lie behind scene b - 1's)"""
    P = case["P"]
    step = next(s for s in (5, 7, 11, 13, 3, 1) if math.gcd(s, P) == 1)
    return (g * step + P // 2) % P


def alloc_outputs(ops, device):
    """buf: the whole canary-filled buffer; views[g]: problem g's [M, N] window (EPI_HEAD: views[s] = scene s's [V H W 7] block of the flat buffer, base = the pointer the
    kernel is given); twin: where the fp32 twin of a projq launch goes"""
    case, dt = ops["case"], ops["dt"]
    P, M, N = case["P"], case["M"], case["N"]
    if case["epi"] == EPI_HEAD:
        se = case["V"] * case["gh"] * case["gw"] * 256 * 7
        buf = torch.full((LEAD_E + case["S"] * (se + case["skip"]) + PAD_E,), float("nan"), dtype=torch.float32, device=device)
        views = [buf[LEAD_E + s * (se + case["skip"]):][:se] for s in range(case["S"])]
        return dict(buf=buf, views=views, base=buf[LEAD_E:], scene_elems=se, dt=dt)
    rows = LEAD + P * (M + GAP) - GAP + PAD
    if case["epi"] == EPI_F32:
        buf = torch.full((rows, N), float("nan"), dtype=torch.float32, device=device)
    else:
        buf = torch.full((rows, N), CANARY16, dtype=torch.int16, device=device)
    starts = [LEAD + slot_of(case, g) * (M + GAP) for g in range(P)]
    return dict(buf=buf, views=[buf[s:s + M] for s in starts], starts=starts, base=buf[starts[0]:], dt=dt, twin=None)


def shuffle_head(case, v):
    """[M, 1792] (feature (i 16 + j) 7 + c of token (gy, gx) of view vv) -> [views, H W 7]"""
    nv, gh, gw = case["S"] * case["V"], case["gh"], case["gw"]
    return v.reshape(nv, gh, gw, 16, 16, 7).permute(0, 1, 3, 2, 4, 5).reshape(nv, gh * 16 * gw * 16 * 7)


def unshuffle_head(case, img):
    nv, gh, gw = case["S"] * case["V"], case["gh"], case["gw"]
    return img.reshape(nv, gh, 16, gw, 16, 7).permute(0, 1, 3, 2, 4, 5).reshape(nv * gh * gw, 1792)


def written(ops, outs, g):
    """what problem g left in its destination, as [M, N] in the output's type"""
    case = ops["case"]
    if case["epi"] == EPI_HEAD:
        return unshuffle_head(case, torch.stack(outs["views"]))
    v = outs["views"][g]
    return v if v.dtype == torch.float32 else v.contiguous().view(DT[ops["dt"]][1])


# ---- what the kernels write, in fp32 (prec: the precision of the products and of the epilogue's arithmetic), with the defects the host file plants
def emulate(ops, outs, prec=torch.float32, scale_after_round=False, skip_dropped=False, scene_mod=False, extra_row=False, swap_dest=False, **defect):
    """Defects: scale_after_round: T(T(v) * out_scale); skip_dropped: the scenes of EPI_HEAD contiguous; scene_mod: scene index vv % head_views; extra_row: every problem
    writes row M - 1 once more behind its rows; swap_dest: the destinations of problems 0 and 1 exchanged; and those of linear / finish."""
    case, dt = ops["case"], ops["dt"]
    lin_kw = {k: v for k, v in defect.items() if k in ("w_mod_L", "bias_unstrided", "sp_row0_zero")}
    fin_kw = {k: v for k, v in defect.items() if k in ("no_period", "start2_off", "scale_cols_off")}
    assert len(lin_kw) + len(fin_kw) == len(defect), defect
    rows = all_rows(ops)
    twin = []
    for g in range(case["P"]):
        pre = linear(ops, g, rows, prec, **lin_kw)
        twin.append(pre.float())
        v = finish(ops, round16(pre, dt).to(prec) if scale_after_round else pre, rows, prec, **fin_kw).float()
        if case["epi"] == EPI_HEAD:
            img, flat, hv = shuffle_head(case, v), outs["buf"], case["hv"]
            ve = img.shape[1]
            for vv in range(img.shape[0]):
                scene = 0 if hv == 0 or skip_dropped else (vv % hv if scene_mod else vv // hv)
                off = LEAD_E + vv * ve + scene * case["skip"]
                flat[off:off + ve] = img[vv]
            continue
        d = {0: 1, 1: 0}.get(g, g) if swap_dest else g
        o = v if case["epi"] == EPI_F32 else round16(v, dt).view(torch.int16)
        outs["views"][d][:] = o
        if extra_row:
            outs["buf"][outs["starts"][d] + case["M"]] = o[-1]
    outs["twin"] = twin


# ---- checks.  Each raises AssertionError with the relation that failed.
def _clean(t):
    return bool((t == CANARY16).all()) if t.dtype == torch.int16 else bool(torch.isnan(t).all())


def check_canaries(ops, outs):
    """Nothing but the destinations is written, and every element of those is."""
    case, buf = ops["case"], outs["buf"]
    mask = torch.zeros(buf.shape[0], dtype=torch.bool, device=buf.device)
    if case["epi"] == EPI_HEAD:
        se = outs["scene_elems"]
        for s in range(case["S"]):
            o = LEAD_E + s * (se + case["skip"])
            mask[o:o + se] = True
    else:
        for s in outs["starts"]:
            mask[s:s + case["M"]] = True
    assert _clean(buf[~mask]), "canaries in front of, behind or between the destinations overwritten"
    inside = buf[mask]
    left = (inside == CANARY16).any() if buf.dtype == torch.int16 else torch.isnan(inside).any()
    assert not bool(left), "elements of a destination not written (or NaN)"


def value_report(ops, outs, rows_of=None, emu=False):
    """dict(err: the worst ratio over the problems, abs: the worst |out - ref|, rtol, atol, problem: where) against fp64; emu: the ratio of the clean fp32 emulation
    on the same operands and device as well"""
    case = ops["case"]
    rtol, atol = bound(case, ops["dt"], ops["kernel"])
    rep = dict(err=0.0, abs=0.0, rtol=rtol, atol=atol, problem=0)
    if emu:
        rep["emu"] = 0.0
    for g in range(case["P"]):
        rows = all_rows(ops) if rows_of is None else rows_of(g).to(ops["A"].device)
        ref = reference(ops, g, rows)
        got = written(ops, outs, g)[rows].double()
        e = ratio(got, ref, rtol, atol)
        if e > rep["err"]:
            rep["err"], rep["problem"] = e, g
        d = (got - ref).abs().max().item()
        rep["abs"] = max(rep["abs"], float("inf") if d != d else d)
        if emu:
            rep["emu"] = max(rep["emu"], ratio(emulated(ops, g, rows).double(), ref, rtol, atol))
    return rep


def assert_values(rep, what=""):
    assert rep["err"] <= 1.0, (what, rep)


def check_scale_bits(ops, outs):
    """projq: out16 == T(v32 * out_scale) on the columns < scale_cols and T(v32) behind them, v32 = outs["twin"] (the fp32 twin of the launch)"""
    case, dt = ops["case"], ops["dt"]
    if case["kind"] != "projq":
        return
    sc = case["scale_cols"]
    for g, v32 in enumerate(outs["twin"]):
        want = round16(torch.cat((v32[:, :sc] * OUT_SCALE, v32[:, sc:]), dim=1), dt)
        assert torch.equal(written(ops, outs, g).view(torch.int16), want.view(torch.int16)), "out16 != T(v32 * out_scale): the scale is not applied to the fp32 value"


def outputs_equal(a, b):
    x, y = a["buf"], b["buf"]     # the whole buffers, canaries (NaN in the fp32 ones) included: as bits
    assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), "bits differ"
