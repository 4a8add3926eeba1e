"""Shared by tests/test_layernorm_forms_gpu.py (every LayerNorm launch form of the model, through must3r_hip_op_layernorm_ex, against fp64) and
tests/test_layernorm_forms_host.py (the checks discriminate): the case table, the operands with their row kinds, the fp64 reference and the fp32
restatement, the bounds, the canary-filled output buffers, the checks, and an emulation of what the kernels write (with the defects the host file plants).
Nothing here needs a GPU.

Dispatch restated (csrc/misc.hip launch_ln_t): below 65536 rows, or with LN_ROWS = 0, one wave per row (`ln`); otherwise 2048 blocks x 4 waves = 8192 waves walk
rows r, r + 8192, ... with 3 (C <= 768) or 4 float4 chunks per lane (`ln_rows/3`, `ln_rows/4`).

Error measure: m(out, ref) = max |out - ref| / (1 + |ref|), the smallest t for which allclose(out, ref, rtol = t, atol = t) holds.
Bounds (fp32 output): benign rows 1e-5, the figure of test_ops_gpu.py::test_layernorm.  Stress rows: no fp32 evaluation reaches 1e-5 there, so the bound of a
kind is 4 x m(fp32 two-pass restatement on the CPU, fp64) over the SAME rows, floored at 1e-5; 4 x because the kernel adds lane partials and then a cross-lane
tree, another order than torch's sum.  16-bit output (u = unit round-off): out16 = round(y32) moves y32 by at most u |y32|, and |y32| <= |ref| + B (1 + |ref|) for a
y32 within the fp32 bound B, so m(out16) <= B + u (1 + B); asserted as max(2u, B + u (1 + B)) -- 2u is test_layernorm's figure and the larger one on benign rows."""
import torch

DT = {"bf16": (0, torch.bfloat16, 2.0 ** -8), "fp16": (1, torch.float16, 2.0 ** -11)}   # id, torch dtype, unit round-off
NWALK = 8192          # row-walking waves of a launch
WALK_MIN = 65536      # rows from which launch_ln_t walks
LEAD, PAD = 2, 3      # canary rows in front of / behind every output's rows: every destination is a row-offset pointer into a larger buffer
CANARY16 = 0x7E55     # fp16: a NaN; bf16: 7e37.  No output of these cases
F16_MAX = 65504.0
BENIGN, MEAN40, SPIKE, LOWVAR, CONST, BIG = range(6)
KIND_NAMES = ("benign", "mean40", "spike", "lowvar", "const", "big")
TOL_BENIGN = 1e-5
FACTOR = 4.0
ALL_OUTS = ("out16", "out16_lo", "out16_dup", "out32", "copy32", "raw16")

# the launch forms, named after their call sites in csrc/model.hip.  add: x + add; x16: 16-bit input; outs: the outputs requested; hcat: out16 | out16_lo | out16_dup are
# column blocks of one [M, ld16] buffer (ld16 = 3 C + ld_extra); big: rows beyond the fp16 range are mixed in
FORMS = {
    "plain16": dict(outs=("out16",)),
    "add_copy": dict(add=True, outs=("out16", "copy32")),
    "split": dict(outs=("out16", "out16_lo", "out32")),
    "head": dict(outs=("out16", "out16_lo", "out16_dup", "out32"), hcat=True),
    "head_wide": dict(outs=("out16", "out16_lo", "out16_dup"), hcat=True, ld_extra=8),
    "mem_norm_y": dict(add=True, outs=("out16",)),
    "mem_raw": dict(add=True, outs=("raw16",), big=True),
    "from_raw": dict(x16=True, outs=("out16",), big=True),
    "grouped": dict(add=True, outs=("out16",)),
    "feedback": dict(outs=("out16",), eps=1e-5),
}


def kernel_name(M, C, ln_rows=1):
    if not ln_rows or M < WALK_MIN:
        return "ln"
    return "ln_rows/3" if C <= 768 else "ln_rows/4"


def _case(form, M, C, R=0, add_groups=0):
    G = M // R if R else 1
    assert not R or G * R == M
    name = f"{form}-M{M}-C{C}" + (f"-R{R}-A{add_groups}" if R else "")
    return dict(name=name, form=form, M=M, C=C, R=R, G=G, add_groups=add_groups, eps=FORMS[form].get("eps", 1e-6))


def _cases():
    out = []
    # ---- one row per wave
    out += [_case(f, 1000, 768) for f in FORMS if f != "grouped"]
    out += [_case(f, 1000, 1024) for f in ("plain16", "add_copy", "split")]
    out += [_case("split", M, 768) for M in (1, 3, 4, 5, 65535)]
    out += [_case("split", 5, C) for C in (128, 200, 260, 772, 1024)]
    out += [_case("split", 1000, C) for C in (128, 200, 260, 772)]
    out += [_case("head_wide", 5, 200), _case("from_raw", 1000, 772), _case("mem_raw", 1000, 200), _case("split", 65535, 772)]
    out += [_case("grouped", 35, C, R=7, add_groups=a) for C in (768, 200) for a in (0, 4, 5)]   # a 4-row block straddles groups
    # ---- row walkers.  65536: 8 rows each; 65537, 8192 * 9 - 1, 65536 + 37: ragged last sweeps; 307200: the render batch
    out += [_case(f, 65536 + 37, 768) for f in FORMS if f != "grouped"]
    out += [_case("split", M, 768) for M in (65536, 65537, 8192 * 9 - 1)]
    out += [_case("split", 65536 + 37, C) for C in (1024, 128, 200, 260, 772)]
    out += [_case("head", 65537, 1024), _case("from_raw", 65536 + 37, 1024), _case("add_copy", 8192 * 9 - 1, 1024)]
    out += [_case(f, 307200, 768) for f in ("plain16", "head", "add_copy")]
    out += [_case("grouped", 12 * 21504, 768, R=21504, add_groups=11)]                               # the benched update (28 scenes)
    out += [_case("grouped", 12 * 5463, 768, R=5463, add_groups=a) for a in (0, 11, 12)]           # every walker changes group between steps
    out += [_case("grouped", 12 * 5463, 1024, R=5463, add_groups=11)]
    return out


CASES = _cases()
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


# ---- operands
def row_kinds(n, big, device):
    """kind of each of n rows.  Stress rows: the first and last 12, every row r = 7 mod 61 (every walker meets some, at every step), and both sides of every
    multiple of 8192 (where a walker's next row starts); the kinds cycle through them in order, a benign row among them."""
    r = torch.arange(n, device=device)
    s = (r < 12) | (r >= n - 12) | (r % 61 == 7) | ((r + 1) % NWALK < 2)
    cyc = torch.tensor([MEAN40, SPIKE, LOWVAR, CONST, BENIGN] + ([BIG] if big else []), device=device)
    return torch.where(s, cyc[(torch.cumsum(s, 0) - 1) % len(cyc)], torch.zeros_like(r))


def make_operands(case, dt, device, seed=0):
    """x (or x16) [M, C], add ([M, C], grouped: [R, C]), w / b [G, C], kinds [M].  Grouped cases place the kinds by the in-group row (add is shared by the groups), so
    the first and last rows of every group are stress rows.  Per kind, x / add:
      benign randn * 3 + 0.5 / randn (test_layernorm's rows)      mean40  benign + 120 (40 sigma)       spike  channels 1, C / 2, C - 1 x 300
      lowvar 0.5 + 3e-3 randn / 0.25 + 1e-3 randn (variance ~1e-5: eps decides)      const 1.75 / 0.5 (every sum and the mean are exact, so y == b)
      big    benign with +-1e5 and +-65504 in four channels (first and last float4 of the row); add is 0 there"""
    f = FORMS[case["form"]]
    M, C, R, G = case["M"], case["C"], case["R"], case["G"]
    tdt = DT[dt][1]
    g = torch.Generator(device=device).manual_seed(4242 + seed)

    def rn(*shape):
        return torch.randn(shape, device=device, generator=g)
    kg = row_kinds(R or M, f.get("big", False), device)     # per (in-group) row
    kinds = kg.repeat(G) if R else kg
    x = rn(M, C) * 3 + 0.5
    x[kinds == MEAN40] += 120.0
    sp = (kinds == SPIKE).nonzero().flatten()
    for c in (1, C // 2, C - 1):
        x[sp, c] *= 300.0
    lv = (kinds == LOWVAR).nonzero().flatten()
    x[lv] = 0.5 + 3e-3 * rn(lv.numel(), C)
    x[kinds == CONST] = 1.75
    bg = (kinds == BIG).nonzero().flatten()
    for c, v in ((0, 1e5), (2, -F16_MAX), (C - 3, F16_MAX), (C - 1, -1e5)):
        x[bg, c] = v
    add = None
    if f.get("add"):
        add = rn(R or M, C)
        lv = (kg == LOWVAR).nonzero().flatten()
        add[lv] = 0.25 + 1e-3 * rn(lv.numel(), C)
        add[kg == CONST] = 0.5
        bg = (kg == BIG).nonzero().flatten()
        for c in (0, 2, C - 3, C - 1):
            add[bg, c] = 0.0
    ops = dict(case=case, dt=dt, M=M, C=C, R=R, G=G, add_groups=case["add_groups"], eps=case["eps"], kinds=kinds,
               x=x, x16=None, add=add, w=rn(G, C), b=rn(G, C))
    if f.get("x16"):   # the stored rows of memory_mode 'raw': what mem_raw writes
        ops["x16"], ops["x"] = round16(x, dt, sat=True), None
    return ops


def round16(v, dt, sat=False):
    """round to nearest even into the 16-bit type; sat: fp16 clamps to +-65504 first (common.hpp cvt4_sat), bf16 has fp32's range"""
    if sat and dt == "fp16":
        v = v.clamp(-F16_MAX, F16_MAX)
    return v.to(DT[dt][1])


def with_float_input(ops):
    """the same case reading float(x16) through the fp32 input"""
    return dict(ops, x=ops["x16"].float(), x16=None)


def group_slice(ops, gi):
    """rows of group gi as an ungrouped case of its own"""
    R = ops["R"]
    sl = slice(gi * R, (gi + 1) * R)
    return dict(ops, M=R, R=0, G=1, add_groups=0, kinds=ops["kinds"][sl], x=ops["x"][sl], add=ops["add"] if gi < ops["add_groups"] else None,
                w=ops["w"][gi:gi + 1], b=ops["b"][gi:gi + 1])


# ---- the operation itself
def resolve(ops, rows, device=None, add_groups=None, add_wrong_row=False, group_shift=0):
    """input rows, add rows (or None), w and b rows of the absolute rows `rows`, moved to `device`.  Defects: add_groups overrides the case's; add_wrong_row takes add
    row (j + g) mod R for in-group row j of group g (an absolute index reads behind add's R rows in groups >= 1: another row of add stands in for what lies there);
    group_shift moves the group boundaries of w / b by that many rows."""
    R, G = ops["R"], ops["G"]
    xin = (ops["x"] if ops["x"] is not None else ops["x16"])[rows]
    add = None
    if R:
        gi = torch.div(rows, R, rounding_mode="floor")
        gw = torch.div(rows + group_shift, R, rounding_mode="floor").clamp(0, G - 1)
        w, b = ops["w"][gw], ops["b"][gw]
        if ops["add"] is not None:
            j = rows - gi * R
            if add_wrong_row:
                j = (j + gi) % R
            ag = ops["add_groups"] if add_groups is None else add_groups
            add = torch.where((gi < ag)[:, None], ops["add"][j], torch.zeros((), device=rows.device))
    else:
        w, b = ops["w"], ops["b"]
        if ops["add"] is not None:
            add = ops["add"][rows]
    if device is not None:
        xin, w, b = xin.to(device), w.to(device), b.to(device)
        add = add.to(device) if add is not None else None
    return xin, add, w, b


def ln_math(xin, add, w, b, eps, prec, onepass=False, div=None, drop_last_chunk=False):
    """(s, y) in `prec`: s = x + add, y = (s - mean) / sqrt(var + eps) * w + b with the two-pass variance.  Defects: onepass: var = E[s^2] - mean^2; div: the
    divisor of mean and variance (C); drop_last_chunk: the statistics miss the last float4 of the row."""
    C = xin.shape[1]
    s = xin.to(prec)
    if add is not None:
        s = s + add.to(prec)
    st = s[:, :C - 4] if drop_last_chunk else s
    d_ = float(div or C)
    mean = st.sum(-1, keepdim=True) / d_
    if onepass:
        var = (st * st).sum(-1, keepdim=True) / d_ - mean * mean
    else:
        var = ((st - mean) * (st - mean)).sum(-1, keepdim=True) / d_
    y = (s - mean) * torch.rsqrt(var + eps) * w.to(prec) + b.to(prec)
    return s, y


def evaluate(ops, rows, prec=torch.float64, device=None, eps=None, resolve_kw=None, **math_kw):
    xin, add, w, b = resolve(ops, rows, device, **(resolve_kw or {}))
    return ln_math(xin, add, w, b, ops["eps"] if eps is None else eps, prec, **math_kw)


def measure(out, ref):
    """per row max |out - ref| / (1 + |ref|); NaN where anything is NaN"""
    ref = ref.double()
    return ((out.double() - ref).abs() / (1.0 + ref.abs())).max(dim=1).values


def stress_bounds(ops):
    """{kind: (restatement error, bound)} of the case's stress kinds: the fp32 two-pass restatement ON THE CPU against fp64 on the same rows."""
    out = {}
    for k in range(1, len(KIND_NAMES)):
        rows = (ops["kinds"] == k).nonzero().flatten()
        if rows.numel() == 0:
            continue
        _, y32 = evaluate(ops, rows, torch.float32, "cpu")
        _, y64 = evaluate(ops, rows, torch.float64, "cpu")
        e = measure(y32, y64).max().item()
        out[k] = (e, max(TOL_BENIGN, FACTOR * e))
    return out


def bound16(B, u):
    return max(2 * u, B + u * (1 + B))


# ---- output buffers
def alloc_outputs(ops, device, form=None):
    """Every output of LnArgs, requested or not, over-allocated by LEAD rows in front and PAD behind and canary-filled (NaN / CANARY16); `form` overrides the case's
    (form "full": all six, each in a buffer of its own).  buf: the whole buffers; view: the [M, C] windows the kernel is given; req: the names passed to it."""
    f = dict(outs=ALL_OUTS) if form == "full" else FORMS[form or ops["case"]["form"]]
    M, C = ops["M"], ops["C"]
    rows = LEAD + M + PAD
    buf, view = {}, {}
    ld16 = 0
    names16 = ("out16", "out16_lo", "out16_dup", "raw16")
    if f.get("hcat"):
        ld16 = 3 * C + f.get("ld_extra", 0)
        buf["hcat"] = torch.full((rows, ld16), CANARY16, dtype=torch.int16, device=device)
        for i, n in enumerate(names16[:3]):
            view[n] = buf["hcat"][LEAD:LEAD + M, i * C:(i + 1) * C]
    for n in ALL_OUTS:
        if n in view:
            continue
        if n in names16:
            buf[n] = torch.full((rows, C), CANARY16, dtype=torch.int16, device=device)
        else:
            buf[n] = torch.full((rows, C), float("nan"), dtype=torch.float32, device=device)
        view[n] = buf[n][LEAD:LEAD + M]
    return dict(buf=buf, view=view, req=tuple(f["outs"]), ld16=ld16, hcat=bool(f.get("hcat")), dt=ops["dt"])


def as16(t, dt):
    return t.view(DT[dt][1])


def emulate(ops, outs, prec=torch.float32, chunk=16384, rows_from=None, skip_rows_from=None, lo_from_y=False, dup_stride_c=False, raw_after_mean=False,
            eps=None, resolve_kw=None, **math_kw):
    """Fill the requested outputs as the kernels do, from an evaluation in `prec` rounded to fp32: out32 = y, out16 = T(y), out16_lo = T(y - float(out16)), out16_dup =
    out16, copy32 = s, raw16 = T_sat(s).  Defects: rows_from(r): row r shows the input row rows_from(r) (its own affine parameters); skip_rows_from: rows from there
    on are not written; lo_from_y; dup_stride_c: the copy is written with row stride C into the ld16 buffer; raw_after_mean; and those of resolve / ln_math."""
    M, C, dt = ops["M"], ops["C"], ops["dt"]
    v, req = outs["view"], outs["req"]
    stop = M if skip_rows_from is None else skip_rows_from
    dev = ops["w"].device
    for r0 in range(0, stop, chunk):
        rows = torch.arange(r0, min(r0 + chunk, stop), device=dev)
        src = rows if rows_from is None else rows_from(rows)
        xin, add, _, _ = resolve(ops, src, None, **(resolve_kw or {}))
        _, _, w, b = resolve(ops, rows, None, **{k: a for k, a in (resolve_kw or {}).items() if k == "group_shift"})
        s, y = ln_math(xin, add, w, b, ops["eps"] if eps is None else eps, prec, **math_kw)
        s, y = s.float(), y.float()
        sl = slice(r0, r0 + rows.numel())
        h = round16(y, dt)
        if "out32" in req:
            v["out32"][sl] = y
        if "out16" in req:
            v["out16"][sl] = h.view(torch.int16)
        if "out16_lo" in req:
            v["out16_lo"][sl] = round16(y if lo_from_y else y - h.float(), dt).view(torch.int16)
        if "out16_dup" in req:
            if dup_stride_c and outs["hcat"]:
                flat = outs["buf"]["hcat"].view(-1)
                base = LEAD * outs["ld16"] + 2 * C
                idx = base + (rows[:, None] * C + torch.arange(C, device=dev)[None, :])
                flat[idx.clamp_max(flat.numel() - 1)] = h.view(torch.int16)
            else:
                v["out16_dup"][sl] = h.view(torch.int16)
        if "copy32" in req:
            v["copy32"][sl] = s
        if "raw16" in req:
            raw = s - s.mean(-1, keepdim=True) if raw_after_mean else s
            v["raw16"][sl] = round16(raw, dt, sat=True).view(torch.int16)


# ---- checks.  Each raises AssertionError with the relation that failed.
def check_canaries(ops, outs):
    """Nothing but the requested windows is written, and every element of those is."""
    M, C = ops["M"], ops["C"]

    def clean(t):
        return bool((t == CANARY16).all()) if t.dtype == torch.int16 else bool(torch.isnan(t).all())
    for n, t in outs["buf"].items():
        assert clean(t[:LEAD]) and clean(t[LEAD + M:]), f"{n}: rows outside [0, M) written"
        if n == "hcat":
            assert clean(t[:, 3 * C:]), "hcat: columns between 3C and ld16 written"
            for i, m in enumerate(("out16", "out16_lo", "out16_dup")):
                if m not in outs["req"]:
                    assert clean(t[:, i * C:(i + 1) * C]), f"{m}: not requested, written"
        elif n not in outs["req"]:
            assert clean(t), f"{n}: not requested, written"
    for n in outs["req"]:
        t = outs["view"][n]
        left = (t == CANARY16).any() if t.dtype == torch.int16 else torch.isnan(t).any()
        assert not bool(left), f"{n}: elements of the requested rows not written (or NaN)"


def check_bits(ops, outs, chunk=65536):
    """The relations between the outputs of one launch and its inputs; no tolerance."""
    M, dt = ops["M"], ops["dt"]
    v, req = outs["view"], outs["req"]
    dev = ops["w"].device
    if "out32" in req and "out16" in req:
        assert torch.equal(v["out16"], round16(v["out32"], dt).view(torch.int16)), "out16 != T(out32)"
    if "out16_lo" in req and "out32" in req:
        want = round16(v["out32"] - as16(v["out16"].contiguous(), dt).float(), dt)
        assert torch.equal(v["out16_lo"], want.view(torch.int16)), "out16_lo != T(out32 - float(out16))"
    if "out16_dup" in req:
        assert torch.equal(v["out16_dup"], v["out16"]), "out16_dup != out16"
    for r0 in range(0, M, chunk):
        rows = torch.arange(r0, min(r0 + chunk, M), device=dev)
        sl = slice(r0, r0 + rows.numel())
        xin, add, w, b = resolve(ops, rows)
        s = xin.float() + add if add is not None else xin.float()   # one fp32 add
        if "copy32" in req:
            assert torch.equal(v["copy32"][sl], s), "copy32 != x + add"
        if "raw16" in req:
            raw = as16(v["raw16"][sl].contiguous(), dt)
            assert torch.equal(raw.view(torch.int16), round16(s, dt, sat=True).view(torch.int16)), "raw16 != T_sat(x + add)"
            assert bool(torch.isfinite(raw.float()).all()), "raw16 holds inf / NaN"
        const = (ops["kinds"][sl] == CONST).nonzero().flatten()
        if const.numel():
            bb = b.expand(rows.numel(), -1)[const]
            if "out32" in req:
                assert torch.equal(v["out32"][sl][const], bb), "constant rows: out32 != b"
            if "out16" in req:
                assert torch.equal(v["out16"][sl][const], round16(bb, dt).view(torch.int16)), "constant rows: out16 != T(b)"


def value_report(ops, outs, chunk=16384):
    """{kind name: dict(err, bound, restated, n)} of out32 (or out16 widened) against fp64 over every row, by row kind; None when the form normalises nothing."""
    dt = ops["dt"]
    u = DT[dt][2]
    req = outs["req"]
    name = "out32" if "out32" in req else "out16" if "out16" in req else None
    if name is None:
        return None
    M = ops["M"]
    dev = ops["w"].device
    err = torch.empty(M, dtype=torch.float64, device=dev)
    for r0 in range(0, M, chunk):
        rows = torch.arange(r0, min(r0 + chunk, M), device=dev)
        _, ref = evaluate(ops, rows)
        got = outs["view"][name][r0:r0 + rows.numel()]
        got = as16(got.contiguous(), dt).float() if name != "out32" else got
        err[r0:r0 + rows.numel()] = measure(got, ref)
    sb = stress_bounds(ops)
    rep = {}
    for k, kn in enumerate(KIND_NAMES):
        m = ops["kinds"] == k
        n = int(m.sum())
        if not n:
            continue
        restated, B = sb[k] if k else (None, TOL_BENIGN)
        e = err[m]
        rep[kn] = dict(err=float("nan") if bool(torch.isnan(e).any()) else e.max().item(), bound=B if name == "out32" else bound16(B, u),
                       restated=restated, n=n, out=name)
    return rep


def assert_values(rep, what=""):
    for kn, r in (rep or {}).items():
        assert r["err"] <= r["bound"], (what, kn, r)


def outputs_equal(a, b, names=None):
    """the named outputs (default: those both launches requested) hold the same bits"""
    for n in names or [n for n in a["req"] if n in b["req"]]:
        assert torch.equal(a["view"][n], b["view"][n]), f"{n}: bits differ"
