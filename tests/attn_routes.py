"""Shared by tests/test_attention_routes_gpu.py (the routes the decoder launches, against fp64) and tests/test_attention_routes_host.py (the bounds
discriminate): the case table, the operands, the fp64 reference, the bounds, and the dispatch formulas of csrc/attention.hip restated."""
import math

import torch

DT = {"bf16": (0, torch.bfloat16, 2.0 ** -8), "fp16": (1, torch.float16, 2.0 ** -11)}   # id, torch dtype, unit round-off
QSCALE = 0.125 * 1.4426950408889634   # kQScale: the decoder's qkv / projq epilogues multiply q by 1/sqrt(64) * log2(e) before rounding
KT = 64                               # keys per tile
LEAD = 3                              # canary rows in front of every launch's rows (outside every view)


def bound(u):
    """|O - ref|_inf / |ref|_inf: P and O are rounded to 16 bit, everything else is fp32 (test_ops_gpu.py::test_attention)."""
    return 8 * u


def bound_p16(u, partial_max, ref_max):
    """Final merge of 16-bit partials (must3r_hip_cp::partial16): each rank's O_s / l_s is rounded to 16 bit once more before the merge, which forms
    the convex combination sum_s (w_s l_s / L) (O_s / l_s).  That rounding moves each term by at most u |O_s / l_s|_inf, so the combination by at
    most u max_s |O_s / l_s|_inf on top of the fp32-partial bound."""
    return bound(u) + u * partial_max / ref_max


# ---- dispatch restated (csrc/attention.hip: attention_is_small, attention_pick_split, launch_attention_phase's block walk)
def is_small(nviews, heads, max_nq, nsplit):
    return nsplit <= 1 and nviews * heads * ((max_nq + 127) // 128) < 192


def pick_split(nviews, heads, max_nq, max_nk):
    base = nviews * heads * ((max_nq + 127) // 128)
    ntiles = (max_nk + KT - 1) // KT
    if base >= 384 or ntiles < 8:
        return 1
    best, best_cost = 1, 1e30
    for s in range(1, min(ntiles // 4, 16) + 1):
        rounds = (base * s + 767) // 768
        cost = rounds * ((ntiles + s - 1) // s) + (3.0 + 0.5 * s if s > 1 else 0.0)
        if cost < best_cost:
            best, best_cost = s, cost
    return best


def kernel_name(nviews, heads, max_nq, nsplit):
    return "attn3/q16" if is_small(nviews, heads, max_nq, nsplit) else "attn3/q32"


def block_walk(nviews, heads, nsplit):
    """attn_block_coords: the (group, split) pairs dealt round-robin over the 8 XCDs, or the blocks themselves when that leaves the XCDs > 10 % apart."""
    npairs = nviews * heads * max(nsplit, 1)
    return "per-block" if ((npairs + 7) // 8) * 8 * 10 > npairs * 11 else "xcd"


def split_tiles(nk, nsplit):
    """[t_begin, t_end) key tiles of every split of one view (attn3_kernel: the split factor cuts each view's OWN tile range)."""
    ntiles = (nk + KT - 1) // KT
    tps = (ntiles + nsplit - 1) // nsplit
    return [(min(s * tps, ntiles), min(s * tps + tps, ntiles)) for s in range(nsplit)]


# ---- the case table.  views: (q_row0, nq, kv_row0, nk, skip_lo, skip_hi) relative to the launch; 'kv': q [R, D] and memory rows [K | V] (ldk = ldv = 2D) as the
# decoder's cross attention reads them; 'qkv': the fused projection's [q | k | v] rows (ldq = ldk = ldv = 3D) of its self attention.  routes: which of
# single / split_dense / split_p0 run; nsplit: the split factor of the split routes (the decoder's pick where it splits).
def _case(name, heads, layout, views, routes=("single",), nsplit=0, note=""):
    Rq = max(v[0] + v[1] for v in views)
    Rk = Rq if layout == "qkv" else max(v[2] + v[3] for v in views)
    max_nq, max_nk = max(v[1] for v in views), max(v[3] for v in views)
    if not nsplit:
        nsplit = max(pick_split(len(views), heads, max_nq, max_nk), 2)
    return dict(name=name, heads=heads, layout=layout, views=views, Rq=Rq, Rk=Rk, max_nq=max_nq, max_nk=max_nk, routes=routes, nsplit=nsplit, note=note)


def _self(nv, n):
    return [(i * n, n, i * n, n, 0, 0) for i in range(nv)]


def _update(Nm, nv, n):   # several views of one update call: old memory + the call's own new tokens, each view's own tokens excluded (model.hip decode)
    return [(i * n, n, 0, Nm + nv * n, Nm + i * n, Nm + (i + 1) * n) for i in range(nv)]


def _causal(Nm, nv, n):   # CausalMUSt3R: prefixes Nm + j n; with an empty memory view 0 attends view 1's tokens behind an excluded [0, n)
    return [(j * n, n, 0, (2 * n if (Nm == 0 and j == 0) else Nm + j * n), 0, (n if (Nm == 0 and j == 0) else 0)) for j in range(nv)]


SPLIT3 = ("single", "split_dense", "split_p0")
CASES = [
    _case("sa_1v196_h12", 12, "qkv", _self(1, 196), note="one-view update self attention: 12 groups x 4 64-row blocks, per-block walk (12 pairs)"),
    _case("sa_3v12_h12", 12, "qkv", _self(3, 12), note="nq = 12: 36 pairs, per-block walk"),
    _case("sa_8v576_h16", 16, "qkv", _self(8, 576), note="batched self attention: 640 blocks of 128 rows, q32, ragged q tail of 64, xcd walk (128 pairs)"),
    _case("sa_1v1600_h16", 16, "qkv", _self(1, 1600), note="one view that fills the chip: q32 with the inline view, 16 pairs (xcd)"),
    _case("ca_render_9v768_h12", 12, "kv", [(i * 768, 768, 0, 20 * 768, 0, 0) for i in range(9)],
          note="render cross attention over 20 x 768 memory rows: single-pass q32 (base 648 blocks), xcd walk with 108 pairs (not a multiple of 8)"),
    _case("ca_render_2v576_h16", 16, "kv", [(i * 576, 576, 0, 10 * 576, 0, 0) for i in range(2)], routes=SPLIT3,
          note="render cross attention of few views: the decoder splits (base 160 blocks)"),
    _case("ca_update_3v196_h12", 12, "kv", _update(1000, 3, 196), routes=SPLIT3,
          note="update call of 3 views over 1000 memory rows: own-token skips [1000 + 196 j, +196), not 64-aligned"),
    _case("ca_lone_768_h16", 16, "kv", [(0, 768, 0, 7 * 768, 0, 0)], routes=SPLIT3, note="lone-view update: nk = Nm, one view inline"),
    _case("ca_lone_12_h12", 12, "kv", [(0, 12, 0, 700, 0, 0)], routes=SPLIT3, nsplit=5,
          note="nq = 12 alone: 11 tiles in 5 splits of 3 -- the last split is empty"),
    _case("ca_causal0_4v196_h12", 12, "kv", _causal(0, 4, 196), routes=SPLIT3, nsplit=5,
          note="causal, empty memory: view 0 nk = 2n behind [0, n), views j nk = j n -- mixed nk, split 0 of view 0 only skipped keys, empty splits"),
    _case("ca_causal_3v768_h16", 16, "kv", _causal(1536, 3, 768), routes=SPLIT3, note="causal prefixes nk = Nm + j n"),
]
CASE = {c["name"]: c for c in CASES}


def route_plan(case):
    """(route, nsplit, dense_rows, inline) launches of a case: every route of the case, with the table and -- one-view cases -- the inline view."""
    out = []
    for r in case["routes"]:
        ns = 1 if r == "single" else case["nsplit"]
        for inline in ((False, True) if len(case["views"]) == 1 else (False,)):
            out.append((r, ns, 1 if r == "split_dense" else 0, inline))
    return out


# ---- operands
def make_operands(case, dt, prescaled, device, seed=0):
    """16-bit Q, K, V with LEAD canary rows in front (and 2 behind) of the launch's rows.  q = randn * 1.5 in fp32; with q_prescaled the decoder's epilogue
    is reproduced: Q = T(fp32(q * QSCALE)).  Planted key pairs: for a set of probe keys j of every view (tile, split and skip boundaries, the last key) one
    query row i of the view gets two keys j, j' equal to q_i -- a score ~26 log2 units above the rest -- with V[j'] = -V[j].  Where both count, row i is ~0;
    dropping, adding or re-weighting either one moves row i by |v_j|: the mutations the route tests must see."""
    heads, D = case["heads"], case["heads"] * 64
    tdt = DT[dt][1]
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    Rq, Rk = case["Rq"] + LEAD + 2, case["Rk"] + (LEAD + 2 if case["layout"] == "qkv" else 0)
    q = torch.randn((Rq, D), device=device, generator=g) * 1.5
    k = torch.randn((Rk, D), device=device, generator=g) * 1.5
    v = torch.randn((Rk, D), device=device, generator=g) * 1.5
    planted, spike_rows = set(), []
    for (q0, nq, k0, nk, slo, shi) in abs_views(case):
        if nk == 0:
            continue
        probes = probe_keys(nk, slo, shi, case["nsplit"])
        for p, j in enumerate(probes):
            if j in planted:
                continue
            jp = _partner(j, nk, slo, shi, planted | set(probes))
            if jp is None:
                continue
            i = (p * 37 + 5) % nq
            k[k0 + j] = q[q0 + i]
            k[k0 + jp] = q[q0 + i]
            v[k0 + jp] = -v[k0 + j]
            planted |= {j, jp}
            spike_rows.append(q0 + i)
    Q = (q * QSCALE).to(tdt) if prescaled else q.to(tdt)
    K, V = k.to(tdt), v.to(tdt)
    if case["layout"] == "qkv":
        qkv = torch.cat([Q, K, V], dim=1)
        Q, K, V = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    else:
        kvm = torch.cat([K, V], dim=1)
        K, V = kvm[:, :D], kvm[:, D:]
    return Q, K, V, sorted(set(spike_rows))


def abs_views(case):
    """views in the operand tensors (LEAD canary rows in front of the q rows; of the k rows too for 'qkv')."""
    kq = LEAD if case["layout"] == "qkv" else 0
    return [(q0 + LEAD, nq, k0 + kq, nk, slo, shi) for (q0, nq, k0, nk, slo, shi) in case["views"]]


def probe_keys(nk, slo, shi, nsplit):
    ks = {0, KT - 1, KT, nk - 1, ((nk - 1) // KT) * KT}
    if shi > slo:
        ks |= {slo - 1, slo, shi - 1, shi}
    for (t0, t1) in split_tiles(nk, nsplit):
        if t1 > t0:
            ks |= {t0 * KT, t1 * KT - 1}
    return sorted(j for j in ks if 0 <= j < nk)


def _partner(j, nk, slo, shi, avoid):
    for d in range(nk):
        c = (j + nk // 2 + d) % nk
        if not (slo <= c < shi) and c not in avoid and c != j:
            return c
    return None


# ---- rows checked against fp64
def sample_rows(case, spike_rows, full_limit=4e8):
    """every row when the launch is small; else every planted row, the first and last row of every 64-row block (the 16-row form's block; two per
    128-row block), every row of a ragged 128-row tail and 8 fixed rows per view."""
    views = abs_views(case)
    work = sum(nq * max(nk, 1) for (_, nq, _, nk, _, _) in views) * case["heads"]
    rows = set()
    for (q0, nq, _, _, _, _) in views:
        if work <= full_limit:
            rows |= set(range(q0, q0 + nq))
            continue
        for b in range(0, nq, 64):
            rows |= {q0 + b, q0 + min(b + 63, nq - 1)}
        tail = nq % 128
        if tail:
            rows |= set(range(q0 + nq - tail, q0 + nq))
        rows |= {q0 + (r * 97 + 11) % nq for r in range(8)}
    rows |= set(spike_rows)
    return sorted(rows)


def reference(Q, K, V, views, heads, prescaled, rows, key_w=None, score_mul=1.0):
    """fp64 attention of the 16-bit operands for the given absolute rows -> [len(rows), heads * 64].  prescaled: softmax_2(Q K^T) over the exact products of
    the rounded operands (the scale is in Q); else softmax(Q K^T / 8).  key_w: per view an optional fp64 weight per key (0 drops a key, 2 counts it twice)
    on top of the skip range; score_mul: scales the scores (a mutation).  A row without any valid key is 0."""
    dev = Q.device
    rows_t = torch.tensor(rows, dtype=torch.long, device=dev)
    out = torch.zeros((len(rows), heads * 64), dtype=torch.float64, device=dev)
    for vi, (q0, nq, k0, nk, slo, shi) in enumerate(views):
        sel = ((rows_t >= q0) & (rows_t < q0 + nq)).nonzero().flatten()
        if sel.numel() == 0 or nk == 0:
            continue
        w = torch.ones(nk, dtype=torch.float64, device=dev)
        w[slo:shi] = 0
        if key_w is not None and key_w.get(vi) is not None:
            w = w * key_w[vi].to(dev)
        if not (w > 0).any():
            continue
        logw = torch.where(w > 0, w.log(), torch.full_like(w, -math.inf))
        qq = Q[rows_t[sel]].double().view(-1, heads, 64)
        kk = K[k0:k0 + nk].double().view(nk, heads, 64)
        vv = V[k0:k0 + nk].double().view(nk, heads, 64)
        for h in range(heads):
            s = qq[:, h] @ kk[:, h].t() * score_mul
            s = s * math.log(2.0) if prescaled else s / 8.0
            p = torch.softmax(s + logw, dim=-1)
            out[sel, h * 64:(h + 1) * 64] = p @ vv[:, h]
    return out


def partials(Q, K, V, view, heads, prescaled, rows, key_mask):
    """fp64 flash partial of one view's rows over the keys in key_mask: (m natural log domain, l, O / l) per row and head."""
    q0, nq, k0, nk, slo, shi = view
    dev = Q.device
    keep = key_mask.clone().to(dev)
    keep[slo:shi] = False
    rows_t = torch.tensor(rows, dtype=torch.long, device=dev)
    n = len(rows)
    m = torch.full((n, heads), -math.inf, dtype=torch.float64, device=dev)
    l = torch.zeros((n, heads), dtype=torch.float64, device=dev)
    o = torch.zeros((n, heads, 64), dtype=torch.float64, device=dev)
    if keep.any():
        qq = Q[rows_t].double().view(n, heads, 64)
        kk = K[k0:k0 + nk].double().view(nk, heads, 64)[keep]
        vv = V[k0:k0 + nk].double().view(nk, heads, 64)[keep]
        for h in range(heads):
            s = qq[:, h] @ kk[:, h].t()
            s = s * math.log(2.0) if prescaled else s / 8.0
            m[:, h] = s.max(dim=1).values
            e = (s - m[:, h:h + 1]).exp()
            l[:, h] = e.sum(dim=1)
            o[:, h] = (e @ vv[:, h]) / l[:, h:h + 1]
    return m, l, o


# ---- context parallel: a memory of labelled rows (n tokens per label, as the memory update appends views) sharded over `world` ranks
CP_HEADS, CP_N, CP_LABELS = 12, 196, 5
CP_NM = CP_N * CP_LABELS
# views of the CP launch: every view attends a PREFIX of the memory (a rank's local rows of a prefix are a prefix of its local rows); view 1 sees
# label 0 only, so every rank but label 0's holds none of its keys
CP_VIEWS = [(0, CP_N, 0, CP_NM, 0, 0), (CP_N, CP_N, 0, CP_N, 0, 0), (2 * CP_N, 100, 0, 3 * CP_N, 0, 0)]
CP_CONTIG = {1: [CP_NM], 2: [784, 196], 3: [300, 0, 680], 4: [196, 392, 0, 392]}   # contiguous shard sizes (a rank with no keys in W = 3, 4)


def cp_shards(world, how):
    """list over ranks of the global memory rows each holds, in order"""
    if how == "mod":
        return [[r for r in range(CP_NM) if (r // CP_N) % world == w] for w in range(world)]
    out, r0 = [], 0
    for n in CP_CONTIG[world]:
        out.append(list(range(r0, r0 + n)))
        r0 += n
    return out


CP_CASE = _case("cp_3v_h12", CP_HEADS, "kv", CP_VIEWS, routes=("split_dense",), nsplit=2)
