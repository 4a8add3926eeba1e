"""CPU: the bounds of tests/test_attention_routes_gpu.py discriminate.  The same operands (tests/attn_routes.py), the same fp64 reference and the same
bounds; plausible wrong outputs of the attention routes emulated in fp64 must miss the bound by at least 4x.  A mutation that does not is a tolerance
to tighten or a case to add."""
import pytest
import torch

from attn_routes import (CASE, CASES, CP_CASE, DT, KT, QSCALE, abs_views, block_walk, bound, bound_p16, cp_shards, is_small, make_operands, partials,
                         reference, route_plan, sample_rows, split_tiles)
from util import rel_inf

SUBSET = ["sa_1v196_h12", "ca_update_3v196_h12", "ca_lone_12_h12", "ca_causal0_4v196_h12"]
MARGIN = 4.0


def _setup(name, dt, prescaled=1):
    case = CASE[name]
    Q, K, V, spikes = make_operands(case, dt, prescaled, "cpu")
    views = abs_views(case)
    rows = sample_rows(case, spikes)
    ref = reference(Q, K, V, views, case["heads"], prescaled, rows)
    return case, Q, K, V, views, rows, ref


def _weights(views, fn):
    return {vi: fn(vi, v) for vi, v in enumerate(views)}


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", SUBSET)
def test_mutations_exceed_the_route_bound(dt, name):
    case, Q, K, V, views, rows, ref = _setup(name, dt)
    b = bound(DT[dt][2])
    H = case["heads"]
    seen = {}

    def check(label, out):
        e = rel_inf(out, ref)
        seen[label] = e
        assert e > MARGIN * b, (label, e, b)

    # the last partial key tile dropped (views whose nk is not a multiple of 64)
    def drop_tail(vi, v):
        nk = v[3]
        if nk % KT == 0:
            return None
        w = torch.ones(nk, dtype=torch.float64)
        w[(nk // KT) * KT:] = 0
        return w
    if any(v[3] % KT for v in views):
        check("last_partial_tile", reference(Q, K, V, views, H, 1, rows, key_w=_weights(views, drop_tail)))
    # the skip range shifted by one key, either way
    if any(v[5] > v[4] for v in views):
        for d in (1, -1):
            shifted = [(a, b_, c, nk, min(max(lo + d, 0), nk), min(max(hi + d, 0), nk)) if hi > lo else (a, b_, c, nk, lo, hi)
                       for (a, b_, c, nk, lo, hi) in views]
            check(f"skip_shift{d:+d}", reference(Q, K, V, shifted, H, 1, rows))
    # one split's partial lost: every split that holds a valid key of some view, one at a time
    ns = case["nsplit"]
    for s in range(ns):
        def lose(vi, v, s=s):
            nk, lo, hi = v[3], v[4], v[5]
            t0, t1 = split_tiles(nk, ns)[s]
            w = torch.ones(nk, dtype=torch.float64)
            w[t0 * KT:min(t1 * KT, nk)] = 0
            return w
        holds = any(any(not (v[4] <= k < v[5]) for k in range(split_tiles(v[3], ns)[s][0] * KT, min(split_tiles(v[3], ns)[s][1] * KT, v[3])))
                    for v in views)
        if holds:
            check(f"split{s}_lost", reference(Q, K, V, views, H, 1, rows, key_w=_weights(views, lose)))
    # a prescaled Q scaled a second time
    check("double_scale", reference(Q, K, V, views, H, 1, rows, score_mul=QSCALE))
    print(name, dt, {k: round(v / b, 1) for k, v in seen.items()})


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("how", ["mod", "contig"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_cp_mutations_exceed_the_merge_bounds(dt, how, world):
    """CP final merge: a rank's partial counted twice (fp32 and 16-bit partials), and the 16-bit merge without the x l_s weight."""
    u = DT[dt][2]
    case = CP_CASE
    Q, K, V, spikes = make_operands(case, dt, 1, "cpu")
    views = abs_views(case)
    rows = sample_rows(case, spikes)
    H = case["heads"]
    ref = reference(Q, K, V, views, H, 1, rows)
    ref_max = ref.abs().max().item()
    shards = cp_shards(world, how)
    # the 16-bit partials of every rank, as the bound of the p16 route sees them
    parts = []
    for sh in shards:
        m_all, l_all, o_all = [], [], []
        for v in views:
            mask = torch.zeros(v[3], dtype=torch.bool)
            mask[[r for r in sh if r < v[3]]] = True
            sel = [r for r in rows if v[0] <= r < v[0] + v[1]]
            m, l, o = partials(Q, K, V, v, H, 1, sel, mask)
            m_all.append(m), l_all.append(l), o_all.append(o)
        parts.append((torch.cat(m_all), torch.cat(l_all), torch.cat(o_all)))
    pmax = max(p[2].abs().max().item() for p in parts)
    b32, b16 = bound(u), bound_p16(u, pmax, ref_max)
    for w_, sh in enumerate(shards):
        if not sh:
            continue
        kw = {}
        for vi, v in enumerate(views):
            w = torch.ones(v[3], dtype=torch.float64)
            w[[r for r in sh if r < v[3]]] = 2.0
            kw[vi] = w
        e = rel_inf(reference(Q, K, V, views, H, 1, rows, key_w=kw), ref)
        assert e > MARGIN * max(b32, b16), ("rank counted twice", w_, e, b32, b16)
    # p16 merge without the x l_s weight
    M = torch.stack([p[0] for p in parts]).max(dim=0).values
    ok = torch.isfinite(M)
    wts = [torch.where(ok, (p[0] - M).exp(), torch.zeros_like(M)) for p in parts]
    L = sum(w * p[1] for w, p in zip(wts, parts))
    acc = sum(w[..., None] * p[2] for w, p in zip(wts, parts))
    mut = torch.where(L[..., None] > 0, acc / L[..., None].clamp_min(1e-300), torch.zeros_like(acc)).view(len(rows), H * 64)
    good = sum(w[..., None] * p[1][..., None] * p[2] for w, p in zip(wts, parts))
    good = torch.where(L[..., None] > 0, good / L[..., None].clamp_min(1e-300), torch.zeros_like(good)).view(len(rows), H * 64)
    assert rel_inf(good, ref) < 1e-12   # the emulated merge itself is exact
    e = rel_inf(mut, ref)
    assert e > MARGIN * b16, ("p16 merge without l_s", e, b16)


def test_case_table_reaches_every_route_and_walk():
    """The GPU file's table launches every (route, view source) pair the decoder has -- q16 / q32 single pass, split-KV with and without dense_rows, each
    with the table and, for one-view launches, the inline view -- and both block walks, with pair counts a multiple of 8 and not."""
    hit, walks = set(), set()
    for c in CASES:
        nv, H = len(c["views"]), c["heads"]
        for (route, ns, dense, inline) in route_plan(c):
            kern = "q16" if is_small(nv, H, c["max_nq"], ns) else "q32"
            hit.add((route if route != "single" else "single_" + kern, "inline" if inline else "table"))
            npairs = nv * H * ns
            walks.add((block_walk(nv, H, ns), npairs % 8 == 0))
    for r in ("single_q16", "single_q32", "split_dense", "split_p0"):
        for src in ("table", "inline"):
            assert (r, src) in hit, (r, src)
    assert {("xcd", True), ("xcd", False), ("per-block", False)} <= walks, walks
