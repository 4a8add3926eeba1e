"""GPU (-m gpu): the attention routes the decoder launches, through must3r_hip_op_attention_ex (ABI 10), against fp64 evaluations of the same 16-bit
operands (tests/attn_routes.py: case table, operands, reference, bounds).  Covered: the 16- and 32-row single pass, split-KV with and without
dense_rows, q_prescaled 0 / 1, the view table and the inline view, bf16 / fp16, both block walks, canary rows and columns, the context-parallel
stages for worlds 1-4, ATTN_LZ = 0, run-to-run bits and rows whose view has no valid key."""
import ctypes as C

import pytest
import torch

from attn_routes import (CASE, CASES, CP_CASE, CP_VIEWS, DT, LEAD, abs_views, block_walk, bound, bound_p16, cp_shards, kernel_name,
                         make_operands, pick_split, reference, route_plan, sample_rows)
from test_ops_gpu import record   # the suite's one metrics log
from util import rel_inf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from must3r_amd import _lib
    return _lib


def P(t):
    return t.data_ptr() if t is not None else None


def launch(lib, dt, Q, K, V, O, heads, views, *, stage=0, nsplit=1, dense=0, inline=False, prescaled=1, total_q_rows=0, max_nk=0,
           slot_o=None, slot_ml=None, p16=0, nslots=0, stride_o=0, stride_ml=0, scratch=None):
    """one must3r_hip_op_attention_ex call on the current stream; returns the main kernel it reports (stages 0 / 1)"""
    L = lib.load()
    d = lib.AttnOp()
    d.dtype = DT[dt][0]
    d.Q, d.K, d.V, d.O = P(Q), P(K), P(V), P(O)
    d.ldq, d.ldk, d.ldv = Q.stride(0), K.stride(0), V.stride(0)
    d.ldo = O.stride(0) if O is not None else 0
    d.heads = heads
    tab = None
    if inline:
        d.view0_inline = 1
        d.view0 = (C.c_int32 * 6)(*views[0])
    else:
        tab = torch.tensor(views, dtype=torch.int32, device="cuda")
        d.views_dev = tab.data_ptr()
    d.n_views = len(views)
    d.max_nq = max(v[1] for v in views)
    d.max_nk = max_nk
    d.q_prescaled = prescaled
    d.nsplit = nsplit
    d.total_q_rows = total_q_rows or max(v[0] + v[1] for v in views)
    if nsplit > 1 and scratch is None:
        scratch = torch.empty((L.must3r_hip_attention_scratch_bytes(nsplit, d.total_q_rows, heads),), dtype=torch.uint8, device="cuda")
    d.scratch = P(scratch)
    d.dense_rows = dense
    d.stage = stage
    d.slot_o, d.slot_ml = P(slot_o), P(slot_ml)
    d.p16, d.nslots, d.stride_o, d.stride_ml = p16, nslots, stride_o, stride_ml
    picked = C.c_char_p()
    d.picked = C.pointer(picked)
    lib.check(L.must3r_hip_op_attention_ex(C.byref(d), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return picked.value.decode() if picked.value else None


def run_route(lib, case, dt, prescaled, Q, K, V, route, ns, dense, inline):
    """One launch of a route into a NaN-filled O with ldo > D.  dense_rows: the launch starts at row LEAD (its rows are exactly the views' rows); otherwise
    the views carry the LEAD offset, so rows 0 .. LEAD-1 lie below total_q_rows in no view (the pre-fill must keep them untouched)."""
    H, D = case["heads"], case["heads"] * 64
    O = torch.full((Q.shape[0], D + 32), float("nan"), dtype=DT[dt][1], device="cuda")
    if dense:
        kq = LEAD if case["layout"] == "qkv" else 0
        args = (Q[LEAD:], K[kq:], V[kq:], O[LEAD:], case["views"])
    else:
        args = (Q, K, V, O, abs_views(case))
    picked = launch(lib, dt, *args[:4], H, args[4], nsplit=ns, dense=dense, inline=inline, prescaled=prescaled, max_nk=case["max_nk"])
    return O, picked


def check_canaries(O, case):
    D = case["heads"] * 64
    assert torch.isnan(O[:, D:].float()).all(), "padding columns written"
    inside = torch.zeros(O.shape[0], dtype=torch.bool)
    for (q0, nq, _, _, _, _) in abs_views(case):
        inside[q0:q0 + nq] = True
    assert torch.isnan(O[~inside.cuda()].float()).all(), "rows outside every view written"
    assert torch.isfinite(O[inside.cuda(), :D].float()).all()


@pytest.mark.parametrize("prescaled", [1, 0])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_route_against_fp64(lib, name, dt, prescaled):
    """Every route of the case (single pass: the 16- or 32-row form by attention_is_small; split-KV with dense_rows = 1 as the decoder, and with the (m, l)
    pre-fill), with the view table and -- one-view cases -- the inline view: within 8u of fp64 on the sampled rows, the kernel the dispatch formula names,
    canaries intact, and the same bits from a second launch."""
    case = CASE[name]
    H, D, nv = case["heads"], case["heads"] * 64, len(case["views"])
    u = DT[dt][2]
    Q, K, V, spikes = make_operands(case, dt, prescaled, "cuda")
    rows = sample_rows(case, spikes)
    ref = reference(Q, K, V, abs_views(case), H, prescaled, rows)
    rows_t = torch.tensor(rows, device="cuda")
    errs = {}
    for (route, ns, dense, inline) in route_plan(case):
        O, picked = run_route(lib, case, dt, prescaled, Q, K, V, route, ns, dense, inline)
        assert picked == kernel_name(nv, H, case["max_nq"], ns), (route, picked)
        check_canaries(O, case)
        e = rel_inf(O[rows_t, :D], ref)
        tag = f"{route}{'/inline' if inline else ''}"
        errs[tag] = dict(err=e, kernel=picked, nsplit=ns, walk=block_walk(nv, H, ns), npairs=nv * H * ns)
        assert e < bound(u), (tag, e)
        O2, _ = run_route(lib, case, dt, prescaled, Q, K, V, route, ns, dense, inline)
        assert torch.equal(O.view(torch.int16), O2.view(torch.int16)), (tag, "run-to-run bits")
    record("attention_route", case=name, dt=dt, prescaled=prescaled, rows=len(rows), routes=errs)


def test_decoder_split_factors_are_the_launched_ones():
    """The split routes of the decoder-shaped cases run the factor decode() picks (model.hip: attention_pick_split, >= 2), except where a case names
    its own to make splits of a short view empty."""
    for c in CASES:
        if "split_dense" in c["routes"] and c["name"] not in ("ca_lone_12_h12", "ca_causal0_4v196_h12"):
            assert c["nsplit"] == max(pick_split(len(c["views"]), c["heads"], c["max_nq"], c["max_nk"]), 2), c["name"]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attn_lz0_single_pass(lib, dt):
    """M3R_ATTN_LZ = 0 (the references move on per-lane score maxima instead of tile row sums) on the single-pass cases: within 8u of fp64.  The bits differ
    from LZ = 1 (measured on every case: P = 2^(s - m) is rounded against other references m), so only the bound is asserted (options.hpp)."""
    u = DT[dt][2]
    out = {}
    try:
        for name in ("sa_1v196_h12", "sa_8v576_h16", "ca_update_3v196_h12", "ca_causal0_4v196_h12"):
            case = CASE[name]
            H, D = case["heads"], case["heads"] * 64
            Q, K, V, spikes = make_operands(case, dt, 1, "cuda")
            rows = sample_rows(case, spikes)
            rows_t = torch.tensor(rows, device="cuda")
            ref = reference(Q, K, V, abs_views(case), H, 1, rows)
            lib.set_option("ATTN_LZ", 1)
            O1, _ = run_route(lib, case, dt, 1, Q, K, V, "single", 1, 0, False)
            lib.set_option("ATTN_LZ", 0)
            O0, _ = run_route(lib, case, dt, 1, Q, K, V, "single", 1, 0, False)
            check_canaries(O0, case)
            e0, e1 = rel_inf(O0[rows_t, :D], ref), rel_inf(O1[rows_t, :D], ref)
            same = torch.equal(O0.view(torch.int16), O1.view(torch.int16))
            out[name] = dict(err_lz0=e0, err_lz1=e1, same_bits=same)
            assert e0 < bound(u), (name, e0)
    finally:
        lib.set_option("ATTN_LZ", 1)
    record("attention_lz0", dt=dt, cases=out)


def _edge_views():
    # view 1: every key excluded; view 2: no key at all; view 0 ordinary
    return [(0, 64, 0, 300, 0, 0), (64, 70, 0, 200, 0, 200), (134, 20, 0, 0, 0, 0)]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_rows_without_a_valid_key_are_zero_on_every_route(lib, dt):
    """A query row whose view has no valid key gets O = 0 on every route (include/must3r_hip.h, must3r_hip_op_attention_ex)."""
    heads, D = 2, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    tdt, u = DT[dt][1], DT[dt][2]
    Q = (torch.randn((160, D), device="cuda", generator=g) * 0.2).to(tdt)
    kv = (torch.randn((300, 2 * D), device="cuda", generator=g) * 1.5).to(tdt)
    K, V = kv[:, :D], kv[:, D:]
    views = _edge_views()
    ref = reference(Q, K, V, views, heads, 1, list(range(64)))
    res = {}
    for (ns, dense) in ((1, 0), (3, 1), (3, 0)):
        for vs, inline in ((views, False), ([(0, 70, 0, 200, 0, 200)], True), ([(0, 20, 0, 0, 0, 0)], True)):
            O = torch.full((160, D + 32), float("nan"), dtype=tdt, device="cuda")
            launch(lib, dt, Q, K, V, O, heads, vs, nsplit=ns, dense=dense, inline=inline, max_nk=300)
            for (q0, nq, _, nk, lo, hi) in vs:
                blk = O[q0:q0 + nq, :D]
                if nk == 0 or (lo == 0 and hi >= nk):
                    assert torch.equal(blk.float(), torch.zeros_like(blk.float())), (ns, dense, inline, (q0, nq, nk))
                else:
                    e = rel_inf(blk, ref)
                    assert e < bound(u), e
            res[f"ns{ns}_dense{dense}_{'inline' if inline else 'table'}_{len(vs)}"] = "zero"
    # context parallel: no rank holds a key of views 1 and 2 -> the final merge writes zeros as well
    _cp_run(lib, dt, Q, K, V, heads, views, [list(range(150)), list(range(150, 300))], p16=0, check_zero_rows=[(64, 154)])
    record("attention_no_valid_key", dt=dt, routes=res)


def _cp_run(lib, dt, Q, K, V, heads, views, shards, p16, check_zero_rows=(), scratch_ns=None):
    """Stages 1 / 2 per rank into slots at a stride larger than the dense default, stage 3 into O (ldo > D).  Returns O, the slots and the kernels."""
    D = heads * 64
    R = max(v[0] + v[1] for v in views)
    tdt = DT[dt][1]
    so = R * D + 256                     # elements of the partial's O type between slots (dense default: R * D)
    sm = R * heads * 2 + 64              # floats
    W = len(shards)
    slot_o = torch.full((W * so,), float("nan"), dtype=tdt if p16 else torch.float32, device="cuda")
    slot_ml = torch.full((W * sm,), float("nan"), dtype=torch.float32, device="cuda")
    kernels = []
    for w, sh in enumerate(shards):
        lv = [(q0, nq, 0, sum(1 for r in sh if r < nk), lo, hi) for (q0, nq, _, nk, lo, hi) in views]
        if sh:
            idx = torch.tensor(sh, device="cuda")
            Kl, Vl = K[idx].contiguous(), V[idx].contiguous()
            kvl = torch.cat([Kl, Vl], dim=1)
            Kl, Vl = kvl[:, :D], kvl[:, D:]
            ns = scratch_ns or max(pick_split(len(lv), heads, max(v[1] for v in lv), max(v[3] for v in lv)), 2)
            kernels.append(launch(lib, dt, Q, Kl, Vl, None, heads, lv, stage=1, nsplit=ns, dense=1, total_q_rows=R, max_nk=len(sh),
                                  slot_o=slot_o[w * so:], slot_ml=slot_ml[w * sm:], p16=p16))
        else:
            launch(lib, dt, Q, K, V, None, heads, lv, stage=2, total_q_rows=R, slot_o=slot_o[w * so:], slot_ml=slot_ml[w * sm:], p16=p16)
            assert torch.equal(slot_o[w * so:w * so + R * D].float(), torch.zeros(R * D, device="cuda"))
            ml = slot_ml[w * sm:w * sm + R * heads * 2].view(-1, 2)
            assert torch.isneginf(ml[:, 0]).all() and (ml[:, 1] == 0).all()
            kernels.append("empty")
    O = torch.full((R + 2, D + 32), float("nan"), dtype=tdt, device="cuda")
    launch(lib, dt, Q, K, V, O, heads, views, stage=3, total_q_rows=R, dense=1, slot_o=slot_o, slot_ml=slot_ml, p16=p16, nslots=W,
           stride_o=so, stride_ml=sm)
    assert torch.isnan(O[:, D:].float()).all() and torch.isnan(O[R:].float()).all()
    for (a, b) in check_zero_rows:
        assert torch.equal(O[a:b, :D].float(), torch.zeros_like(O[a:b, :D].float()))
    return O, slot_o, slot_ml, so, kernels


@pytest.mark.parametrize("p16", [0, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("how", ["mod", "contig"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_context_parallel_merge(lib, world, how, dt, p16):
    """A memory of 5 labelled views sharded over W ranks by label modulo or contiguously (a rank with no keys at W = 3, 4 contiguous: stage 2; view 1 sees label
    0 only, so most ranks hold none of its keys); per rank stage 1 into a slot, then the final merge (stage 3) against fp64 over all keys.  Bound: 8u with fp32
    partials; with 16-bit partials bound_p16 (one more rounding of O_s / l_s per partial).  Stages run twice give the same bits."""
    case = CP_CASE
    H, D = case["heads"], case["heads"] * 64
    u = DT[dt][2]
    Q, K, V, spikes = make_operands(case, dt, 1, "cuda")
    views = CP_VIEWS
    shards = cp_shards(world, how)
    rows = sample_rows(case, spikes)
    # the operands carry LEAD rows in front of the q rows: the CP launch uses the plain views on Q[LEAD:]
    Qv = Q[LEAD:]
    ref = reference(Qv, K, V, views, H, 1, [r - LEAD for r in rows])
    rows_t = torch.tensor([r - LEAD for r in rows], device="cuda")
    O, slot_o, slot_ml, so, kernels = _cp_run(lib, dt, Qv, K, V, H, views, shards, p16)
    e = rel_inf(O[rows_t, :D], ref)
    R = max(v[0] + v[1] for v in views)
    if p16:
        pmax = max(slot_o[w * so:w * so + R * D].float().abs().max().item() for w in range(world))
        b = bound_p16(u, pmax, ref.abs().max().item())
    else:
        b = bound(u)
    O2, slot_o2, slot_ml2, _, _ = _cp_run(lib, dt, Qv, K, V, H, views, shards, p16)
    assert torch.equal(slot_o.view(torch.int8) if p16 else slot_o.view(torch.int32), slot_o2.view(torch.int8) if p16 else slot_o2.view(torch.int32))
    assert torch.equal(slot_ml.view(torch.int32), slot_ml2.view(torch.int32))
    assert torch.equal(O.view(torch.int16), O2.view(torch.int16)), "run-to-run bits"
    record("attention_cp", world=world, how=how, dt=dt, p16=p16, err=e, bound=b, shard_sizes=[len(s) for s in shards], kernels=kernels)
    assert e < b, (e, b)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_one_fp32_slot_is_phase2_bits(lib, dt):
    """kernels.hpp: one fp32 slot through the final merge reproduces bit for bit what phase 2 of the same split launch writes."""
    case = CP_CASE
    H, D = case["heads"], case["heads"] * 64
    Q, K, V, _ = make_operands(case, dt, 1, "cuda")
    Qv = Q[LEAD:]
    views = CP_VIEWS
    R = max(v[0] + v[1] for v in views)
    for ns in (2, 5):
        O, _, _, _, _ = _cp_run(lib, dt, Qv, K, V, H, views, [list(range(K.shape[0]))], 0, scratch_ns=ns)
        O0 = torch.full((R + 2, D + 32), float("nan"), dtype=DT[dt][1], device="cuda")
        launch(lib, dt, Qv, K, V, O0, H, views, stage=0, nsplit=ns, dense=1, max_nk=K.shape[0])
        assert torch.equal(O.view(torch.int16), O0.view(torch.int16)), ns
