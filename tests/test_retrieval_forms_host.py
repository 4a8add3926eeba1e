"""CPU: the checks of tests/test_retrieval_forms_gpu.py discriminate.  The same case tables, operands, references, bounds and check functions
(tests/retrieval_forms.py): the fp32 emulation of what each kernel of csrc/retrieval.hip writes stays within every bound at every case of the GPU table, and
each planted defect exceeds its bound, or breaks its exact relation, in every case that it can reach -- a defect that no case reaches is a failure of the table.
The bitonic network of topk_kernel is emulated with the comparator as a parameter: the one before the fix misorders and indexes past N once a key is NaN (the
record of the bug, shown here and never on a GPU); the total order equals the stable descending sort on every top-k case.  Last, the symbols and the argument
refusals of the built library, which return before anything is launched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import retrieval_forms as R


def _affine_groups():
    """cases by (type, b_transposed, shape)"""
    out = {}
    for c in R.affine_cases():
        out.setdefault((c["double"], c["bt"], c["M"], c["N"], c["K"]), []).append(c)
    return out


AFFINE_GROUPS = _affine_groups()


@pytest.mark.parametrize("key", list(AFFINE_GROUPS), ids=lambda k: f"{'f64' if k[0] else 'f32'}-bt{k[1]}-{k[2]}x{k[3]}x{k[4]}")
def test_affine_emulation_and_defects(key):
    worst, seen = 0.0, {d: [] for d in R.AFFINE_DEFECTS}
    for c in AFFINE_GROUPS[key]:
        ops = R.affine_operands(c)
        rb = R.affine_ref(ops)
        dest = R.affine_dest(ops, "cpu")
        R.affine_emulate(ops, dest)
        r, fails = R.affine_check(ops, dest, rb)
        assert fails == [], (c["name"], fails)
        worst = max(worst, r)
        for d in R.AFFINE_DEFECTS:
            if not R.affine_reaches(d, c):
                continue
            dest = R.affine_dest(ops, "cpu")
            R.affine_emulate(ops, dest, d)
            rd, fails = R.affine_check(ops, dest, rb)
            seen[d].append((c["name"], rd))
            assert fails and rd > 1.0, (c["name"], d, rd)
    print(key, "clean emulation: worst |got - ref| / bound", round(worst, 4))
    for d, v in seen.items():
        print(f"  {d}: {len(v)} cases reached" + (f", smallest ratio {min(r for _, r in v):.3g}" if v else ""))


def test_affine_every_defect_is_reached_by_the_table():
    cases = R.affine_cases()
    for d in R.AFFINE_DEFECTS:
        hit = [c["name"] for c in cases if R.affine_reaches(d, c)]
        print(d, len(hit), "cases, e.g.", hit[:3])
        assert hit, d
        # both types where the defect is not one of the fp64 path alone, both layouts of B, both input kinds
        assert {c["bt"] for c in cases if R.affine_reaches(d, c)} == {0, 1}
        if d not in ("acc32", "bias_after_cast"):
            assert {c["double"] for c in cases if R.affine_reaches(d, c)} == {0, 1}


def test_row_norm_emulation_and_defect():
    worst, reached = 0.0, []
    for c in R.ROWNORM_CASES:
        ops = R.rownorm_operands(c)
        ref, bound = R.rownorm_ref(ops)
        dest = R.Guarded((c["M"],), "cpu")
        R.rownorm_emulate(ops, dest)
        r, fails = R.value_check(dest, ref, bound)
        assert fails == [], (c["name"], fails)
        worst = max(worst, r)
        if c["C"] % 64:
            dest = R.Guarded((c["M"],), "cpu")
            R.rownorm_emulate(ops, dest, "drop_cols")
            rd, fails = R.value_check(dest, ref, bound)
            reached.append((c["name"], rd))
            assert fails and rd > 1.0, (c["name"], rd)
    print("row_norm clean emulation: worst ratio", round(worst, 4), "; drop_cols reached", reached)
    assert len(reached) >= 15


def test_l2_normalize_emulation_and_defect():
    worst, reached = 0.0, []
    for c in R.L2_CASES:
        ops = R.l2_operands(c)
        shape = (c["outer"], c["L"], c["inner"])
        for in_place in (0, 1):
            dest = R.Guarded(shape, "cpu")
            if in_place:
                dest.fill(ops["x"])
            R.l2_emulate(ops["x"], dest)
            r, fails = R.l2_check(ops, dest)
            assert fails == [], (c["name"], fails)
            worst = max(worst, r)
        if c["inner"] == 1 and c["L"] % 64:
            dest = R.Guarded(shape, "cpu")
            R.l2_emulate(ops["x"], dest, "drop_cols")
            rd, fails = R.l2_check(ops, dest)
            reached.append((c["name"], rd))
            assert fails, (c["name"], rd)
    print("l2_normalize clean emulation: worst ratio", round(worst, 4), "; drop_cols reached", reached)
    assert len(reached) == 2
    # the vector kinds are all there where there are vectors enough
    ops = R.l2_operands(R.L2_CASES[2])
    n = ops["x"].double().square().sum(1).sqrt()
    assert bool((n == 0).any()) and bool(((n > 0) & (n < 1e-12)).any()) and bool((n > 1e3).any())


def test_weighted_spoc_emulation_and_defects():
    worst, seen = 0.0, {"drop_token": [], "cols256": []}
    for c in R.SPOC_CASES:
        ops = R.spoc_operands(c)
        n = (ops["feat"].double() * ops["attn"].double()[:, :, None]).sum(1).norm(dim=1)
        assert n[0] > 1e-3 and n[1] == 0 and 0 < n[2] < 5e-13, n          # the three images are what they are named
        dest = R.Guarded((3, c["C"]), "cpu")
        R.spoc_emulate(ops, dest)
        r, fails = R.spoc_check(ops, dest)
        assert fails == [], (c["name"], fails)
        worst = max(worst, r)
        for d in seen:
            if d == "cols256" and c["C"] <= 256:
                continue
            dest = R.Guarded((3, c["C"]), "cpu")
            R.spoc_emulate(ops, dest, d)
            rd, fails = R.spoc_check(ops, dest)
            seen[d].append((c["name"], rd))
            assert fails and rd > 1.0, (c["name"], d, rd)
    print("weighted_spoc clean emulation: worst ratio", round(worst, 4), "; defects reached", seen)
    assert len(seen["drop_token"]) == 4 and len(seen["cols256"]) == 2


def test_layernorm_act_emulation_and_defects():
    rows, seen = [], {"onepass": [], "mean_padded": []}
    for c in R.LN_CASES:
        ops = R.ln_operands(c)
        dest = R.Guarded((c["M"], c["C"]), "cpu")
        R.ln_emulate(ops, dest)
        fails = R.ln_check(ops, dest, rows)
        assert fails == [], (c["name"], fails)
        for d in seen:
            if not R.ln_reaches(d, ops):
                continue
            dest = R.Guarded((c["M"], c["C"]), "cpu")
            R.ln_emulate(ops, dest, d)
            fails = R.ln_check(ops, dest)
            seen[d].append(c["name"])
            assert fails, (c["name"], d)
    worst = {}
    for r in rows:
        worst[r[1]] = max(worst.get(r[1], 0.0), r[5])
    print("layernorm_act clean emulation: worst e / bound per kind", {k: round(v, 4) for k, v in worst.items()})
    print({d: len(v) for d, v in seen.items()}, "cases reached")
    assert set(worst) == set(R.LN_KINDS) and all(len(v) >= 20 for v in seen.values())


# ---- top-k
def _topk_key_sets(nan):
    for N in R.TOPK_N:
        for Bn in R.TOPK_IMAGES:
            for kind in (R.TOPK_KEYS + R.TOPK_NAN_KEYS if nan else R.TOPK_KEYS):
                yield N, Bn, kind, R.topk_keys(kind, Bn, N)


def _run_topk(feat, attn, k, **kw):
    Bn, N, Cc = feat.shape
    dests = R.topk_dests(Bn, k, Cc, "cpu")
    R.topk_emulate(feat, attn, k, dests, **kw)
    return R.topk_check(feat, attn, k, dests)


@pytest.mark.parametrize("N", R.TOPK_N)
def test_total_order_equals_the_stable_sort_on_every_case(N):
    """the network with the fixed comparator over the whole GPU table, NaN keys included: the full order first (padding last, behind a real -inf), then what the kernel
    writes for every k and C"""
    n = 0
    for Bn in R.TOPK_IMAGES:
        for kind in R.TOPK_KEYS + R.TOPK_NAN_KEYS:
            attn = R.topk_keys(kind, Bn, N)
            net = R.topk_network(attn)
            want = R.topk_expected(attn, N)
            for b in range(Bn):
                key, idx = net[b]
                assert np.array_equal(idx[:N], want[b].numpy()), (N, Bn, kind, b)
                assert bool((idx[N:] == R.PAD_IDX).all())
            for Cc in R.TOPK_C:
                feat = R.topk_feat(Bn, N, Cc)
                for k in R.topk_ks(N):
                    dests = R.topk_dests(Bn, k, Cc, "cpu")
                    R.topk_emulate(feat, attn, k, dests, net=net)
                    assert R.topk_check(feat, attn, k, dests) == [], (N, Bn, kind, Cc, k)
                    n += 1
    print("N", N, ":", n, "cases equal the stable descending sort")


def test_topk_planted_defects_are_seen_where_they_reach():
    """ties by higher index and a padding key of 0: wherever the keys say the defect reaches the first k, the check fails; where they say it does not, it passes (so the
    reach rule is exact, not merely safe)."""
    seen = {"high_index": [0, 0], "pad_zero": [0, 0]}
    for N, Bn, kind, attn in _topk_key_sets(nan=True):
        if N > 1000:
            continue
        feat = R.topk_feat(Bn, N, 4)
        for d, kw in (("high_index", dict(comparator=R.cmp_high)), ("pad_zero", dict(pad_key=0.0))):
            net = R.topk_network(attn, **kw)
            for k in R.topk_ks(N):
                reach = R.topk_reaches(d, attn, k)
                fails = _run_topk(feat, attn, k, net=net)
                seen[d][0 if reach else 1] += 1
                assert bool(fails) == reach, (d, N, Bn, kind, k, fails)
    print("top-k defects (cases reached, cases not reached):", seen)
    assert seen["high_index"][0] > 100 and seen["pad_zero"][0] > 50


def _nan_keys(N, count, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randperm(N, generator=g).float() + 1.0) * 0.25
    a[torch.randperm(N, generator=g)[:count]] = math.nan
    return a


@pytest.mark.parametrize("N,count", [(768, 1), (768, 77), (100, 1), (100, 11)])
def test_old_comparator_misorders_and_indexes_past_N(N, count):
    """The record of the bug.  `ka > kb || (ka == kb && ia < ib)` ranks a NaN key neither before nor after anything, so the network permutes without sorting: the numbers
    come out of order, and a padding slot (index 0x7fffffff) lands among the first N positions -- from where the gather read `feat + (b N + 0x7fffffff) C`.  With
    77 NaNs in 768 keys it lands below the default nfeat = 300.  The total order sorts the same keys."""
    worst_pos = N
    misordered = past = 0
    seeds = range(8)
    for seed in seeds:
        a = _nan_keys(N, count, seed)
        key, idx = R.bitonic(a.numpy(), R.cmp_old)
        nums = key[:N][~np.isnan(key[:N])]
        misordered += bool((nums[:-1] < nums[1:]).any()) or not np.array_equal(idx[:N], R.topk_expected(a[None], N)[0].numpy())
        where = np.nonzero(idx[:N] >= N)[0]
        if len(where):
            past += 1
            worst_pos = min(worst_pos, int(where[0]))
        key, idx = R.bitonic(a.numpy(), R.cmp_total)
        assert np.array_equal(idx[:N], R.topk_expected(a[None], N)[0].numpy()) and bool((idx[N:] == R.PAD_IDX).all())
    print(f"N {N}, {count} NaN keys, {len(seeds)} key sets: old comparator misorders {misordered}, puts an index >= N among the first N in {past}, earliest position {worst_pos}")
    assert misordered == len(seeds)
    assert past > 0, "no padding slot among the first N: the record needs another key set"
    if (N, count) == (768, 77):
        assert worst_pos < 300


def test_old_comparator_fails_the_check_on_the_nan_cases():
    """as a planted defect: on the table's NaN cases the check rejects what the old comparator writes -- in every case listed here, i.e. wherever the network's output
    differs from the sort (it can come out right by luck: two keys, the NaN second, is one exchange that happens to be the right one)."""
    reached, lucky = [], []
    for N in R.TOPK_N:
        if N > 1000:
            continue
        for Bn in R.TOPK_IMAGES:
            for kind in R.TOPK_NAN_KEYS:
                attn = R.topk_keys(kind, Bn, N)
                net = R.topk_network(attn, R.cmp_old)
                feat = R.topk_feat(Bn, N, 4)
                fails = _run_topk(feat, attn, N, net=net)
                (reached if fails else lucky).append((N, Bn, kind))
    print("old comparator rejected in", len(reached), "NaN cases; right by luck in", lucky)
    assert all(N <= 3 for N, _, _ in lucky), lucky                   # from 63 keys on, every NaN case shows it
    assert len(reached) >= 6 * 2 * 4


# ---- the built library: symbols and refusals (every refusal returns before a launch, so no GPU is needed)
ENTRY_POINTS = ("must3r_hip_affine", "must3r_hip_row_norm", "must3r_hip_topk_gather", "must3r_hip_weighted_spoc", "must3r_hip_l2_normalize",
                "must3r_hip_layernorm_act_f32")


def test_symbols_and_refusals():
    from must3r_amd import _lib
    lib = _lib.load()
    for n in ENTRY_POINTS:
        assert hasattr(lib, n) and n in _lib.PROTOTYPES, n
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def refused(rc, word):
        msg = lib.must3r_hip_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    refused(lib.must3r_hip_topk_gather(p, p, 1, 8, 4, 9, p, p, p, None), "topk")           # k > N
    refused(lib.must3r_hip_topk_gather(p, p, 1, 4097, 4, 8, p, p, p, None), "topk")        # N > 4096
    refused(lib.must3r_hip_topk_gather(p, p, 1, 8, 6, 4, p, p, p, None), "topk")           # C % 4
    refused(lib.must3r_hip_topk_gather(p, p, 1, 8, 0, 4, p, p, p, None), "topk")           # C <= 0
    for neg in ((-1, 8, 4, 4), (1, -8, 4, 4), (1, 8, -4, 4), (1, 8, 4, -4)):
        refused(lib.must3r_hip_topk_gather(p, p, *neg, p, p, p, None), "topk")
    refused(lib.must3r_hip_topk_gather(None, p, 1, 8, 4, 4, p, p, p, None), "topk")
    for dbl in (0, 1):
        refused(lib.must3r_hip_affine(dbl, p, None, p, 0, None, None, p, 4, 4, 0, None), "K must be positive")
        for neg in ((-1, 4, 4), (4, -1, 4), (4, 4, -1)):
            refused(lib.must3r_hip_affine(dbl, p, None, p, 0, None, None, p, *neg, None), "affine")
        refused(lib.must3r_hip_affine(dbl, None, None, p, 0, None, None, p, 4, 4, 4, None), "affine")
    refused(lib.must3r_hip_row_norm(p, -1, 4, p, None), "row_norm")
    refused(lib.must3r_hip_row_norm(p, 4, 0, p, None), "row_norm")
    refused(lib.must3r_hip_row_norm(None, 4, 4, p, None), "row_norm")
    refused(lib.must3r_hip_weighted_spoc(p, p, -1, 4, 4, p, None), "weighted_spoc")
    refused(lib.must3r_hip_weighted_spoc(p, p, 1, -4, 4, p, None), "weighted_spoc")
    refused(lib.must3r_hip_weighted_spoc(p, p, 1, 4, 0, p, None), "weighted_spoc")
    refused(lib.must3r_hip_weighted_spoc(p, None, 1, 4, 4, p, None), "weighted_spoc")
    for neg in ((-1, 4, 4), (4, -1, 4), (4, 4, -1)):
        refused(lib.must3r_hip_l2_normalize(p, neg[0], neg[1], neg[2], p, None), "l2_normalize")
    refused(lib.must3r_hip_l2_normalize(None, 4, 4, 4, p, None), "l2_normalize")
    refused(lib.must3r_hip_layernorm_act_f32(p, None, None, 1e-5, -1, 4, 0, p, None), "layernorm_act_f32")
    refused(lib.must3r_hip_layernorm_act_f32(p, None, None, 1e-5, 4, 0, 0, p, None), "layernorm_act_f32")
    refused(lib.must3r_hip_layernorm_act_f32(None, None, None, 1e-5, 4, 4, 0, p, None), "layernorm_act_f32")
    # and the empty problems are served without a launch
    assert lib.must3r_hip_topk_gather(None, None, 1, 8, 4, 0, None, None, None, None) == 0
    assert lib.must3r_hip_topk_gather(None, None, 0, 8, 4, 4, None, None, None, None) == 0
    assert lib.must3r_hip_affine(1, None, None, None, 0, None, None, None, 0, 4, 4, None) == 0
    assert lib.must3r_hip_row_norm(None, 0, 4, None, None) == 0
    assert lib.must3r_hip_l2_normalize(None, 0, 4, 4, None, None) == 0
    assert lib.must3r_hip_layernorm_act_f32(None, None, None, 1e-5, 0, 4, 0, None, None) == 0
    assert lib.must3r_hip_weighted_spoc(None, None, 0, 4, 4, None, None) == 0
