"""CPU: the checks of tests/test_lnfold_forms_gpu.py discriminate.  The same operands, reference, bounds and check functions (tests/lnfold_forms.py).  The clean fp32
emulation of what the kernels write stays within HALF of every bound on every case, the constants of the consumer bound are the smallest powers of two for which it does,
the bound stays inside twice the unfolded 16-bit bounds on the rows with kappa <= 2, and each plausible defect of the fold (mu from 47 of the 48 fragments, tail rows
reading row M - 1's statistics, s_n dropped in one column tile, the shift added twice, ln_shift_init ignored, eps dropped on the constant row, x16 rounded from x where
x - shift belongs) fails at least one case.  The chain of three blocks passes under the emulation in both weight modes."""
import pytest
import torch

import lnfold_forms as F

_clean = {}


def _consumer(name, **defect):
    key = (name, tuple(sorted(defect.items())))
    if defect or key not in _clean:
        ops = F.make_consumer(F.CASE[name])
        outs = F.alloc_consumer(ops)
        F.emulate(F.consumer_op(ops, outs), **defect)
        if defect:
            return ops, outs
        _clean[key] = (ops, outs, F.consumer_reference(ops))
    return _clean[key]


def test_case_table_reaches_every_form_and_kernel():
    want_c = {"g64/e2/w2/n64", "g48k128/e0/w2/n48", "g96/e1/w2/n96", "g64/e1/w1/n64"}
    assert {F.kernel_of(c) for c in F.CCASES} == want_c
    assert F.consumer_kernel(F.EPI_STORE16, "split", bk128=0) == "g48/e0/w2/n48"
    fams = {(c["form"], c["weights"], F.kernel_of(c).split("/")[0]) for c in F.PCASES}
    for form, w in (("embed", "plain"), ("proj", "split"), ("fc2", "split"), ("fc2", "plain"), ("fc2_last", "split"), ("fc2_last", "plain")):
        assert {(form, w, "g64p"), (form, w, "g48k128")} <= fams, (form, w)
    assert not [c for c in F.PCASES if F.kernel_of(c).split("/")[0] not in ("g64p", "g64", "g48", "g48k128", "g96")]   # never the 256-row, g128 or sparse kernels
    for M in F.MS:   # the ragged last tiles the module's docstring states
        assert [M % bm for bm in (48, 64, 96)] == {12: [12, 12, 12], 196: [4, 4, 4], 700: [28, 60, 28], 768: [0, 0, 0], 1024: [16, 0, 64]}[M]
    x, shift = F.make_rows(26, 0)
    kap = F.kappa(x - shift[:, None])
    K = {n: i for i, n in enumerate(F.KINDS)}
    assert kap[K["benign_exact"]] < 1.001 and kap[K["benign_stale"]] < 1.1 and 9 < kap[K["off10_none"]] < 11 and 35 < kap[K["off40_none"]] < 45
    assert kap[K["off40_5pct"]] > 2 and kap[K["constant"]] == 1 and float((x - shift[:, None])[K["saturate"]].abs().max()) > 65504
    assert F.kappa(F.make_rows(26, 0, unshifted=True)[0])[K["tiny_sigma"]] > F.KAPPA_CONTRACT


@pytest.mark.parametrize("name", [c["name"] for c in F.CCASES])
def test_clean_consumer_emulation_stays_within_half_of_the_bound(name):
    ops, outs, R = _consumer(name)
    rep = F.check_consumer(ops, outs, R)
    print(name, rep)
    assert rep["err"] <= 0.5 and rep["out_of_contract"] <= 0.5 and rep["shift"] <= 0.5, rep
    low = R["kappa"] <= 2      # the bound does not hide a failure of the well-conditioned rows
    assert bool(low.any()) and float((R["bound"][low] / F.unfolded_bound(ops["case"], R["ref"])[low]).max()) <= 1.0
    assert rep["kappa_max"] > 35 and set(rep["kinds"]) >= set(F.KINDS[:min(ops["case"]["M"], 10)])


def test_the_constants_are_the_smallest_powers_of_two():
    """C_R = C_V = 1 is the floor; with C_A / 2 (and with C_V_OUT / 2) the emulation leaves half of the bound on some case"""
    assert F.C_R == 1.0 and F.C_V == 1.0
    worst_a, worst_v = 0.0, 0.0
    for c in F.CCASES:
        ops, outs, R = _consumer(c["name"])
        rep = F.check_consumer(ops, outs, R)
        worst_v = max(worst_v, rep["out_of_contract"])
        try:
            F.C_A /= 2
            worst_a = max(worst_a, F.check_consumer(ops, outs)["err"])
        finally:
            F.C_A *= 2
    assert worst_a > 0.5 and 0.25 < worst_v <= 0.5, (worst_a, worst_v)


@pytest.mark.parametrize("name", [c["name"] for c in F.PCASES])
def test_clean_producer_emulation_stays_within_half_of_the_bound(name):
    ops = F.make_producer(F.CASE[name])
    outs = F.alloc_producer(ops)
    F.emulate(F.producer_op(ops, outs))
    rep = F.check_producer(ops, outs)
    print(name, ops["kernel"], rep)
    assert rep["err"] <= 0.5 and rep["s1"] <= 0.5 and rep["s2"] <= 0.5, rep
    if ops["case"]["fold"] and ops["case"]["M"] > 12 and (ops["case"]["epi"] == F.EPI_RESID_F32 or ops["case"]["K"] == 256):   # a value beyond the fp16 range, saturated
        assert int((outs["x16"].view(torch.float16).float().abs() == 65504.0).sum()) > 0


def _rejected(names, **defect):
    caught = []
    for n in names:
        ops, outs = _consumer(n, **defect)
        try:
            F.check_consumer(ops, outs)
        except AssertionError as e:
            caught.append((n, str(e)[:60]))
    return caught


RAGGED = ["qkv-split-M196", "projq-split-M700", "fc1-split-M1024", "fc1-plain-M196"]


def test_wrong_row_statistics_are_rejected():
    assert len(_rejected(["qkv-split-M12", "projq-split-M196", "fc1-plain-M196"], frags47=True)) == 3
    for n in RAGGED:   # the tile height of the kernel the case runs
        bm = {"g64": 64, "g48k128": 48, "g96": 96}[F.kernel_of(F.CASE[n]).split("/")[0]]
        assert _rejected([n], tail_stats=bm), n
    assert _rejected(["fc1-split-M12"], no_eps=True) and "finite" in _rejected(["fc1-split-M12"], no_eps=True)[0][1]


def test_a_dropped_s_tile_is_rejected():
    assert len(_rejected(["qkv-split-M196", "projq-split-M12", "fc1-plain-M700"], drop_s_tile=True)) == 3


def test_wrong_shift_bookkeeping_is_rejected():
    for n in ("qkv-split-M12", "qkv-split-M196-first", "projq-split-M700", "fc1-plain-M196"):
        got = _rejected([n], shift_twice=True)
        assert got and "ln_shift" in got[0][1], (n, got)
    got = _rejected(["qkv-split-M12-first", "qkv-split-M700-first"], ignore_init=True)
    assert len(got) == 2 and all("ln_shift not finite" in g[1] for g in got), got


def test_x16_of_the_unshifted_rows_is_rejected():
    for n in ("proj-split-M12", "fc2-plain-M196", "fc2-split-M700"):
        ops = F.make_producer(F.CASE[n])
        outs = F.alloc_producer(ops)
        F.emulate(F.producer_op(ops, outs), x16_unshifted=True)
        with pytest.raises(AssertionError, match="x16"):
            F.check_producer(ops, outs)


@pytest.mark.parametrize("precision", ["fp16w2", "fp16wa"])
def test_chain_under_the_emulation(precision):
    reps = F.run_chain(F.make_chain(precision), F.emulate)
    print(reps)
    assert len(reps) == 3 * F.CHAIN_L
    for r in reps:
        assert r["kappa"] <= 2.0 and r["err"] <= 0.5 and r["shift"] <= 0.5, r
