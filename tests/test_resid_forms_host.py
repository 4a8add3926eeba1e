"""CPU: the table of tests/test_resid_forms_gpu.py is complete and its checks discriminate (tests/resid_forms.py).  Every kernel name the restated dispatch returns for
the six sites and three weight modes over M = 4, 8 .. 40000 has its ragged and its whole-tile case: the share left out is zero.  An fp32 emulation of what the kernels
write stays within HALF of every allowance on the boundary rows of the small cases: of gemm_forms.bound for the twin, of the same bound for RESID against fp64 once
the rounding of the sum (2^-24 |out|, which a correctly rounded result reaches in full) is taken off, of 2u / 2u (8u) for GELU against fp64.  GELU against the twin
has no such room by construction: u |g| + h is one correct rounding and 1.3e-6 is gelu_erf's own documented error, of which the fit uses 1.17e-6 (at x = 3.63); the
emulation is held to the whole bound there and the share of the 1.3e-6 it uses is printed.  Each planted defect fails the check named for it: the old residual kept in its top
24 bits, the old row added twice in the ragged block and (x0 + acc) + bias fail the exact relation; a row written past M fails the canary; the tanh GELU fails the GELU
bound in fp16; max(x, 0) dropped from the GELU fails the sign rule."""
import pytest
import torch

import gemm_forms as F
import resid_forms as R


def test_table_reaches_every_kernel_name_of_the_sweep():
    reached, missing, total = set(), [], 0
    for site in R.SITES:
        for w in R.WEIGHTS:
            for kern in R.sweep_names(site, w):
                total += 1
                have = {c["rows"]: c for c in R.CASES if (c["site"], c["weights"], c["kernel"]) == (site[0], w, kern)}
                if set(have) != {"ragged", "whole"}:
                    missing.append((site[0], w, kern))
                    continue
                reached.add(kern)
                rag, whole = have["ragged"], have["whole"]
                assert 0 < rag["M"] % rag["tile"] <= 4 and whole["M"] % whole["tile"] == 0 and whole["M"] > rag["M"] and whole["K"] == site[3]
                for c in (rag, whole):
                    assert F.kernel_of(c, w) == kern
    print(sorted(reached))
    print("names over the sweep:", total, "left out:", len(missing))
    assert not missing, missing
    fams = {k.split("/")[0] for k in reached}
    assert {k.split("/")[0] for k in reached if "/e3/" in k} == {"g64p", "g48k128", "g64", "g96", "g128", "g256p", "g256ps", "g256s", "g256"}
    assert {k.split("/")[0] for k in reached if "/e1/" in k} == fams and fams - {k.split("/")[0] for k in reached if "/e3/" in k} == {"g256o2"}
    assert {"g256p/e3/w1/n256", "g256p/e3/w2/n128", "g256/e3/w2/n192", "g256/e3/w2/n256", "g256ps/e1/w3/n128", "g256s/e1/w3/n256"} <= reached
    assert R.CASE["dec_proj-sparse-g256s_e3_w3_n256-ragged-M17412-K128"]["M"] == 68 * 256 + 4
    for fam in fams:     # the pipelines' edges: one and two K-tiles, and a site's own K
        for e in ("/e1/", "/e3/"):
            ks = {c["K"] for c in R.CASES if c["kernel"].startswith(fam + e)}
            assert not ks or {R._small_k(fam, False), R._small_k(fam, True)} <= ks and ks & {768, 1024, 3072, 4096}, (fam, e, ks)
    # the domain runs: the per-row and the whole-fragment store paths on 64-column wave tiles, and chip-filling GELU families
    n = R.domain()[0].numel()
    kern = {(t, dt, w): R.domain_kernel(w, M, n) for t, dt, w, M in R.DOMAIN_RUNS}
    assert kern[("row", "fp16", "plain")] == kern[("frag", "fp16", "plain")] == "g128/e1/w1/n128"
    assert {k.split("/")[0] for (t, _, _), k in kern.items() if t == "chip"} == {"g256p", "g256o2"}
    assert {M for t, _, _, M in R.DOMAIN_RUNS if t == "row"} == {4} and {M for t, _, _, M in R.DOMAIN_RUNS if t == "frag"} == {64}


SMALL = [c["name"] for c in R.CASES if c["rows"] == "ragged" or c["M"] <= 1024]     # small K, or few rows at the site's K


def _host(name, dt):
    case = R.CASE[name]
    ops = R.make_operands(case, dt, "cpu")
    rows = R.edge_rows(case)
    return case, ops, rows, F.reference(ops, 0, rows)


def _dts(case):
    return ("bf16", "fp16") if case["weights"] == "plain" else ("fp16",)


@pytest.mark.parametrize("name", SMALL)
def test_clean_emulation_stays_within_half_of_every_bound(name):
    worst = {}
    for dt in _dts(R.CASE[name]):
        case, ops, rows, p64 = _host(name, dt)
        rt, at = R.f32_bound(case, dt, R.twin_ops(ops)["kernel"])
        if case["epi"] == R.RESID:
            x0 = R.make_x0(len(rows), case["N"], "cpu")
            out, v32 = R.emulate_resid(ops, x0, rows)
            R.check_resid_exact(out, x0, v32)
            assert R.resid_ratio64(out, x0, p64, rt, at) <= 1.0
            e = {"twin": F.ratio(v32, p64, rt, at), "resid64": R.resid_ratio64(out, x0, p64, rt, at, room=True)}
        else:
            out, v32 = R.emulate_gelu(ops, rows)
            rg, ag = R.gelu_bound64(case, dt, ops["kernel"])
            assert R.gelu_ratio(out, v32, dt) <= 1.0
            e = {"twin": F.ratio(v32, p64, rt, at), "gelu64": F.ratio(out, R.sat(R.gelu64(p64), dt), rg, ag)}
            worst[dt + " share of 1.3e-6"] = round(R.gelu_ratio(out, v32, dt, room=True), 3)
        worst[dt] = {k: round(v, 3) for k, v in e.items()}
        assert max(e.values()) <= 0.5, (name, dt, e)
    print(name, worst)


def test_clean_domain_emulation_passes_and_defects_fail():
    x, nf = R.domain()
    for dt in ("bf16", "fp16"):
        out = R.round16(R.gelu_kernel(x), dt)
        r = R.check_domain(out, x, nf, dt)
        print("domain", dt, "emulated ratio", round(r, 3), "share of 1.3e-6", round(R.gelu_ratio(out[:nf], x[:nf], dt, room=True), 3))
        with pytest.raises(AssertionError, match="sign rule"):       # max(x, 0) dropped
            R.check_sign(R.round16(R.gelu_kernel(x[:nf], no_max=True), dt), x[:nf])
        with pytest.raises(AssertionError, match="GELU bound"):       # the tanh form
            R.check_domain(R.round16(R.gelu_kernel(x, tanh=True), dt), x, nf, dt)
        R.check_store_domain(R.round16(0 + x, dt), x, nf, dt)
        lost = R.round16(0 + x, dt)
        lost[nf] = -65504.0                                            # the clamp that swallowed a NaN
        with pytest.raises(AssertionError, match="NaN"):
            R.check_store_domain(lost, x, nf, dt)
        keep = out.clone()                                             # a tail that never reaches max(x, 0): the identity rule
        sel = (x >= 1) & (R.erfc_term64(x) < R.HALF_STEP[dt]) & (x < 60000)
        keep[sel] = R.round16(x[sel] * (1 - 2 * F.DT[dt][2]), dt)
        with pytest.raises(AssertionError):
            R.check_domain(keep, x, nf, dt)


RESID_SMALL = ["enc_proj-plain-g64p_e3_w1_n64-ragged-M4-K64", "dec_fc2-split-g48k128_e3_w2_n48-ragged-M532-K384", "dec_fc2-sparse-g96_e3_w2_n96-ragged-M2596-K64",
               "enc_fc2-split-g64_e3_w2_n64-ragged-M1028-K128", "dec_proj-sparse-g256s_e3_w3_n256-ragged-M17412-K128", "enc_proj-plain-g64p_e3_w1_n64-whole-M64-K1024"]
GELU_SMALL = ["enc_fc1-plain-g64p_e1_w1_n64-whole-M64-K1024", "dec_fc1-split-g96_e1_w2_n96-ragged-M580-K64", "dec_fc1-sparse-g256s_e1_w3_n256-ragged-M4356-K128"]


@pytest.mark.parametrize("name", RESID_SMALL)
def test_planted_residual_defects_fail_the_exact_relation(name):
    for dt in _dts(R.CASE[name]):
        case, ops, rows, _ = _host(name, dt)
        x0 = R.make_x0(len(rows), case["N"], "cpu")
        defects = [dict(trunc24=True), dict(bias_last=True)] + ([dict(double_ragged=True)] if case["rows"] == "ragged" else [])
        for d in defects:
            out, v32 = R.emulate_resid(ops, x0, rows, **d)
            with pytest.raises(AssertionError, match="exact relation"):
                R.check_resid_exact(out, x0, v32)
        # the round-1 bound (rtol 1e-5, atol 1e-4) lets the 24-bit residual through on the rows of order 1: what this file is for
        out, v32 = R.emulate_resid(ops, x0, rows, trunc24=True)
        small = x0.abs() <= 2
        assert bool((((out - (x0 + v32)).abs() <= 1e-4 + 1e-5 * (x0 + v32).abs()) | ~small).all())


def test_row_written_past_M_fails_the_canary():
    for fill, dtype in ((R.CANARY_X, torch.float32), (F.CANARY16, torch.int16), (float("nan"), torch.float32)):
        buf, view = R.frame(torch.ones((5, 64), dtype=dtype), fill)
        R.check_frame(buf, fill, 5, "clean")
        for row in (F.LEAD - 1, F.LEAD + 5):
            b = buf.clone()
            b[row] = b[row] + view[4] if fill == R.CANARY_X else view[4]      # the read-modify-write of the residual epilogue, or a store
            with pytest.raises(AssertionError, match="canary"):
                R.check_frame(b, fill, 5, "past M")


@pytest.mark.parametrize("name", GELU_SMALL)
def test_tanh_gelu_fails_the_gelu_bound_in_fp16(name):
    case, ops, rows, p64 = _host(name, "fp16")
    out, v32 = R.emulate_gelu(ops, rows)
    assert R.gelu_ratio(out, v32, "fp16") <= 1.0
    out, v32 = R.emulate_gelu(ops, rows, tanh=True)
    assert R.gelu_ratio(out, v32, "fp16") > 1.0
    out, v32 = R.emulate_gelu(ops, rows, no_max=True)
    with pytest.raises(AssertionError, match="sign rule"):
        R.check_sign(out, v32)


def test_position_halfwords_round_trip():
    g = torch.Generator().manual_seed(3)
    lo = (torch.randn((64, 128), generator=g) * 2.0 ** -12).half()
    lo[:, ::7] = 0
    lo[:5, :8] = 0
    pos, two = R.pruned_positions(lo)
    assert bool(two.any()) and not bool(two.all())
    idx = R.encode_idx(pos)
    assert idx.shape == (2, 2, 64)
    assert torch.equal(R.decode_idx(idx, 64, 128), pos)
    R.check_positions(idx, lo)
    bad = idx ^ 1                 # the first kept position of group q = 0, in half of the rows
    with pytest.raises(AssertionError, match="position"):
        R.check_positions(bad, lo)
