"""GPU (-m gpu): the fp32 residual epilogue and the exact-erf GELU epilogue in every kernel the default dispatch reaches from the proj / fc1 / fc2 Linears of the encoder
and decoder blocks, through must3r_hip_op_gemm_ex, against fp64 (tests/resid_forms.py: case table, relations, bounds, checks).  Per case and dtype, under the default
options: the kernel the restated dispatch names ran; its EPI_F32 twin against fp64; RESID: out == fl32(x0 + v32) bit for bit and against fp64; GELU: against gelu64 of the
twin and against fp64; canaries in front of and behind every destination; A, W, the packed low part and the bias untouched; a second launch the same bits; the sparse
pack's position halfwords against the 2:4 rule.  Then gelu_erf over its whole domain through launches with A = 0.  The measured ratios go through test_ops_gpu.record
and, as a table, to the file M3R_RESID_FORMS_TABLE names (kept as profiles/resid_forms_errors.txt)."""
import os
import time

import pytest
import torch

import gemm_forms as F
import resid_forms as R
from test_gemm_forms_gpu import DEFAULTS, launch, pack_sparse   # the descriptor filling of must3r_hip_op_gemm_ex and its `picked` field
from test_ops_gpu import record

pytestmark = pytest.mark.gpu
_rows = []     # (site, weights, dt, kernel, twin kernel, twin ratio, resid ratio, gelu / twin ratio, gelu / fp64 ratio, exact, resid room)
_domain = []   # (tag, dt, weights, M, kernel, ratio, share of 1.3e-6, gelu(+inf), gelu(-inf))


@pytest.fixture(scope="module")
def lib():
    from must3r_amd import _lib
    t0 = time.time()
    for n, v in DEFAULTS:
        _lib.set_option(n, v)
    yield _lib
    for n, v in DEFAULTS:
        _lib.set_option(n, v)
    table = os.environ.get("M3R_RESID_FORMS_TABLE")
    if _rows and table:
        with open(table, "w") as f:
            f.write("# tests/test_resid_forms_gpu.py: worst ratios per site, weights, dtype and picked kernel (gemm_last_kernel()) over the kernel's two cases (ragged last row block,\n"
                    "# whole tiles at the site's K).  twin = max |v32 - fp64| / (atol + rtol |fp64|) of the EPI_F32 launch of the same operands (kernel: `twin kernel`; bound:\n"
                    "# 1e-5 / 1e-4 plain, 2e-6 / 8e-6 split or sparse).  resid64 = max |out - (x0 + p64)| / (bound(p64) + 2^-24 |out|).  exact = out == fl32(x0 + v32) bit for bit;\n"
                    "# room = max (|out - (x0 + p64)| - 2^-24 |out|) / bound(p64): what is used of the product's allowance beside the one rounding of the sum.\n"
                    "# gelu/twin = max |out - gelu64(v32)| / (u |g| + 1.3e-6 + h).  gelu64 = max |out - gelu64(p64)| / (2u + 2u |.|), 8u absolute with a sparse low part.\n"
                    "# A ratio <= 1 passes; `-` = not that epilogue.  Below: gelu_erf over its domain (A = 0, bias = x), ratio of u |g| + 1.3e-6 + h, the share of the 1.3e-6 that is\n"
                    "# used once the rounding u |g| + h is taken off, and what +-inf gives.\n"
                    f"# wall time of the file: {time.time() - t0:.0f} s\n")
            f.write(f"{'site':<10}{'weights':<8}{'dt':<5}{'kernel':<20}{'twin kernel':<20}{'cases':>6}{'twin':>8}{'resid64':>9}{'room':>7}{'exact':>7}{'gelu/twin':>11}{'gelu64':>8}\n")
            agg = {}
            for (site, w, dt, kern, tk, tw, rr, gt, g64, exact, room) in _rows:
                a = agg.setdefault((site, w, dt, kern), [0, set(), 0.0, None, None, None, True, None])
                a[0] += 1
                a[1].add(tk)
                a[2] = max(a[2], tw)
                for i, v in ((3, rr), (4, gt), (5, g64), (7, room)):
                    if v is not None:
                        a[i] = v if a[i] is None else max(a[i], v)
                a[6] = a[6] and exact is not False

            def fmt(v, w):
                return f"{'-':>{w}}" if v is None else f"{v:>{w}.3f}"
            for (site, w, dt, kern), a in agg.items():
                ex = "-" if a[3] is None else ("yes" if a[6] else "NO")
                f.write(f"{site:<10}{w:<8}{dt:<5}{kern:<20}{'|'.join(sorted(a[1])):<20}{a[0]:>6}{a[2]:>8.3f}{fmt(a[3], 9)}{fmt(a[7], 7)}{ex:>7}{fmt(a[4], 11)}{fmt(a[5], 8)}\n")
            f.write(f"\n{'domain':<8}{'dt':<5}{'weights':<8}{'M':>6}  {'kernel':<20}{'ratio':>8}{'of 1.3e-6':>11}  {'gelu(+inf)':>11}{'gelu(-inf)':>11}\n")
            for (tag, dt, w, M, kern, r, share, pinf, ninf) in _domain:
                f.write(f"{tag:<8}{dt:<5}{w:<8}{M:>6}  {kern:<20}{r:>8.3f}{share:>11.3f}  {pinf!r:>11}{ninf!r:>11}\n")


def _snapshot(ops):
    keep = [ops["A"], ops["W"], ops["bias"]] + (list(ops["packed"]) if "packed" in ops else [])
    return keep, [t.clone() for t in keep]


def _go(lib, ops, epi, view):
    return launch(lib, dict(ops, case=dict(ops["case"], epi=epi)), dict(base=view))


@pytest.mark.parametrize("name,dt", R.COMBOS, ids=[f"{n}-{dt}" for n, dt in R.COMBOS])
def test_site_kernel_against_fp64(lib, name, dt):
    case = R.CASE[name]
    M, N, epi = case["M"], case["N"], case["epi"]
    ops = R.make_operands(case, dt, "cuda")
    if case["weights"] == "sparse":
        _, idx = pack_sparse(lib, ops)
        torch.cuda.synchronize()
        R.check_positions(idx, ops["lo"][0])
    live, saved = _snapshot(ops)
    # the fp32 twin
    tops = R.twin_ops(ops)
    tbuf, v32 = R.frame_like(case, torch.float32, "cuda", float("nan"))
    twin_kernel = launch(lib, tops, dict(base=v32))
    assert twin_kernel == tops["kernel"], (twin_kernel, tops["kernel"])
    R.check_frame(tbuf, float("nan"), M, "twin")
    R.check_written(v32, None, "twin")
    p64 = F.reference(ops, 0)
    rt, at = R.f32_bound(case, dt, twin_kernel)
    e_twin = F.ratio(v32, p64, rt, at)
    e_res = e_gt = e_g64 = exact = room = None
    if epi == R.RESID:
        x0 = R.make_x0(M, N, "cuda", seed=M)
        buf, out = R.frame(x0, R.CANARY_X)
        picked = _go(lib, ops, epi, out)
        R.check_frame(buf, R.CANARY_X, M, "resid")
        e_res = R.resid_ratio64(out, x0, p64, rt, at)
        room = R.resid_ratio64(out, x0, p64, rt, at, room=True)
        fam = picked.split("/")[0]
        try:
            R.check_resid_exact(out, x0, v32, (name, dt, picked, twin_kernel))
            exact = True
        except AssertionError:
            exact = False
            if fam not in R.LEGIT_ORDER:
                _rows.append((case["site"], case["weights"], dt, picked, twin_kernel, e_twin, e_res, None, None, False, room))
                print(name, dt, picked, "twin", twin_kernel, e_twin, "resid64", e_res)
                raise
        buf2, out2 = R.frame(x0, R.CANARY_X)
        _go(lib, ops, epi, out2)
        assert torch.equal(R.bits(buf), R.bits(buf2)), "a second launch from a fresh copy of x0 gives other bits"
        del buf2, out2, x0
    else:
        buf, win = R.frame_like(case, torch.int16, "cuda", F.CANARY16)
        picked = _go(lib, ops, epi, win)
        R.check_frame(buf, F.CANARY16, M, "gelu")
        R.check_written(win, F.CANARY16, "gelu")
        out = win.contiguous().view(F.DT[dt][1])
        e_gt = R.gelu_ratio(out, v32, dt)
        rg, ag = R.gelu_bound64(case, dt, picked)
        e_g64 = F.ratio(out, R.sat(R.gelu64(p64), dt), rg, ag)
        buf2, win2 = R.frame_like(case, torch.int16, "cuda", F.CANARY16)
        _go(lib, ops, epi, win2)
        assert torch.equal(buf, buf2), "a second launch gives other bits"
        del buf2, win2
    for t, s in zip(live, saved):
        assert torch.equal(R.bits(t), R.bits(s)), "an input changed under the launch"
    _rows.append((case["site"], case["weights"], dt, picked, twin_kernel, e_twin, e_res, e_gt, e_g64, exact, room))
    record("resid_form", case=name, dt=dt, kernel=picked, twin_kernel=twin_kernel, twin=e_twin, resid64=e_res, resid_room=room, exact=exact, gelu_twin=e_gt, gelu64=e_g64)
    print(name, dt, picked, "twin", twin_kernel, e_twin, "resid64", e_res, "exact", exact, "gelu/twin", e_gt, "gelu64", e_g64)
    assert picked == case["kernel"], (picked, case["kernel"])
    assert e_twin <= 1.0, ("twin against fp64", e_twin)
    if epi == R.RESID:
        assert e_res <= 1.0, ("RESID against fp64", e_res)
    else:
        assert e_gt <= 1.0, ("GELU against gelu64 of the twin: u |g| + 1.3e-6 + h", e_gt)
        assert e_g64 <= 1.0, ("GELU against fp64", e_g64)
    del ops, tops, p64, v32, tbuf, buf, out, live, saved
    torch.cuda.empty_cache()


def _domain_launch(lib, tag, dt, weights, M, epi):
    """A = 0, bias = the domain: every row stores T(epi(+0 + bias[n])).  Returns (x, the number of finite inputs, the stored row, the picked kernel)"""
    x, nf = R.domain()
    x = x.cuda()
    N, K = x.numel(), 64
    case = F._case("gelu", f"domain-{tag}", epi, N, K, M)
    g = torch.Generator(device="cuda").manual_seed(5)
    tdt = F.DT[dt][1]
    Wf = torch.randn((1, N, K), device="cuda", generator=g)
    W = Wf.to(tdt) if weights == "plain" else torch.cat((Wf.half(), (Wf - Wf.half().float()).half()), dim=2)
    ops = dict(case=case, dt=dt, weights=weights, A=torch.zeros((M, K), device="cuda", dtype=tdt), W=W.contiguous(), bias=x.clone()[None], bias2=None)
    buf, win = R.frame_like(case, torch.int16, "cuda", F.CANARY16)
    picked = launch(lib, ops, dict(base=win))
    assert picked == R.domain_kernel(weights, M, N, epi), picked
    R.check_frame(buf, F.CANARY16, M, "domain")
    assert bool((win == win[0]).all()), "rows differ although every row has the same inputs"
    return x, nf, win[0].contiguous().view(tdt), picked


@pytest.mark.parametrize("tag,dt,weights,M", R.DOMAIN_RUNS, ids=[f"{t}-{dt}-{w}-M{M}" for t, dt, w, M in R.DOMAIN_RUNS])
def test_gelu_over_its_domain(lib, tag, dt, weights, M):
    """A = 0: the accumulator is exactly +0 and every row stores T(gelu_erf(bias[n]))"""
    x, nf, out, picked = _domain_launch(lib, tag, dt, weights, M, R.GELU)
    pinf, ninf = out[nf + 1].item(), out[nf + 2].item()
    r = R.gelu_ratio(out[:nf], x[:nf], dt)
    share = R.gelu_ratio(out[:nf], x[:nf], dt, room=True)
    _domain.append((tag, dt, weights, M, picked, r, share, pinf, ninf))
    record("gelu_domain", run=tag, dt=dt, weights=weights, M=M, kernel=picked, ratio=r, share_of_gelu_abs=share, gelu_pos_inf=repr(pinf), gelu_neg_inf=repr(ninf))
    print(tag, dt, weights, M, picked, "ratio", r, "gelu(+inf)", pinf, "gelu(-inf)", ninf)
    R.check_domain(out, x, nf, dt)


@pytest.mark.parametrize("tag,dt,weights,M", R.DOMAIN_RUNS, ids=[f"{t}-{dt}-{w}-M{M}" for t, dt, w, M in R.DOMAIN_RUNS])
def test_store16_over_the_same_domain(lib, tag, dt, weights, M):
    """the 16-bit store alone on the same inputs: T(x) bit for bit, fp16 saturated, NaN kept"""
    x, nf, out, picked = _domain_launch(lib, tag, dt, weights, M, F.EPI_STORE16)
    print(tag, dt, weights, M, picked, "store(+inf)", out[nf + 1].item(), "store(-inf)", out[nf + 2].item())
    R.check_store_domain(out, x, nf, dt)
