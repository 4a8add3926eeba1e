"""CPU: the checks of tests/test_cam_gpu.py discriminate.  The same cases, fp64 reference, derived bounds and check functions (tests/cam_cases.py); what
cam_kernel + cam_solve_kernel compute is emulated (fp32 terms, fp64 sums, the kernels' block layout) and must stay within HALF of every bound against
fp64; the same emulation with a plausible defect planted must miss by at least 4x the bound on every case that is there to see it.  What a defect does
on every other case is measured too and printed with the rest (``pytest -s``) and recorded with the test metrics, as ``cam_host_ratios``: a case that a defect
changes and that still passes is named there, not silent.  A defect that slips through is a case to add or a bound to tighten.

Measured (smallest error / bound over the cases that are there to see it):
    9 steps 344, 11 steps 268, 5 steps 2.9e3, 0 steps 1.3e4, previous step's weights 2.9e3 (focal; the contaminated cases)
    principal point ((W-1)/2,(H-1)/2) 349 (and no case passes it), u/v swapped on a square image 2.5e5, wrong width for the strided slots 2.8e3 (focal)
    a block's partial dropped 10.6 (focal) and 1.8e3 (R), added twice 9.1 and 1.5e3; a launch's views shifted by one 3.1e3 (focal), 6e6 (R)
    1e-8 clip missing, non-finite ratios kept: NaN focal (infinite ratio)
    registration weights conf 1.2e3, uniform 3.2e3; x, y exchanged in M 2.6e5; reflection returned 2.2e6 (and det R = -1); eigenvector of A[0][0] 8.2e6
    fp32 instead of fp64 for the cross-block sums: 5.4 on R (128x160: 20 and 10 blocks per view) -- a defect of the registration, whose uncentred
    moments lose in fp32 what the centring needs
BENIGN: the same fp32 cross-block sums as far as the focal goes: N and D take two roundings more where K (cond_N + 1) >= 22 are allowed for; the largest
ratio over all cases is 0.14.
The clean emulation's largest ratios against fp64: focal 0.19, R 0.37, t 0.23."""
import json

import pytest
import torch

import cam_cases as C
from oracle import cam_ref
from test_ops_gpu import record

MARGIN = 4.0
NAMES = [c["name"] for c in C.CASES]
CONTAMINATED = [n for n in NAMES if n.startswith(("contaminated", "degenerate"))]
SCENES = [n for n in NAMES if n.startswith(("clean", "contaminated"))]
FOCAL = ("focal_vs_fp64",)
SEEN = {}


def _multi_block(n):
    d = C.case_data(n)
    return max(g for _, g, _ in C.launch_plan(d.V, d.H, d.W)) > 1


# defect -> (emulate's arguments, the cases that are there to see it, the quantities that must miss)
DEFECTS = {
    "9_steps": (dict(n_iter=9), CONTAMINATED, FOCAL),
    "11_steps": (dict(n_iter=11), CONTAMINATED, FOCAL),
    "5_steps": (dict(n_iter=5), CONTAMINATED, FOCAL),
    "0_steps": (dict(n_iter=0), CONTAMINATED, FOCAL),
    "previous_weights": (dict(prev_weights=True), CONTAMINATED, FOCAL),
    "pp_half_pixel": (dict(pp_half=True), CONTAMINATED, FOCAL),
    "uv_swapped_square": (dict(swap_uv=True), [n for n in CONTAMINATED if n.endswith("x16x16")], FOCAL),
    "wrong_width_strided": (dict(wrong_width=True), ["contaminated_24x128x160", "clean_24x128x160"], FOCAL),
    "block_dropped": (dict(drop_block=1), [n for n in SCENES if _multi_block(n)], FOCAL + ("R_vs_fp64",)),
    "block_twice": (dict(dup_block=1), [n for n in SCENES if _multi_block(n)], FOCAL + ("R_vs_fp64",)),
    "launch_shifted": (dict(shift_launch=True), ["clean_300x16x16", "contaminated_300x16x16"], FOCAL + ("R_vs_fp64",)),
    "no_1e-8_clip": (dict(no_clip=True), ["degenerate_3x64x96"], FOCAL),
    "nonfinite_kept": (dict(keep_nonfinite=True), ["degenerate_3x64x96"], FOCAL),
    "weights_conf": (dict(reg_weights="conf"), SCENES, ("R_vs_fp64",)),
    "weights_uniform": (dict(reg_weights="uniform"), SCENES, ("R_vs_fp64",)),
    "xy_exchanged_in_M": (dict(swap_xy=True), SCENES + ["mirror_3x64x96", "offset100_3x64x96"], ("R_vs_fp64",)),
    "reflection": (dict(reflection=True), ["mirror_3x64x96"], ("R_vs_fp64",)),
    "eigenvector_of_A00": (dict(first_eig=True), ["rot180x_3x64x96", "rot180y_3x64x96", "rot180z_3x64x96"], ("R_vs_fp64",)),
    # fp32 for the sums across blocks: a defect of the registration (the uncentred moments lose what the centring needs); for the focal see
    # test_fp32_cross_block_sums_are_benign_for_the_focal
    "fp32_cross_block_sums": (dict(fp32_cross=True), [n for n in SCENES if n.endswith("x128x160")], ("R_vs_fp64",)),
}


def _emulate(name, **defect):
    d = C.case_data(name)
    return d, C.emulate(d.p3, d.pl, d.cf, d.H, d.W, **defect)


def _report(name, **defect):
    d, (f, c) = _emulate(name, **defect)
    return C.report(d, f, c, d.p3, d.pl, d.cf)


def _passes(name, **defect):
    d, (f, c) = _emulate(name, **defect)
    try:
        C.check(d, f, c, d.p3, d.pl, d.cf)
    except AssertionError:
        return False
    return True


@pytest.fixture(scope="module", autouse=True)
def _dump():
    yield
    print("\ncam host ratios (defect: smallest error/bound over its cases):", json.dumps(SEEN, indent=1))
    record("cam_host_ratios", **SEEN)


@pytest.mark.parametrize("name", NAMES)
def test_clean_emulation_is_within_half_of_every_bound(name):
    """The kernels' arithmetic, emulated, passes every check, with at most half of each bound against fp64.  (Against the fp32 restatement the bound holds
    that restatement's own error, which a perfect implementation shows in full: there it has to pass, not to halve.)"""
    d, (f, c) = _emulate(name)
    rep = C.check(d, f, c, d.p3, d.pl, d.cf)
    SEEN.setdefault("clean_emulation", {})[name] = {k: round(r["ratio"], 3) for k, r in rep.items()}
    for k, r in rep.items():
        assert r["ratio"] <= (0.5 if k.endswith("fp64") else 1.0), (name, k, r)
    ref = C.case_reference(d, max(p for _, _, p in C.launch_plan(d.V, d.H, d.W)))
    # the roundings K leaves out (the weights', amplified by the cancellation in dx, dy) as a root-sum-square x 4: well inside the bound
    assert float((ref.amp_rss / ref.bf).max()) < 0.5, (ref.amp_rss / ref.bf).max()
    assert torch.equal(ref.steps[10], ref.focal64)          # the step-by-step restatement the bounds read rho from IS the truth's iteration
    assert bool((ref.gap > 0.02).all()) and bool((ref.cond >= 2.0).all())


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_misses_by_4x(defect):
    kw, cases, keys = DEFECTS[defect]
    assert cases, defect
    seen = SEEN.setdefault(defect, {})
    for name in cases:
        rep = _report(name, **kw)
        for k in keys:
            seen[k] = min(seen.get(k, float("inf")), rep[k]["ratio"])
            assert rep[k]["ratio"] >= MARGIN, (defect, name, k, rep[k])
        assert not _passes(name, **kw)
    for k in keys:
        seen[k] = float(f"{seen[k]:.3g}")
    # every other case: what the defect does there is on record
    unseen, unchanged = [], []
    for name in NAMES:
        if name in cases or C.case_data(name).V > 100:
            continue
        (f0, c0), (f1, c1) = _emulate(name)[1], _emulate(name, **kw)[1]
        if torch.equal(f0, f1) and torch.equal(c0, c1):
            unchanged.append(name)
        elif _passes(name, **kw):
            unseen.append(name)
    seen["changes_but_passes_on"] = unseen
    seen["changes_nothing_on"] = unchanged


def test_structure_defects_are_rejected_outright():
    """the reflection fails det R = 1, not only the value; a wrong last row, a wrong dtype and a wrong activation output are rejected"""
    d, (f, c) = _emulate("mirror_3x64x96", reflection=True)
    with pytest.raises(AssertionError, match="det R"):
        C.check_structure(d, f, c)
    d, (f, c) = _emulate("clean_2x37x53")
    bad = c.clone()
    bad[1, 3, 3] = 0.0
    with pytest.raises(AssertionError, match="last row"):
        C.check_structure(d, f, bad)
    with pytest.raises(AssertionError):
        C.check_structure(d, f.double(), c)
    for k in ("p3", "pl", "cf"):
        arrs = dict(p3=d.p3, pl=d.pl, cf=d.cf)
        arrs[k] = arrs[k].clone()
        arrs[k].view(-1)[-1] *= 1.0 + 1e-5
        with pytest.raises(AssertionError, match="activation output"):
            C.check_activation(d, **arrs)
    nan = f.clone()
    nan[0] = float("nan")
    with pytest.raises(AssertionError):
        C.assert_values(C.report(d, nan, c, d.p3, d.pl, d.cf))


def test_fp32_cross_block_sums_are_benign_for_the_focal():
    """fp32 for N and D across blocks costs the focal two roundings more where K * (cond_N + 1) >= 22 are allowed for: the ratio is reported and stays
    under 4x on every case, so no case is forced for it.  (The registration does see it: DEFECTS above.)"""
    worst = max(_report(name, fp32_cross=True)["focal_vs_fp64"]["ratio"] for name in NAMES)
    SEEN["BENIGN_fp32_cross_block_sums_focal"] = float(f"{worst:.3g}")
    assert worst < MARGIN      # would it ever exceed 4x, it belongs with the defects above


def test_contamination_makes_the_iteration_visible():
    """fp64 reference alone: 9 and 11 steps differ from 10 by >= 1e-3 in every view of the contaminated few-view cases (1e-4 over the 300 tiny views),
    the clean inputs by <= 2e-5 -- the figures of cam_cases' docstring."""
    table = {}
    for name in NAMES:
        d = C.case_data(name)
        ref = C.case_reference(d, max(p for _, _, p in C.launch_plan(d.V, d.H, d.W)))
        st = ref.steps
        sep = {k: float(((st[k] - st[10]) / st[10]).abs().min()) for k in (0, 5, 9, 11)}
        table[name] = dict({f"{k}_steps": float(f"{v:.2g}") for k, v in sep.items()}, rho_median=round(float(ref.rho.nan_to_num(0.0).median()), 2),
                           fp32_vs_fp64=float(f"{float(ref.focal_ref32_err.max()):.2g}"), bound=float(f"{float(ref.bf.max()):.2g}"))
        if name.startswith(("contaminated", "degenerate")):
            floor = 1e-4 if d.V > 100 else 1e-3
            assert sep[9] >= floor and sep[11] >= floor / 2, (name, sep)
        elif name.startswith("clean"):
            assert float(((st[9] - st[10]) / st[10]).abs().max()) <= 2e-5, name
    SEEN["reference_step_separation"] = table


def test_edges_are_well_defined():
    """at every registration edge the fp64 and the fp32 restatements agree: the reference itself is well defined there"""
    table = {}
    for e in C.EDGES:
        d = C.case_data(f"{e}_{C._name(C.EDGE_SHAPE)}")
        ref = C.case_reference(d, 1)
        table[e] = dict(R=float(f"{float(ref.R_ref32_err.max()):.2g}"), t=float(f"{float(ref.t_ref32_err.max()):.2g}"))
        assert float(ref.R_ref32_err.max()) < 1e-5 and float(ref.t_ref32_err.max()) < 1e-5, (e, table[e])
        R = ref.c2w64[:, :3, :3]
        assert torch.allclose(torch.det(R), torch.ones(d.V, dtype=torch.float64), atol=1e-12)
        x, y, w = d.pl.double().reshape(d.V, -1, 3), d.p3.double().reshape(d.V, -1, 3), d.cf.double().reshape(d.V, -1) - 1
        w = w / w.sum(1, keepdim=True)
        xh, yh = x - (w[..., None] * x).sum(1, keepdim=True), y - (w[..., None] * y).sum(1, keepdim=True)
        M = torch.einsum("vp,vpi,vpj->vij", w, yh, xh)
        if e == "mirror":        # the SVD form's det(U V^T) = -1 branch
            assert bool((torch.det(M) < 0).all())
        if e.startswith("rot180"):      # qw = 0: trace R = -1
            assert torch.allclose(R.diagonal(dim1=1, dim2=2).sum(1), -torch.ones(d.V, dtype=torch.float64), atol=1e-2)
        if e == "exact":
            assert torch.equal(d.p3, d.pl) and torch.allclose(R, torch.eye(3, dtype=torch.float64).expand(d.V, 3, 3), atol=1e-12)
        if e == "offset100":
            assert float(ref.c2w64[:, :3, 3].norm(dim=1).min()) > 50.0      # 100 extents of about 0.65
        assert torch.equal(cam_ref.special_procrustes(M), R)
    SEEN["edges_fp32_vs_fp64"] = table


def test_case_table_reaches_every_launch_form():
    """launch_plan on a 256-CU part gives what the module states: G = 1; a ragged second block; G > 1 with ppt = 1; ppt > 1; two launches."""
    for shape, plan in C.PLAN_256.items():
        assert C.launch_plan(*shape) == plan, shape
    assert C.PLAN_256[(5, 16, 16)][0][1:] == (1, 1)
    assert (37 * 53) % C.CAM_T and C.CAM_T % 53 and C.PLAN_256[(2, 37, 53)][0][1] == 2
    assert C.PLAN_256[(2, 128, 160)][0][1] > 1 and C.PLAN_256[(2, 128, 160)][0][2] == 1
    assert C.PLAN_256[(24, 128, 160)][0][1] > 1 and C.PLAN_256[(24, 128, 160)][0][2] > 1
    assert len(C.PLAN_256[(300, 16, 16)]) == 2
    assert {c["shape"] for c in C.CASES} == set(C.PLAN_256)
    kinds = {c["kind"] for c in C.CASES}
    assert kinds == {"clean", "contaminated", "degenerate", *C.EDGES}
