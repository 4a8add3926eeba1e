"""Cases, fp64 reference, derived bounds, check functions and an emulation for ``postprocess(compute_cam=True)`` (must3r_amd/csrc/cam.hip).
Shared by tests/test_cam_gpu.py (the kernels) and tests/test_cam_host.py (the checks discriminate); needs no GPU.

TRUTH is ``oracle.cam_ref.compute_cam(..., dtype=torch.float64)``; the fp32 restatement is the second yardstick.  Both are evaluated on the ACTIVATED
maps the checked implementation itself returns (p3, pl, cf): the kernels register and iterate on exactly the fp32 values they store, and the activation is
checked on its own against ``oracle.must3r_ref.postprocess`` -- so the bounds below are bounds on the camera arithmetic alone, not on ``expm1f``.

CASES.  ``make_cam_pointmaps(noise=0.02)`` is an almost perfect pinhole scene: its closed-form L2 focal already is the Weiszfeld fixed point to four
digits, and the iteration is invisible.  ``contaminate`` multiplies x and y of ``pts3d_local`` by ``1 + tail * |N(0,1)|`` on a seeded random fraction of
the pixels (through the raw channels, so the activation still produces the points).  Re-measured on this file's cases, fp64 reference formulas, relative
change of the focal against 10 steps, minimum over views (tests/test_cam_host.py::test_contamination_makes_the_iteration_visible asserts the floor):

                                   0 steps   5 steps   9 steps   11 steps   rho (median)   fp32 restatement vs fp64 (max over views)
    contaminated 5x16x16           2.4e-1    3.9e-2    2.9e-3    1.9e-3     0.74           3.8e-7
    contaminated 2x37x53           2.6e-1    4.8e-2    3.3e-3    2.1e-3     0.64           1.1e-8
    contaminated 2x128x160         2.5e-1    5.4e-2    4.8e-3    3.2e-3     0.66           1.4e-7
    contaminated 24x128x160        2.5e-1    5.3e-2    4.4e-3    2.9e-3     0.68           3.3e-7
    contaminated 300x16x16         1.7e-1    4.9e-3    1.6e-4    7.7e-5     0.69           1.1e-6      (the minimum is over 300 views)
    2x37x53, frac 0.45, tail 3.0   7.9e-2    1.7e-2    2.0e-3    1.6e-3     0.78           1.2e-7
    degenerate 3x64x96             2.5e-1    5.0e-2    4.3e-3    2.9e-3     0.68           4.7e-8
    clean (noise 0.02), 5 shapes   <= 1.8e-4 <= 6.2e-6 <= 2.1e-7 <= 1.1e-7  0.50 .. 0.54   <= 2.5e-7
against focal bounds of 2.7e-6 .. 1.4e-5: the contaminated cases see one step more or less by 268x the bound and more (test_cam_host.py), the clean
ones do not see it at all.

SHAPES are the smallest that reach each launch form.  ``launch_plan`` restates the host code of cam.hip; on a 256-CU part with one resident block per CU
(138.6 KB of LDS per block), slots = 256 and:

    (5,16,16)      G = 1, ppt = 1, one launch          one block per view
    (2,37,53)      G = 2, ppt = 1, one launch          P = 1961: no multiple of the block (1024) nor of W; the second block is ragged
    (2,128,160)    G = 20, ppt = 1, one launch         several blocks per view
    (24,128,160)   G = 10, ppt = 2, one launch         several blocks per view, strided slots (the (col,row) walk of the iteration loop)
    (300,16,16)    G = 1, ppt = 1, launches of 256+44  more views than one cooperative launch holds
    (3,64,96)      G = 6, ppt = 1                      the degenerate-pixel case and the registration edges

slots = CUs x occupancy, so these depend on the device: the GPU test reads the CU count and skips only this claim, never the check, when it differs.

FOCAL BOUND.  The kernel forms every per-pixel term in fp32 and every sum across threads and blocks in fp64 (<= P * 2^-53: nothing).  One IRLS step is
f' = N(f) / D(f) with N = sum w (qx u + qy v), D = sum w (qx^2 + qy^2), w = 1 / max(|pix - f q|, 1e-8).  A relative rounding of size e = 2^-24 on the path
of one elementary product moves N by at most e * sum|w qx u| + |w qy v|, so by the condition number cond_N = (sum |w qx u| + |w qy v|) / |N| relative to
N; D has only non-negative terms, cond_D = 1.  An error of f re-enters the next step through the weights; the map contracts with ratio rho, read off the
fp64 reference's own successive steps, rho = |f11 - f10| / |f10 - f9| (per view), so the one-step errors e, e rho, e rho^2 ... add up to e / (1 - rho):

    B_f = K * 2^-24 * (cond_N + cond_D) / (1 - rho)                                   (worst-case sum: every rounding at its bound, same sign)

Among hundreds of tiny contaminated views some have not contracted after ten steps (rho near or above 1) and some clean ones have converged to fp64's own
noise (rho = 0/0); the start and ten steps cannot add up more than 11 one-step errors while rho <= 1, so 1 / (1 - rho) is capped at 11.

K = 10 + ppt is the number of fp32 roundings on the path of one term, counted from cam_kernel:
    q = x / z                      1   (correctly rounded division)
    q.x * u, q.y * vv, their sum   2   (the two products are parallel: one level, then the add; an fma only removes one)
    focal * q.x                    1
    u - focal * q.x                1
    dx * dx, dy * dy, their sum    2
    v_rsq_f32 (1 ulp)              2   (two half-ulp roundings' worth)
    w * (...)                      1
    sa += ... (per-thread fp32)    ppt - 1
    focal = (float)(N / D)         1   (the division itself is fp64)
                                   = 10 + ppt
What K does not count is the cancellation in dx = u - focal * q.x: a pixel whose residual |d| is small against |u| has the roundings of its weight
amplified by |u| / |d|.  Those roundings are independent from pixel to pixel and enter the sums with random signs, so their sum grows like the root of
the pixel count while N and D grow like the count.  Moreover N and D share the weight: f' moves by (dN - f dD) / D = sum (dw / w) w (q . d) / D, and
q . d is small where d is.  ``amp_rss`` evaluates that root-sum-square (times RSS_MULT) per case; test_cam_host.py requires it to stay under half of B_f
(measured: <= 0.33 B_f, at 300x16x16; <= 0.06 elsewhere), and the emulation below -- which has these roundings -- to stay under half of B_f (measured:
<= 0.19 B_f; the kernels on the MI355X: <= 0.14 B_f).

C2W BOUND.  The kernel accumulates uncentred moments S = sum fl(w y_i) x_j (the product of two fp32 numbers is exact in fp64), sums fl(w x), fl(w y) and
w, then M = S / sw - ybar xbar^T.  The only roundings are the fp32 products w * x_j and w * y_i.  A rounding d_p (|d_p| <= e) of fl(w y_i) at pixel p
moves M_ij by d_p w y_i (x_j - xbar_j) / sw -- the centring happens, but after the rounding, so a common offset of y is NOT removed from the error -- and
a rounding of fl(w x_j) moves M_ij by -ybar_i d_p w x_j / sw.  Model: ROOT-SUM-SQUARE of the per-rounding bounds, times RSS_MULT = 4.  Why not the worst
case: it assumes 3 P roundings of equal sign and is sqrt(P) (80 to 440 here) times looser, which would pass registration weights ``conf`` for ``conf - 1``
(4.5e-5 at 1x384x512).  A rounding error is uniform within its bound, sigma = bound / sqrt 3, so the multiple is 6.9 sigma of a sum of thousands of
independent terms (Gaussian to all purposes): 5e-12 per entry.

    dM_ij = 4 e sqrt( sum_p (w y_i (x_j - xbar_j))^2 + ybar_i^2 sum_p (w x_j)^2 ) / sw,      |dR|_F <= 2 |dM|_F / (s2 + d s3)

(the perturbation bound of the polar / special-Procrustes factor; s1 >= s2 >= s3 the singular values of the fp64 reference's M, d = sign det M), then
dt <= dybar + |dR|_F |xbar| + |dxbar| with dybar_i = 4 e sqrt(sum (w y_i)^2) / sw and R dxbar likewise, and the fp32 rounding of the stored result:
e for the entries of R (they are <= 1), e * max|t| for t.  t is taken relative to max(1, max|c2w|), as tests/test_cam_gpu.py always did; R is held to
its own bound, absolutely -- lumping the two under the scale would let a far translation hide a rotation error, which is what the offset case is about.
Horn's 4x4 form in fp64 (Jacobi until the off-diagonals are below 1e-14 of the largest entry) adds nothing at this level.

Against the fp32 restatement the bound is the same plus that restatement's own distance from fp64, measured on the same data (triangle inequality).

REGISTRATION EDGES, each against ``special_procrustes`` in fp64 (shape 3x64x96):
    exact      zero noise, rotation = identity, translation = 0: y == x bit for bit, M is symmetric and the first row of Horn's matrix is zero at entry
    rot180x/y/z  qw = 0: the largest eigenvalue is not A[0][0]
    mirror     world = reflected local + noise: the SVD form takes its det(U V^T) = -1 branch; Horn's form must return the same proper rotation
    offset100  world moved 100 scene extents off the origin.  The moved fp32 points are the case's data.  Its bound is the derived one above, in its
               STATISTICAL (root-sum-square x 4) form; what the offset costs is the factor y_i inside dM.
For each edge test_cam_host.py checks that the fp64 and fp32 restatements agree (to 1e-5; measured 2e-7 .. 1.5e-6), i.e. that the reference is well
defined there.  None had to be dropped.  Offset 100 emulates to a rotation error of 2.2e-7 (the fp32 restatement: 4.3e-7; the bound: 7.2e-6).  At offset
10 000 the kernel arithmetic (2e-6 .. 2.5e-5) no longer matches the fp32 restatement (1e-7 .. 3e-7); that size is documented in cam.hip's header, not
tested.
"""
import functools
import math
from types import SimpleNamespace

import torch

from oracle import cam_ref, must3r_ref as R
from must3r_amd import synthetic as S

EPS32 = 2.0 ** -24
RSS_MULT = 4.0
N_STEPS = 10
CAM_T, CAM_PPT = 1024, 16
REF_CUS = 256
ACT_RTOL, ACT_ATOL = 2e-6, 1e-6          # the activation outputs against oracle.must3r_ref.postprocess (as tests/test_cam_gpu.py always had)

SHAPES = [(5, 16, 16), (2, 37, 53), (2, 128, 160), (24, 128, 160), (300, 16, 16)]
EDGE_SHAPE = (3, 64, 96)
EDGES = ("exact", "rot180x", "rot180y", "rot180z", "mirror", "offset100")
# what launch_plan gives on a 256-CU part: shape -> [(views, G, ppt) per launch]
PLAN_256 = {(5, 16, 16): [(5, 1, 1)], (2, 37, 53): [(2, 2, 1)], (2, 128, 160): [(2, 20, 1)], (24, 128, 160): [(24, 10, 2)],
            (300, 16, 16): [(256, 1, 1), (44, 1, 1)], (3, 64, 96): [(3, 6, 1)]}


def _name(shape):
    return "x".join(map(str, shape))


def _case(shape, kind, **kw):
    c = dict(shape=tuple(shape), kind=kind, frac=0.3, tail=1.0, offset=0.0)
    c.update(kw)
    c["name"] = f"{kind}_{_name(shape)}" + (f"_f{c['frac']}_t{c['tail']}" if kind == "contaminated" and (c["frac"], c["tail"]) != (0.3, 1.0) else "")
    return c


CASES = ([_case(s, "clean") for s in SHAPES] + [_case(s, "contaminated") for s in SHAPES] +
         [_case((2, 37, 53), "contaminated", frac=0.45, tail=3.0), _case(EDGE_SHAPE, "degenerate")] +
         [_case(EDGE_SHAPE, e, offset=100.0 if e == "offset100" else 0.0) for e in EDGES])
BY_NAME = {c["name"]: c for c in CASES}


def launch_plan(V, H, W, ncu=REF_CUS, per_cu=1):
    """must3r_hip_postprocess_cam_act's launches: [(views, G, ppt)]"""
    P = H * W
    slots = ncu * per_cu
    gmin, gmax = -(-P // (CAM_T * CAM_PPT)), -(-P // CAM_T)
    vmax = slots // gmin
    plan = []
    for v0 in range(0, V, vmax):
        nv = min(V - v0, vmax)
        G = min(slots // nv, gmax, max(gmin, 64))
        plan.append((nv, G, -(-P // (G * CAM_T))))
    return plan


# ------------------------------------------------------------------------------------------------ inputs
def _norm_exp(v):
    d = v.norm(dim=-1, keepdim=True)
    return v / d.clip(min=1e-8) * torch.expm1(d)


def _inv_norm_exp(p):
    d = p.norm(dim=-1, keepdim=True)
    return p / d.clip(min=1e-8) * torch.log1p(d)


def contaminate(pm, frac, tail, seed):
    """x and y of pts3d_local times 1 + tail |N(0,1)| on a seeded random fraction of the pixels, through the raw channels"""
    g = torch.Generator().manual_seed(seed)
    local = _norm_exp(pm[..., 3:6].double())
    hit = torch.rand(local.shape[:-1], generator=g) < frac
    fac = 1.0 + tail * torch.randn(local.shape[:-1], generator=g).abs().double()
    local[..., :2] *= torch.where(hit, fac, torch.ones_like(fac)).unsqueeze(-1)
    pm = pm.clone()
    pm[..., 3:6] = _inv_norm_exp(local).float()
    return pm


def set_world(pm, rot, t, noise, seed):
    """world = rot @ (activated local) + t + noise N(0,1), written through the raw channels; rot [V,3,3] or [3,3], t [V,3] or [3]"""
    g = torch.Generator().manual_seed(seed)
    local = _norm_exp(pm[..., 3:6].float()).double()
    V = pm.shape[0]
    rot = torch.as_tensor(rot, dtype=torch.float64).expand(V, 3, 3)
    t = torch.as_tensor(t, dtype=torch.float64).expand(V, 3)
    world = torch.einsum("nij,nhwj->nhwi", rot, local) + t.view(V, 1, 1, 3) + noise * torch.randn(local.shape, generator=g).double()
    pm = pm.clone()
    pm[..., 0:3] = _inv_norm_exp(world).float()
    return pm


def _rot180(axis):
    d = [-1.0, -1.0, -1.0]
    d[axis] = 1.0
    return torch.diag(torch.tensor(d, dtype=torch.float64))


def make_pm(case):
    """raw head outputs [V, H, W, 7] of a case"""
    V, H, W = case["shape"]
    kind, seed = case["kind"], V + H + W
    pm = S.make_cam_pointmaps(V, H, W, focal=0.9 * max(H, W), noise=0.02, seed=seed)
    if kind == "contaminated":
        pm = contaminate(pm, case["frac"], case["tail"], seed + 1)
    elif kind == "degenerate":
        pm = contaminate(pm, 0.3, 1.0, seed + 1)
        pm[0, 3, 4, 3:6] = torch.tensor([0.3, -0.2, 0.0])     # z = 0: +-inf ratios, dropped like nan_to_num does
        pm[1, 10, 20, 3:6] = 0.0                              # 0 / 0 -> nan -> 0
        pm[2, :8, :, 6] = -200.0                              # conf - 1 == 0 exactly
        pm[:, H // 2, W // 2, 3:6] = torch.tensor([0.0, 0.0, 0.5])   # on the principal point's ray: |d| = 0, only the 1e-8 clip keeps w finite
    elif kind == "exact":
        pm[..., 0:3] = pm[..., 3:6]                           # y == x bit for bit
    elif kind.startswith("rot180"):
        pm = set_world(pm, _rot180("xyz".index(kind[-1])), torch.tensor([0.3, -0.2, 0.5]), 0.02, seed + 2)
    elif kind == "mirror":
        q, _ = torch.linalg.qr(torch.randn(V, 3, 3, generator=torch.Generator().manual_seed(seed + 3)).double())
        q = q * (-torch.sign(torch.det(q))).view(V, 1, 1)      # det = -1
        pm = set_world(pm, q, torch.tensor([0.3, -0.2, 0.5]), 0.02, seed + 2)
    elif kind == "offset100":
        act = R.postprocess(pm)
        extent = float(act["pts3d_local"].reshape(-1, 3).std(0).norm())      # one scene extent: the rms radius of the local points
        world = act["pts3d"].double() + case["offset"] * extent * torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64)
        pm[..., 0:3] = _inv_norm_exp(world).float()
    else:
        assert kind == "clean", kind
    return pm


def data_from_pm(name, pm):
    """raw maps [..., H, W, 7] and their CPU activation, the batch dimensions flattened to V views"""
    H, W = pm.shape[-3:-1]
    pm = pm.reshape(-1, H, W, 7)
    act = R.postprocess(pm)
    return SimpleNamespace(name=name, V=pm.shape[0], H=H, W=W, pm=pm, p3=act["pts3d"], pl=act["pts3d_local"], cf=act["conf"])


@functools.lru_cache(maxsize=None)
def case_data(name):
    """the case's raw maps and their CPU activation (made once, shared, never written to)"""
    return data_from_pm(name, make_pm(BY_NAME[name]))


# ------------------------------------------------------------------------------------------------ fp64 reference and bounds
def _ratios64(pl, H, W):
    pix = cam_ref.xy_grid(W, H).double().view(1, -1, 2) - torch.tensor((W / 2, H / 2), dtype=torch.float64).view(1, 1, 2)
    pts = pl.double().reshape(-1, H * W, 3)
    q = (pts[..., :2] / pts[..., 2:3]).nan_to_num(posinf=0, neginf=0)
    return pix, q


def focal_steps64(pl, H, W, n_iter=11):
    """the reference's formulas in fp64: [n_iter + 1, V] focal after 0 .. n_iter steps"""
    pix, q = _ratios64(pl, H, W)
    a, b = (q * pix).sum(-1), q.square().sum(-1)
    f = a.mean(1) / b.mean(1)
    out = [f]
    for _ in range(n_iter):
        w = (pix - f.view(-1, 1, 1) * q).norm(dim=-1).clip(min=1e-8).reciprocal()
        f = (w * a).mean(1) / (w * b).mean(1)
        out.append(f)
    return torch.stack(out)


def reference(p3, pl, cf, H, W, ppt=1):
    """truth (fp64), the fp32 restatement, and the derived bounds, from activated maps [V, H, W, .] / [V, H, W]; every figure per view"""
    V = cf.shape[0]
    p3, pl, cf = p3.reshape(V, H, W, 3), pl.reshape(V, H, W, 3), cf.reshape(V, H, W)
    o64 = cam_ref.compute_cam(p3, pl, cf, dtype=torch.float64)
    o32 = cam_ref.compute_cam(p3, pl, cf)
    r = SimpleNamespace(focal64=o64["focal"], c2w64=o64["c2w"], focal32=o32["focal"], c2w32=o32["c2w"])
    # focal
    steps = focal_steps64(pl, H, W)
    f9, f10, f11 = steps[9], steps[10], steps[11]
    r.steps = steps
    r.rho = (f11 - f10).abs() / (f10 - f9).abs()
    # one-step errors e, e rho, e rho^2, ... add up to e / (1 - rho); the start and ten steps cannot add up to more than 11 e while rho <= 1, which also
    # covers a view that has converged to fp64's own noise (rho = 0/0)
    r.gain = (1.0 / (1.0 - r.rho)).nan_to_num(nan=N_STEPS + 1.0).clip(min=1.0, max=N_STEPS + 1.0)
    pix, q = _ratios64(pl, H, W)
    d = pix - f9.view(-1, 1, 1) * q                          # the weights of the tenth step
    dn = d.norm(dim=-1).clip(min=1e-8)
    w = dn.reciprocal()
    prod = (q * pix).abs().sum(-1)
    r.cond = (w * prod).sum(1) / (w * (q * pix).sum(-1)).sum(1).abs() + 1.0
    K = 10 + ppt
    r.K = K
    r.bf = K * EPS32 * r.cond * r.gain
    # the amplified roundings of the weights (root-sum-square over the pixels): dw / w <= 3 e (|dx| |f qx| + |dy| |f qy|) / |d|^2
    amp = 3.0 * (d.abs() * (f9.view(-1, 1, 1) * q).abs()).sum(-1) / dn.square()
    # ... move f' = N / D by (dN - f dD) / D = sum (dw / w) w q.d / D: the two sums share the weight, and what is left of it is the residual again
    res = w * (q * d).sum(-1)
    r.amp_rss = RSS_MULT * EPS32 * (amp * res).square().sum(1).sqrt() / (f10.abs() * (w * q.square().sum(-1)).sum(1)) * r.gain
    r.focal_ref32_err = ((o32["focal"].double() - o64["focal"]) / o64["focal"]).abs()
    # c2w
    x, y, wt = pl.double().reshape(V, -1, 3), p3.double().reshape(V, -1, 3), cf.double().reshape(V, -1) - 1.0
    sw = wt.sum(1)
    xb, yb = (wt[..., None] * x).sum(1) / sw[:, None], (wt[..., None] * y).sum(1) / sw[:, None]
    M = torch.einsum("vp,vpi,vpj->vij", wt, y - yb[:, None], x - xb[:, None]) / sw[:, None, None]
    sv = torch.linalg.svdvals(M)
    r.gap = sv[:, 1] + torch.sign(torch.det(M)) * sv[:, 2]
    wy, wx = wt[..., None] * y, wt[..., None] * x
    dM2 = (torch.einsum("vpi,vpj->vij", wy.square(), (x - xb[:, None]).square()) +
           yb.square()[:, :, None] * wx.square().sum(1)[:, None, :]) / sw.square()[:, None, None]
    dM = RSS_MULT * EPS32 * dM2.sum((1, 2)).sqrt()
    r.dR = 2.0 * dM / r.gap + EPS32
    dyb = RSS_MULT * EPS32 * wy.square().sum(1).sum(1).sqrt() / sw
    dxb = RSS_MULT * EPS32 * wx.square().sum(1).sum(1).sqrt() / sw
    r.scale = o64["c2w"].abs().amax((1, 2)).clip(min=1.0)
    r.dt = (dyb + r.dR * xb.norm(dim=1) + dxb + EPS32 * o64["c2w"][:, :3, 3].abs().amax(1)) / r.scale
    r.R_ref32_err, r.t_ref32_err = _rt_err(o32["c2w"].double(), o64["c2w"], r.scale)
    return r


def _rt_err(c, ref, scale):
    """largest error of the rotation entries (they are <= 1: absolute) and of the translation (relative to the scene scale), per view"""
    d = (c - ref).abs()
    return d[:, :3, :3].amax((1, 2)), d[:, :3, 3].amax(1) / scale


_REF_CACHE = {}


def case_reference(data, ppt=1):
    """the reference of the case's own (CPU-activated) maps, computed once"""
    key = (data.name, ppt)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = reference(data.p3, data.pl, data.cf, data.H, data.W, ppt)
    return _REF_CACHE[key]


# ------------------------------------------------------------------------------------------------ checks
def _worst(err, bound):
    """largest err / bound over the views; a non-finite error is an infinite ratio"""
    ratio = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    i = int(ratio.argmax())
    return float(err[i]) if math.isfinite(float(ratio[i])) else float("inf"), float(bound[i]), float(ratio[i])


def report(data, focal, c2w, p3, pl, cf, ppt=None):
    """errors, bounds and error / bound of an implementation's outputs (CPU tensors, [V] / [V,4,4] / [V,H,W,.]) against both yardsticks.  The yardsticks
    are evaluated on the implementation's own activated maps; when those are the case's own tensors the shared reference is used."""
    V, H, W = data.V, data.H, data.W
    if ppt is None:
        ppt = max(p for _, _, p in launch_plan(V, H, W))
    own = p3 is data.p3 and pl is data.pl and cf is data.cf
    ref = case_reference(data, ppt) if own else reference(p3, pl, cf, H, W, ppt)
    f, c = focal.reshape(V).double(), c2w.reshape(V, 4, 4).double()
    rep = {}
    ef64 = ((f - ref.focal64) / ref.focal64).abs()
    ef32 = ((f - ref.focal32.double()) / ref.focal32.double()).abs()
    eR64, et64 = _rt_err(c, ref.c2w64, ref.scale)
    eR32, et32 = _rt_err(c, ref.c2w32.double(), ref.scale)
    for k, err, bound in (("focal_vs_fp64", ef64, ref.bf), ("focal_vs_fp32", ef32, ref.bf + ref.focal_ref32_err),
                          ("R_vs_fp64", eR64, ref.dR), ("R_vs_fp32", eR32, ref.dR + ref.R_ref32_err),
                          ("t_vs_fp64", et64, ref.dt), ("t_vs_fp32", et32, ref.dt + ref.t_ref32_err)):
        e, b, q = _worst(err, bound)
        rep[k] = dict(err=e, bound=b, ratio=q)
    return rep


def assert_values(rep, what=""):
    for k, r in rep.items():
        assert r["err"] <= r["bound"], (what, k, r)


def check_structure(data, focal, c2w):
    V = data.V
    assert focal.dtype == torch.float32 and c2w.dtype == torch.float32, (focal.dtype, c2w.dtype)
    assert focal.numel() == V and c2w.numel() == V * 16, (focal.shape, c2w.shape)
    c = c2w.reshape(V, 4, 4)
    det = torch.det(c[:, :3, :3].double())
    assert torch.allclose(det, torch.ones(V, dtype=torch.float64), atol=1e-5), ("det R != 1 (a reflection, or no rotation)", det)
    assert torch.equal(c[:, 3, :], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(V, 4)), "last row of c2w"


def check_activation(data, p3, pl, cf):
    V, H, W = data.V, data.H, data.W
    for k, got, want in (("pts3d", p3, data.p3), ("pts3d_local", pl, data.pl), ("conf", cf, data.cf)):
        assert got.dtype == torch.float32 and got.numel() == want.numel(), (k, got.dtype, got.shape)
        assert torch.allclose(got.reshape(want.shape), want, rtol=ACT_RTOL, atol=ACT_ATOL), "activation output " + k


def check(data, focal, c2w, p3, pl, cf, ppt=None, on_report=None):
    """every check of one case; raises AssertionError; returns the value report (``on_report`` gets it before anything is asserted on it)"""
    check_activation(data, p3, pl, cf)
    assert focal.numel() == data.V and c2w.numel() == data.V * 16, (focal.shape, c2w.shape)
    rep = report(data, focal, c2w, p3, pl, cf, ppt)
    if on_report is not None:
        on_report(rep)
    check_structure(data, focal, c2w)
    assert_values(rep, data.name)
    return rep


# ------------------------------------------------------------------------------------------------ emulation
def _quat_to_rot(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), -1).reshape(*q.shape[:-1], 3, 3)


def _horn(M, first_eig=False):
    """cam_solve_kernel's rotation: the eigenvector of the largest eigenvalue of Horn's 4x4 matrix (s[a][b] = M[b][a])"""
    s = M.transpose(-1, -2)
    sxx, sxy, sxz, syx, syy, syz, szx, szy, szz = s.reshape(-1, 9).unbind(-1)
    A = torch.stack((sxx + syy + szz, syz - szy, szx - sxz, sxy - syx,
                     syz - szy, sxx - syy - szz, sxy + syx, szx + sxz,
                     szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy,
                     sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz), -1).reshape(-1, 4, 4)
    lam, vec = torch.linalg.eigh(A)
    if first_eig:      # the Jacobi column that started as e0, whatever its eigenvalue: the eigenvector closest to (1,0,0,0)
        pick = vec[:, 0, :].abs().argmax(-1)
    else:
        pick = lam.argmax(-1)
    q = vec[torch.arange(vec.shape[0]), :, pick]
    return _quat_to_rot(q / q.norm(dim=-1, keepdim=True))


def emulate(p3, pl, cf, H, W, ncu=REF_CUS, n_iter=10, prev_weights=False, pp_half=False, swap_uv=False, wrong_width=False, drop_block=None,
            dup_block=None, shift_launch=False, no_clip=False, keep_nonfinite=False, reg_weights="conf-1", swap_xy=False, reflection=False,
            first_eig=False, fp32_cross=False):
    """What cam_kernel + cam_solve_kernel compute, term by term: fp32 per-pixel terms (one rounding per operation, no fma), the per-thread fp32 partial
    sums of the iteration, fp64 sums across threads and blocks in the kernels' block layout, uncentred registration sums, M = S / sw - ybar xbar^T, Horn's
    4x4 eigenproblem in fp64.  v_rsq_f32 is taken correctly rounded.  Returns (focal [V] fp32, c2w [V,4,4] fp32).  The keyword arguments plant defects."""
    V = cf.shape[0]
    P = H * W
    x_all, y_all, c_all = pl.reshape(V, P, 3).float(), p3.reshape(V, P, 3).float(), cf.reshape(V, P).float()
    focal_out, c2w_out = torch.empty(V), torch.zeros(V, 4, 4)
    ppx, ppy = ((W - 1) / 2, (H - 1) / 2) if pp_half else (W / 2, H / 2)
    v0 = 0
    for li, (nv, G, ppt) in enumerate(launch_plan(V, H, W, ncu)):
        stride = G * CAM_T
        n = ppt * stride

        def lay(t):      # [nv, P, ...] -> [nv, ppt, G, T, ...]: pixel i = k * stride + g * T + thread, zero beyond P
            pad = torch.zeros((nv, n - P) + t.shape[2:], dtype=t.dtype)
            return torch.cat((t, pad), 1).reshape((nv, ppt, G, CAM_T) + t.shape[2:])

        def across(t, dt=torch.float64):      # [nv, G] per-block sums -> [nv]
            if drop_block is not None and G > 1:
                t = t.clone()
                t[:, drop_block % G] = 0
            if dup_block is not None and G > 1:
                t = t.clone()
                t[:, dup_block % G] *= 2
            if fp32_cross:
                acc = torch.zeros(nv, dtype=torch.float32)
                for g in range(G):
                    acc = acc + t[:, g].float()
                return acc.double()
            return t.sum(1)

        x, y, conf = lay(x_all[v0:v0 + nv]), lay(y_all[v0:v0 + nv]), lay(c_all[v0:v0 + nv])
        idx = torch.arange(n).reshape(1, ppt, G, CAM_T)
        valid = (idx < P).expand(nv, ppt, G, CAM_T)
        w = {"conf-1": conf - 1.0, "conf": conf, "uniform": torch.ones_like(conf)}[reg_weights]
        w = torch.where(valid, w, torch.zeros_like(w))
        a, b = x[..., 0] / x[..., 2], x[..., 1] / x[..., 2]
        if not keep_nonfinite:
            a = torch.where(a.abs() <= 3.402823466e38, a, torch.zeros_like(a))
            b = torch.where(b.abs() <= 3.402823466e38, b, torch.zeros_like(b))
        a, b = torch.where(valid, a, torch.zeros_like(a)), torch.where(valid, b, torch.zeros_like(b))
        u, vv = (idx % W).float() - ppx, (idx // W).float() - ppy
        if swap_uv:
            u, vv = vv, u
        # the data pass: 16 registration sums and the two of the closed-form start
        wx, wy = w[..., None] * x, w[..., None] * y
        terms = torch.cat((w[..., None].double(), wx.double(), wy.double(),
                           (wy.double()[..., :, None] * x.double()[..., None, :]).flatten(-2)), -1)
        Sreg = torch.stack([across(terms[..., j].sum((1, 3))) for j in range(16)], -1)          # [nv, 16]
        t16 = torch.where(valid, a * u + b * vv, torch.zeros_like(a)).double()
        t17 = torch.where(valid, a * a + b * b, torch.zeros_like(a)).double()
        focal = (across(t16.sum((1, 3))) / across(t17.sum((1, 3)))).float()
        # the iteration: (col, row) of slot k walked from slot 0
        ui, vi = u, vv
        if wrong_width:      # slots k >= 1 take their (col, row) with the image's other side as the width
            Wb = H if H != W else W + 1
            uw, vw = (idx % Wb).float() - ppx, (idx // Wb).float() - ppy
            k = torch.arange(ppt).view(1, ppt, 1, 1)
            ui, vi = torch.where(k >= 1, uw, u), torch.where(k >= 1, vw, vv)
            if swap_uv:
                ui, vi = vi, ui
        prev = focal
        for _ in range(n_iter):
            fw = prev if prev_weights else focal
            fb = fw.view(nv, 1, 1, 1)
            dx, dy = ui - fb * a, vi - fb * b
            s2 = dx * dx + dy * dy
            if not no_clip:
                s2 = s2.clip(min=1e-16)
            wi = s2.double().rsqrt().float()
            ta = torch.where(valid, wi * (a * ui + b * vi), torch.zeros_like(a))
            tb = torch.where(valid, wi * (a * a + b * b), torch.zeros_like(a))
            sa, sb = ta[:, 0], tb[:, 0]
            for k in range(1, ppt):      # per-thread fp32 partial sums
                sa, sb = sa + ta[:, k], sb + tb[:, k]
            prev = focal
            focal = (across(sa.double().sum(2)) / across(sb.double().sum(2))).float()
        # the solve
        sw = Sreg[:, 0]
        xb, yb = Sreg[:, 1:4] / sw[:, None], Sreg[:, 4:7] / sw[:, None]
        M = Sreg[:, 7:].reshape(nv, 3, 3) / sw[:, None, None] - yb[:, :, None] * xb[:, None, :]
        if swap_xy:      # sum w x_i y_j for sum w y_i x_j
            M = M.transpose(-1, -2)
        if reflection:      # U V^T without the sign fix
            U, _, Vh = torch.linalg.svd(M)
            Rm = U @ Vh
        else:
            Rm = _horn(M, first_eig)
        t = yb - (Rm @ xb[..., None]).squeeze(-1)
        c = torch.zeros(nv, 4, 4)
        c[:, :3, :3], c[:, :3, 3], c[:, 3, 3] = Rm.float(), t.float(), 1.0
        f = focal.clone()
        if shift_launch and li >= 1:      # the launch's outputs land one view late
            f, c = f.roll(1, 0), c.roll(1, 0)
        focal_out[v0:v0 + nv], c2w_out[v0:v0 + nv] = f, c
        v0 += nv
    return focal_out, c2w_out
