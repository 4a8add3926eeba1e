"""The case table of the stream-order tests (tests/test_stream_order_gpu.py, tests/test_stream_order_host.py): one case per entry point of
include/must3r_hip.h whose declaration ends in ``void* stream)``.  Building a case needs no GPU.

A case is a function that returns a ``Spec``:
  A, B     two complete, valid input sets (name -> CPU tensor) of the same shapes and other values; B is the decoy.  ``shared`` names the inputs that are the
           same in both on purpose (view tables, offsets, RoPE tables).
  ranges   name -> (lo, hi): every element of that input lies in [lo, hi) in both sets (positions, view tables, codebook and quadrant ids, offsets)
  bufs     name -> (shape, dtype) or a callable returning a byte count: the outputs and the scratch the caller owns; the tests fill them with PATTERN bytes
  outs     the names of ``d`` that are compared afterwards: output buffers and the inputs that are written in place (in/out)
  run(d)   one call (or one chain of calls on the same stream) on the device tensors ``d`` (inputs, bufs and whatever ``prepare`` added), through the Python
           wrapper where there is one and it does not synchronise by itself, through ctypes otherwise.  Tensors the wrapper allocates come back as a dict.
  prepare  optional, once after allocation and outside every timed region: device pointer tables

Every stream argument is ``_lib.stream_ptr(device)``, the current torch stream, in the wrappers and here (``ST``): the control of the GPU test replaces that one
function to send a call to the null stream.
"""
import ctypes as C
import math

import numpy as np
import torch

from must3r_amd import _lib

PATTERN = 0xA5
f32, f16, i16, i32, i64, u8, f64 = torch.float32, torch.float16, torch.int16, torch.int32, torch.int64, torch.uint8, torch.float64


class Spec:
    def __init__(self, inputs, run, outs=(), bufs=None, ranges=None, shared=(), prepare=None, no_inputs=False):
        self.A, self.B = inputs(0), inputs(1)
        self.run, self.outs, self.bufs, self.ranges, self.shared, self.prepare = run, tuple(outs), dict(bufs or {}), dict(ranges or {}), tuple(shared), prepare
        self.no_inputs = no_inputs


class Case:
    def __init__(self, name, entries, src, fn, syncs, reason, control):
        self.name, self.entries, self.src, self.fn, self.syncs, self.reason, self.control = name, tuple(entries), src, fn, syncs, reason, control
        self._spec = None

    def spec(self):
        if self._spec is None:
            self._spec = self.fn()
        return self._spec


CASES = []
# entry points with a stream argument that have no case: none.  (The fp8 attention flag is refused by the default build and has no entry point of its own;
# must3r_hip_set_profiling / must3r_hip_get_profile take no stream.)  At most 4 entries.
EXCLUDED = {}


def case(name, entries, src, syncs=False, reason=None, control=False):
    def deco(fn):
        CASES.append(Case(name, [e if e.startswith("must3r_hip_") else "must3r_hip_" + e for e in entries], src, fn, syncs, reason, control))
        return fn
    return deco


# ---- helpers
def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ST():
    return C.c_void_p(_lib.stream_ptr(torch.cuda.current_device()))


def L():
    return _lib.load()


def gen(seed, salt):
    return torch.Generator().manual_seed(7919 * salt + 31 * seed + 5)


def rn(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g) * scale


def split_w(Wf):
    hi = Wf.half()
    return torch.cat((hi, (Wf - hi.float()).half()), dim=1).contiguous()


def rope_tab(npos):
    t = torch.empty((npos, 16, 2), dtype=f32)
    _lib.check(L().must3r_hip_rope_table(100.0, 1.0, npos, C.c_void_p(t.data_ptr())))
    return t


def grid_pos(g, rows, npos):
    return torch.randint(0, npos, (rows, 2), generator=g, dtype=i64)


def nbytes(fn, *a):
    def f():
        n = fn(*a)
        assert n > 0, _lib.load().must3r_hip_last_error().decode()
        return n
    return f


def views_ranges(name, rows_q, rows_k):
    """a view table int32 [n][6] = q_row0, nq, kv_row0, nk, skip_lo, skip_hi: every entry inside [0, max(rows) + 1); check_views holds the rows themselves"""
    return {name: (0, max(rows_q, rows_k) + 1)}


def check_views(tab, rows_q, rows_k):
    for q0, nq, k0, nk, lo, hi in torch.as_tensor(tab).tolist():
        assert 0 <= q0 and q0 + nq <= rows_q and 0 <= k0 and k0 + nk <= rows_k and 0 <= lo <= hi <= nk, (q0, nq, k0, nk, lo, hi)


# =====================================================================================================================================================
# misc.hip: the output activation
# =====================================================================================================================================================
@case("postprocess", ["postprocess"], "misc.hip", control=True)
def _postprocess():
    """(no wrapper: engine.postprocess calls the _act forms)"""
    n = 1000

    def run(d):
        _lib.check(L().must3r_hip_postprocess(P(d["pm"]), P(d["p3"]), P(d["pl"]), P(d["cf"]), n, ST()))
    return Spec(lambda s: dict(pm=rn(gen(s, 1), n, 7)), run, outs=("p3", "pl", "cf"), bufs=dict(p3=((n, 3), f32), pl=((n, 3), f32), cf=((n,), f32)))


@case("postprocess_act", ["postprocess_act"], "misc.hip")
def _postprocess_act():
    from must3r_amd.engine import postprocess
    return Spec(lambda s: dict(pm=rn(gen(s, 2), 2, 37, 53, 7)), lambda d: postprocess(d["pm"], "linear"))


@case("postprocess_act_grad", ["postprocess_act_grad"], "misc.hip")
def _postprocess_act_grad():
    """(its only caller is the backward of an autograd function)"""
    n = 1000

    def inputs(s):
        g = gen(s, 3)
        return dict(pm=rn(g, n, 7), g3=rn(g, n, 3), gl=rn(g, n, 3), gc=rn(g, n))

    def run(d):
        _lib.check(L().must3r_hip_postprocess_act_grad(P(d["pm"]), _lib.ACT_NORM_EXP, P(d["g3"]), P(d["gl"]), P(d["gc"]), P(d["grad"]), n, ST()))
    return Spec(inputs, run, outs=("grad",), bufs=dict(grad=((n, 7), f32)))


# =====================================================================================================================================================
# cam.hip: activation + focal + pose (cooperative launch behind a slot fill)
# =====================================================================================================================================================
def _cam_pm(s):
    from must3r_amd.synthetic import make_cam_pointmaps
    with torch.random.fork_rng(devices=[]):
        return dict(pm=make_cam_pointmaps(2, 37, 53, seed=100 + s).contiguous())


@case("postprocess_cam", ["postprocess_cam"], "cam.hip", control=True)
def _postprocess_cam():
    V, H, W = 2, 37, 53

    def run(d):
        sc = d["scratch"]
        _lib.check(L().must3r_hip_postprocess_cam(P(d["pm"]), V, H, W, P(d["p3"]), P(d["pl"]), P(d["cf"]), P(d["focal"]), P(d["c2w"]), P(sc), sc.numel(), ST()))
    return Spec(_cam_pm, run, outs=("p3", "pl", "cf", "focal", "c2w"),
                bufs=dict(p3=((V, H, W, 3), f32), pl=((V, H, W, 3), f32), cf=((V, H, W), f32), focal=((V,), f32), c2w=((V, 4, 4), f32),
                          scratch=nbytes(lambda: L().must3r_hip_postprocess_cam_scratch_bytes(V, H, W))))


@case("postprocess_cam_act", ["postprocess_cam_act"], "cam.hip")
def _postprocess_cam_act():
    from must3r_amd.engine import postprocess
    return Spec(_cam_pm, lambda d: postprocess(d["pm"], compute_cam=True))


# =====================================================================================================================================================
# retrieval.hip: the six operators at (3, 48, 256)
# =====================================================================================================================================================
RB, RN, RC = 3, 48, 256


@case("affine", ["affine"], "retrieval.hip")
def _affine():
    from must3r_amd import retrieval

    def inputs(s):
        g = gen(s, 10)
        return dict(x=rn(g, RB, RN, RC), sub=rn(g, 1, RC).double(), B=(rn(g, RC, RC) / 16).double(), bias=rn(g, RC).double(), resid=rn(g, RB, RN, RC))
    return Spec(inputs, lambda d: dict(out=retrieval.affine(d["x"], d["sub"], d["B"], False, bias=d["bias"], resid=d["resid"], double=True)))


@case("row_norm", ["row_norm"], "retrieval.hip", control=True)
def _row_norm():
    """(called from inside RetrievalModel only)"""
    M = RB * RN

    def run(d):
        _lib.check(L().must3r_hip_row_norm(P(d["x"]), M, RC, P(d["out"]), ST()))
    return Spec(lambda s: dict(x=rn(gen(s, 11), M, RC)), run, outs=("out",), bufs=dict(out=((M,), f32)))


@case("l2_normalize", ["l2_normalize"], "retrieval.hip")
def _l2_normalize():
    from must3r_amd import retrieval

    def run(d):
        retrieval.l2_normalize(d["x"], -1)      # in place
    return Spec(lambda s: dict(x=rn(gen(s, 12), RB, RN, RC)), run, outs=("x",))


@case("layernorm_act_f32", ["layernorm_act_f32"], "retrieval.hip")
def _layernorm_act():
    M = RB * RN

    def inputs(s):
        g = gen(s, 13)
        return dict(x=rn(g, M, RC), gamma=1 + 0.1 * rn(g, RC), beta=0.1 * rn(g, RC))

    def run(d):
        from types import SimpleNamespace
        from must3r_amd import retrieval
        ln = SimpleNamespace(normalized_shape=(RC,), weight=d["gamma"], bias=d["beta"], eps=1e-5)      # what the wrapper reads of an nn.LayerNorm
        return dict(out=retrieval.layernorm_act(d["x"], ln, True))
    return Spec(inputs, run)


def _feat_attn(salt):
    def inputs(s):
        g = gen(s, salt)
        return dict(feat=rn(g, RB, RN, RC), attn=torch.rand((RB, RN), generator=g) + 0.1)
    return inputs


@case("topk_gather", ["topk_gather"], "retrieval.hip")
def _topk():
    from must3r_amd import retrieval

    def run(d):
        of, oa, oi = retrieval.how_select_local(d["feat"], d["attn"], 20)
        return dict(of=of, oa=oa, oi=oi)
    return Spec(_feat_attn(14), run)


@case("weighted_spoc", ["weighted_spoc"], "retrieval.hip")
def _spoc():
    from must3r_amd import retrieval
    return Spec(_feat_attn(15), lambda d: dict(out=retrieval.weighted_spoc(d["feat"], d["attn"])))


# =====================================================================================================================================================
# asmk.hip
# =====================================================================================================================================================
AK, AD, AM = 512, 256, 300


@case("asmk_quantize", ["asmk_centroid_sqnorm", "asmk_quantize"], "asmk.hip")
def _asmk_quantize():
    """the norms of the codebook, then the 5 nearest centroids of every row through the wrapper (its scratch is its own)"""
    from must3r_amd import asmk

    def inputs(s):
        g = gen(s, 20)
        return dict(feat=rn(g, AM, AD), codebook=rn(g, AK, AD))

    def run(d):
        _lib.check(L().must3r_hip_asmk_centroid_sqnorm(P(d["codebook"]), AK, AD, P(d["csq"]), ST()))
        return dict(ids=asmk.quantize(d["feat"], d["codebook"], 5, c_sqnorm=d["csq"]))
    return Spec(inputs, run, outs=("csq",), bufs=dict(csq=((AK,), f32)))


@case("asmk_aggregate_scores", ["asmk_aggregate", "asmk_scores"], "asmk.hip", control=True)
def _asmk_aggregate():
    """database (k_use 1) and query (k_use 5) aggregates of ragged images, then the scores; the wrapper of aggregate reads its counts back, so ctypes"""
    off = torch.tensor([0, 70, 71, 190, AM], dtype=i32)
    n = off.numel() - 1
    rows = int((off[1:] - off[:-1]).max())

    def inputs(s):
        g = gen(s, 21)
        return dict(feat=rn(g, AM, AD), codebook=rn(g, AK, AD), ids=torch.randint(0, AK, (AM, 5), generator=g, dtype=i32), off=off.clone())

    def run(d):
        lib = L()
        for side, k in (("q", 5), ("d", 1)):
            _lib.check(lib.must3r_hip_asmk_aggregate(P(d["feat"]), P(d["codebook"]), AK, AD, P(d["ids"]), 5, k, P(d["off"]), n, rows, P(d["w" + side]), P(d["b" + side]),
                                                     P(d["c" + side]), ST()))
        for normalize, out in ((1, "scores"), (0, "scores_raw")):      # (normalised, an image scores 1 against itself in both sets)
            _lib.check(lib.must3r_hip_asmk_scores(P(d["wq"]), P(d["bq"]), P(d["cq"]), P(d["off"]), 5, n, P(d["wd"]), P(d["bd"]), P(d["cd"]), P(d["off"]), 1, n, AD, 3.0, 0.0,
                                                  normalize, P(d[out]), ST()))
    bufs = dict(scores=((n, n), f64), scores_raw=((n, n), f64))
    for side, k in (("q", 5), ("d", 1)):
        bufs.update({"w" + side: ((AM * k,), i32), "b" + side: ((AM * k, AD // 32), i32), "c" + side: ((n,), i32)})
    # the slots behind an image's last word are never written: only the scores and the counts are compared
    return Spec(inputs, run, outs=("scores", "scores_raw", "cq", "cd"), bufs=bufs, ranges=dict(ids=(0, AK), off=(0, AM + 1)), shared=("off",))


# =====================================================================================================================================================
# nn.hip / nn_index.hip
# =====================================================================================================================================================
@case("nn_query", ["nn_query"], "nn.hip", control=True)
def _nn_query():
    """20000 database points: 10 splits of 2048 over the chip, merged through atomicMin on the bit patterns"""
    from must3r_amd import slam_nn

    def inputs(s):
        g = gen(s, 30)
        return dict(db=rn(g, 20000, 3), q=rn(g, 1000, 3))
    return Spec(inputs, lambda d: dict(out=slam_nn.nn_distances(d["db"], d["q"])))


@case("quadrant_ids", ["quadrant_ids"], "nn.hip")
def _quadrant_ids():
    from must3r_amd import slam_nn
    return Spec(lambda s: dict(pts=rn(gen(s, 31), 1000, 3)), lambda d: dict(out=slam_nn.quadrant_ids(d["pts"], [0.1, -0.2, 0.3], 3)))


@case("nn_index_bvh", ["nn_index_build", "nn_index_query"], "nn_index.hip")
def _nn_index_bvh():
    """through the searcher: the points and their quadrant ids appended to its store, the index built by the first query"""
    from must3r_amd import slam_nn
    cc = [0.1, -0.2, 0.3]

    def inputs(s):
        g = gen(s, 33)
        return dict(xyz=rn(g, 1000, 3), q=rn(g, 1000, 3))

    def run(d):
        b = slam_nn.BVH_hip(2)
        b.add_pts(d["xyz"], cam_center=cc)
        return dict(out=b.query_device(d["q"], cam_center=cc))
    return Spec(inputs, run)


@case("nn_index", ["nn_index_build", "nn_index_query"], "nn_index.hip", control=True)
def _nn_index():
    """the two entry points on buffers of the caller (the control needs them: the searcher's own copies would stay on the side stream)"""
    n, div = 1000, 2
    cc = (C.c_float * 3)(0.1, -0.2, 0.3)

    def inputs(s):
        g = gen(s, 32)
        return dict(xyz=rn(g, n, 3), qid=torch.randint(0, 2 * div * div, (n,), generator=g, dtype=i32), q=rn(g, n, 3))

    def run(d):
        lib = L()
        _lib.check(lib.must3r_hip_nn_index_build(P(d["xyz"]), P(d["qid"]), n, div, P(d["index"]), P(d["scratch"]), ST()))
        _lib.check(lib.must3r_hip_nn_index_query(P(d["index"]), P(d["q"]), n, cc, div, P(d["out"]), ST()))
    return Spec(inputs, run, outs=("out", "index"), ranges=dict(qid=(0, 2 * div * div)),
                bufs=dict(out=((n,), f32), index=nbytes(lambda: L().must3r_hip_nn_index_bytes(n, div)), scratch=nbytes(lambda: L().must3r_hip_nn_index_scratch_bytes(n))))


# =====================================================================================================================================================
# export.hip: count (synchronises), then the three scatters, on ragged views
# =====================================================================================================================================================
EXPORT_SHAPES = [(7, 13), (33, 37), (1, 5), (40, 64)]      # "ragged" of tests/test_export_gpu.py


@case("export", ["export_count", "export_scatter_points", "export_vertices", "export_scatter_faces"], "export.hip", syncs=True, control=True,
      reason="include/must3r_hip.h, must3r_hip_export_count: \"returns the totals per threshold ... after one small copy (the call synchronises `stream`)\"; "
             "only the launches in front of that synchronisation are held by the premise, every launch by the bits")
def _export():
    """point mode (GLB and PLY scatters of two thresholds), then mesh mode (vertices, faces).  Through ctypes on buffers of the largest size: the exporter sizes
    its buffers by the totals, which differ between the two input sets."""
    npix = sum(h * w for h, w in EXPORT_SHAPES)
    thr = (C.c_float * 2)(0.5, 1.2)

    def inputs(s):
        g = gen(s, 40)
        d = {}
        for i, (h, w) in enumerate(EXPORT_SHAPES):
            d.update({f"conf{i}": torch.rand((h, w), generator=g) * 2, f"pts{i}": rn(g, h, w, 3), f"rgb{i}": torch.rand((h, w, 3), generator=g)})
        return d
    mats = np.random.default_rng(3).standard_normal((len(EXPORT_SHAPES), 12))

    def table(d):
        t = (_lib.ExportView * len(EXPORT_SHAPES))()
        for i, (h, w) in enumerate(EXPORT_SHAPES):
            t[i].conf, t[i].pts, t[i].rgb, t[i].H, t[i].W = d[f"conf{i}"].data_ptr(), d[f"pts{i}"].data_ptr(), d[f"rgb{i}"].data_ptr(), h, w
            for j in range(12):
                t[i].M[j] = float(mats[i, j])
        return t

    def run(d):
        lib, t, n = L(), table(d), len(EXPORT_SHAPES)
        totals = (C.c_int64 * 2)()
        sc = d["scratch"]
        _lib.check(lib.must3r_hip_export_count(t, n, thr, 2, 0, P(sc), sc.numel(), totals, ST()))
        _lib.check(lib.must3r_hip_export_scatter_points(t, n, thr, 2, 0, _lib.EXPORT_GLB, P(sc), P(d["pos"]), P(d["col"]), P(d["mm"]), ST()))
        _lib.check(lib.must3r_hip_export_scatter_points(t, n, thr, 2, 1, _lib.EXPORT_PLY, P(sc), P(d["ply"]), None, P(d["mm2"]), ST()))
        scm = d["scratch_mesh"]
        _lib.check(lib.must3r_hip_export_count(t, n, thr, 2, 1, P(scm), scm.numel(), totals, ST()))
        _lib.check(lib.must3r_hip_export_vertices(t, n, 2, P(scm), P(d["vpos"]), P(d["vcol"]), P(d["mm3"]), ST()))
        _lib.check(lib.must3r_hip_export_scatter_faces(t, n, thr, 2, 0, P(scm), P(d["faces"]), ST()))

    def scratch(mesh):
        def f():
            v = (_lib.ExportView * len(EXPORT_SHAPES))()
            for i, (h, w) in enumerate(EXPORT_SHAPES):
                v[i].H, v[i].W = h, w
                v[i].conf = v[i].pts = v[i].rgb = 256      # sizes only: the pointers are not read
            n = L().must3r_hip_export_scratch_bytes(v, len(EXPORT_SHAPES), 2, mesh)
            assert n > 0, L().must3r_hip_last_error().decode()
            return n
        return f
    nquads = sum(max(h - 1, 0) * max(w - 1, 0) for h, w in EXPORT_SHAPES)
    return Spec(inputs, run, outs=("pos", "col", "mm", "ply", "mm2", "vpos", "vcol", "mm3", "faces"),
                bufs=dict(pos=((npix, 3), f32), col=((npix, 4), u8), mm=((6,), f32), ply=((npix, 16), u8), mm2=((6,), f32), vpos=((npix, 3), f32), vcol=((npix, 4), u8),
                          mm3=((6,), f32), faces=((4 * nquads, 3), i32), scratch=scratch(0), scratch_mesh=scratch(1)))


# =====================================================================================================================================================
# metrics.hip
# =====================================================================================================================================================
def _metrics_inputs(salt, B=2, V=2, H=7, W=13):
    def inputs(s):
        g = gen(s, salt)
        cam = torch.eye(4).repeat(B, 1, 1) + 0.05 * rn(g, B, 4, 4)
        cam[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
        w2c = torch.eye(4).repeat(B, V, 1, 1) + 0.05 * rn(g, B, V, 4, 4)
        w2c[:, :, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
        return dict(gt=rn(g, B, V, H, W, 3), cam=cam, w2c=w2c, pr=rn(g, B, V, H, W, 3), prl=rn(g, B, V, H, W, 3), conf=1 + torch.rand((B, V, H, W), generator=g),
                    valid=(torch.rand((B, V, H, W), generator=g) < 0.7).to(u8), pr_scale=1 + torch.rand((B,), generator=g))
    return inputs


def _metrics_kw(d):
    return dict(w2c=d["w2c"], pr_local=d["prl"], conf=d["conf"], pr_scale=d["pr_scale"], loss_in_log=True, alpha=0.2)


@case("metrics_loss", ["metrics_loss"], "metrics.hip")
def _metrics_loss():
    from must3r_amd import losses

    def run(d):
        counts, sums, pix = losses.loss_pass(d["gt"], d["cam"], d["pr"], d["valid"], per_pixel=True, **_metrics_kw(d))
        return dict(counts=counts, sums=sums, pix_g=pix[0], pix_l=pix[1], msk_g=pix[2], msk_l=pix[3])
    return Spec(_metrics_inputs(50), run)


@case("metrics_factor", ["metrics_factor"], "metrics.hip", control=True)
def _metrics_factor():
    """the median mode: a memset of the histograms, the distance pass, three histogram passes"""
    from must3r_amd import losses

    def inputs(s):
        g = gen(s, 51)
        return dict(pts=rn(g, 2, 2, 7, 13, 3), valid=(torch.rand((2, 2, 7, 13), generator=g) < 0.7).to(u8), trf=torch.eye(4).repeat(2, 1, 1) + 0.05 * rn(g, 2, 4, 4))

    def run(d):
        factor, dist = losses.norm_factor(d["pts"], d["valid"], "median_dis", trf=d["trf"], return_dist=True)
        return dict(factor=factor, dist=dist)
    return Spec(inputs, run)


@case("metrics_loss_grad", ["metrics_loss_grad"], "metrics.hip")
def _metrics_loss_grad():
    """the forward for its counts, then the backward with the scale path of both scenes (its reduction launches); the wrapper uploads `own` from pageable
    memory, so the argument blocks come from the wrapper's loss_args and the call is made here"""
    from must3r_amd import losses
    B, V, H, W = 2, 2, 7, 13
    base = _metrics_inputs(52)

    def inputs(s):
        d = base(s)
        d.update(w=torch.tensor([0.5 + s]), own=torch.ones((B,), dtype=u8))
        return d

    def run(d):
        lib = L()
        counts, _ = losses.loss_pass(d["gt"], d["cam"], d["pr"], d["valid"], **_metrics_kw(d))
        a, keep, _, _ = losses.loss_args(d["gt"], d["cam"], d["pr"], d["valid"], **_metrics_kw(d))
        n_valid = d["valid"].reshape(B, -1).sum(dim=1, dtype=i64)
        g = _lib.MetricsLossGradArgs()
        g.w_g, g.w_l, g.weighting, g.counts = P(d["w"]), P(d["w"]), _lib.LOSS_W_CONF, P(counts)
        g.factor_mode, g.n_own, g.own_factor, g.n_valid = _lib.NORM_AVG_DIS, B, P(d["own"]), P(n_valid)
        g.grad_pts, g.grad_local, g.grad_conf = P(d["gp"]), P(d["gl"]), P(d["gc"])
        sc = d["scratch"]
        _lib.check(lib.must3r_hip_metrics_loss_grad(C.byref(a), C.byref(g), P(sc), sc.numel(), ST()))
        return dict(counts=counts, n_valid=n_valid)
    return Spec(inputs, run, outs=("gp", "gl", "gc"), shared=("own",),
                bufs=dict(gp=((B, V, H, W, 3), f32), gl=((B, V, H, W, 3), f32), gc=((B, V, H, W), f32),
                          scratch=nbytes(lambda: L().must3r_hip_metrics_loss_grad_scratch_bytes(B, V, H, W))))


# =====================================================================================================================================================
# image.hip
# =====================================================================================================================================================
RESAMPLE_PAIRS = [((40, 56), (24, 32)), ((33, 47), (16, 20)), ((48, 64), (32, 48)), ((25, 31), (16, 16)), ((64, 48), (48, 32)), ((37, 53), (16, 32))]


def resample_descs(srcs, pairs):
    """descriptors of F32_CHW sources resampled whole to their target size, written one after the other; returns (descs, elements of the output)"""
    from must3r_amd import image
    descs, o = [], 0
    for src, ((h, w), (th, tw)) in zip(srcs, pairs):
        descs.append(image._desc(src, _lib.IMG_F32_CHW, 3, h, w, w, h * w, (0, 0, h, w), (th, tw), (0, 0, th, tw), o))
        o += 3 * th * tw
    return descs, o


def resample_inputs(pairs, salt):
    def inputs(s):
        g = gen(s, salt)
        return {f"src{i}": rn(g, 3, h, w) for i, ((h, w), _) in enumerate(pairs)}
    return inputs


def resample_run(pairs):
    from must3r_amd import image

    def run(d):
        srcs = [d[f"src{i}"] for i in range(len(pairs))]
        descs, _ = resample_descs(srcs, pairs)
        image._resample(_lib.RESAMPLE_AA_BILINEAR, descs, d["out"], srcs)
    return run


@case("resample", ["resample"], "image.hip", control=True)
def _resample():
    """two size pairs in one call: table upload through the pinned ring, one launch per pass"""
    pairs = RESAMPLE_PAIRS[:2]
    n = sum(3 * th * tw for _, (th, tw) in pairs)
    return Spec(resample_inputs(pairs, 60), resample_run(pairs), outs=("out",), bufs=dict(out=((n,), f32)))


# =====================================================================================================================================================
# model.hip: the operator-level entry points of the inference kernels (gemm.hip, attention.hip, misc.hip launchers)
# =====================================================================================================================================================
NPOS = 64


@case("op_gemm", ["op_gemm"], "model.hip", control=True)
def _op_gemm():
    """EPI_RESID_F32: out is read and written"""
    M, N, K = 200, 192, 128

    def inputs(s):
        g = gen(s, 70)
        return dict(A=rn(g, M, K).half(), W=(rn(g, N, K) / math.sqrt(K)).half(), bias=rn(g, N), out=rn(g, M, N))

    def run(d):
        _lib.check(L().must3r_hip_op_gemm(_lib.F16, _lib.EPI_RESID_F32, P(d["A"]), P(d["W"]), P(d["bias"]), P(d["out"]), M, N, K, K, N, None, None, 0, 0, None, 0, 0,
                                          0, 0, 0, 0, 0, ST()))
    return Spec(inputs, run, outs=("out",))


@case("op_gemm_sp", ["op_sparse24_pack", "op_gemm_sp"], "model.hip")
def _op_gemm_sp():
    M, N, K = 130, 256, 128

    def inputs(s):
        g = gen(s, 71)
        Wf = rn(g, N, K) / math.sqrt(K)
        return dict(A=rn(g, M, K).half(), Wf=Wf, W2=split_w(Wf), bias=rn(g, N))

    def run(d):
        lib = L()
        _lib.check(lib.must3r_hip_op_sparse24_pack(P(d["Wf"]), N, K, P(d["vals"]), P(d["idx"]), ST()))
        _lib.check(lib.must3r_hip_op_gemm_sp(_lib.EPI_STORE16, P(d["A"]), P(d["W2"]), P(d["vals"]), P(d["idx"]), P(d["bias"]), P(d["out"]), M, N, K, K, N, None, None, 0, 0, ST()))
    return Spec(inputs, run, outs=("out", "vals", "idx"), bufs=dict(out=((M, N), f16), vals=((K // 64, N, 32), f16), idx=((K // 64, N // 32, 64), i32)))


def _fold_inputs(salt, M, D, Kp, N, split_p, split_c, frag):
    """producer x += a Wp^T + bp (x16, copy, fragment sums of x - shift), consumer out = epi(LN(x) W^T + b) from them"""
    def inputs(s):
        g = gen(s, salt)
        Wp = rn(g, D, Kp) / math.sqrt(Kp)
        gam, bet = 1 + 0.3 * rn(g, D), 0.2 * rn(g, D)
        W, b = rn(g, N, D) / math.sqrt(D), rn(g, N)
        Wg = W * gam
        x = rn(g, M, D) * (1 + 3 * torch.rand((M, 1), generator=g))
        return dict(a=rn(g, M, Kp).half(), Wp=split_w(Wp) if split_p else Wp.half(), bp=rn(g, D), x=x, shift=x.mean(1).contiguous(),
                    Wg=split_w(Wg) if split_c else Wg.half(), s_n=Wg.double().sum(1).float(), c_n=(W.double() @ bet.double() + b.double()).float(),
                    pos=grid_pos(g, M, NPOS), tab=rope_tab(NPOS))
    return inputs


def _fold_bufs(M, D, N, frag):
    return dict(x16=((M, D), f16), cp=((M, D), f32), st=((M, D // frag, 2), f32), out=((M, N), f16))


@case("op_gemm_lnfold", ["op_gemm_lnfold"], "model.hip")
def _op_gemm_lnfold():
    """producer (EPI_RESID_F32, x in place) then the qkv consumer (RoPE, scaled q) on the same stream, at M = 196"""
    M, D, N = 196, 768, 2304

    def run(d):
        lib = L()
        _lib.check(lib.must3r_hip_op_gemm_lnfold(1, _lib.EPI_RESID_F32, P(d["a"]), P(d["Wp"]), P(d["bp"]), P(d["x"]), M, D, D, D, D, P(d["x16"]), P(d["cp"]), P(d["st"]),
                                                 None, None, 0.0, P(d["shift"]), 0, None, None, 0, 0, 0.0, 0, ST()))
        _lib.check(lib.must3r_hip_op_gemm_lnfold(1, _lib.EPI_QKV_ROPE, P(d["x16"]), P(d["Wg"]), P(d["c_n"]), P(d["out"]), M, N, D, D, N, None, None, None, P(d["st"]),
                                                 P(d["s_n"]), 1e-6, P(d["shift"]), 0, P(d["pos"]), P(d["tab"]), 2 * D, NPOS, 0.18, D, ST()))
    return Spec(_fold_inputs(72, M, D, D, N, True, True, 16), run, outs=("x", "x16", "cp", "st", "out", "shift"), bufs=_fold_bufs(M, D, N, 16),
                ranges=dict(pos=(0, NPOS)), shared=("tab",))


@case("op_gemm_lnfold_ex", ["op_gemm_lnfold_ex"], "model.hip")
def _op_gemm_lnfold_ex():
    """the plain-weight forms: an fc2-like producer (K = 256) and the fc1 consumer (GELU) that starts the shift (ln_shift_init)"""
    M, D, Kp, N = 196, 768, 256, 768

    def run(d):
        lib = L()
        p = _lib.LnFoldOp()
        p.dtype, p.epi, p.A, p.W, p.bias, p.out = 1, _lib.EPI_RESID_F32, d["a"].data_ptr(), d["Wp"].data_ptr(), d["bp"].data_ptr(), d["x"].data_ptr()
        p.M, p.N, p.K, p.lda, p.ldc, p.wsplit = M, D, Kp, Kp, D, 0
        p.x16_out, p.copy32_out, p.stats_out = d["x16"].data_ptr(), d["cp"].data_ptr(), d["st"].data_ptr()
        _lib.check(lib.must3r_hip_op_gemm_lnfold_ex(C.byref(p), ST()))
        c = _lib.LnFoldOp()
        c.dtype, c.epi, c.A, c.W, c.bias, c.out = 1, _lib.EPI_STORE16_GELU, d["x16"].data_ptr(), d["Wg"].data_ptr(), d["c_n"].data_ptr(), d["out"].data_ptr()
        c.M, c.N, c.K, c.lda, c.ldc, c.wsplit = M, N, D, D, N, 0
        c.ln_stats, c.ln_s, c.ln_eps, c.ln_shift, c.ln_shift_init = d["st"].data_ptr(), d["s_n"].data_ptr(), 1e-6, d["shift_out"].data_ptr(), 1
        _lib.check(lib.must3r_hip_op_gemm_lnfold_ex(C.byref(c), ST()))
    bufs = _fold_bufs(M, D, N, 16)
    bufs["shift_out"] = ((M,), f32)
    return Spec(_fold_inputs(73, M, D, Kp, N, False, False, 16), run, outs=("x", "x16", "cp", "st", "out", "shift_out"), bufs=bufs, ranges=dict(pos=(0, NPOS)),
                shared=("tab",))


@case("op_gemm_fold256", ["op_gemm_fold256"], "model.hip")
def _op_gemm_fold256():
    """the fold on the 256 x 256 tiles, plain weights: producer (one row tile) and the GELU consumer"""
    M, D, N = 256, 768, 768

    def run(d):
        lib = L()
        _lib.check(lib.must3r_hip_op_gemm_fold256(_lib.EPI_RESID_F32, 0, P(d["a"]), P(d["Wp"]), None, None, P(d["bp"]), P(d["x"]), M, D, D, D, D, P(d["x16"]), P(d["cp"]),
                                                  P(d["st"]), None, None, 0.0, P(d["shift"]), None, None, 0, 0, 0.0, 0, ST()))
        _lib.check(lib.must3r_hip_op_gemm_fold256(_lib.EPI_STORE16_GELU, 0, P(d["x16"]), P(d["Wg"]), None, None, P(d["c_n"]), P(d["out"]), M, N, D, D, N, None, None, None,
                                                  P(d["st"]), P(d["s_n"]), 1e-6, P(d["shift"]), None, None, 0, 0, 0.0, 0, ST()))
    return Spec(_fold_inputs(74, M, D, D, N, False, False, 64), run, outs=("x", "x16", "cp", "st", "out", "shift"), bufs=_fold_bufs(M, D, N, 64),
                ranges=dict(pos=(0, NPOS)), shared=("tab",))


@case("op_gemm_ex", ["op_gemm_ex"], "model.hip")
def _op_gemm_ex():
    """grouped kv_all of tests/gemm_forms.py: L = 3 weight groups x S = 4 scenes of 12 rows, every problem to its own slot of the output through out_table"""
    import gemm_forms as F
    c = F.CASE["kv_all-L3-S4-r12"]
    Pn, M, N, K, S = c["P"], c["M"], c["N"], c["K"], c["S"]

    def inputs(s):
        ops = F.make_operands(c, "fp16", "plain", "cpu", seed=s)
        return dict(A=ops["A"], W=ops["W"], bias=ops["bias"])

    def prepare(d):
        d["table"] = torch.tensor([d["out"][F.slot_of(c, g)].data_ptr() for g in range(Pn)], dtype=i64).to(d["out"].device)

    def run(d):
        op = _lib.GemmOp()
        op.dtype, op.epi, op.A, op.W, op.bias = 1, c["epi"], d["A"].data_ptr(), d["W"].data_ptr(), d["bias"].data_ptr()
        op.M, op.N, op.K, op.lda, op.ldc = M, N, K, K, N
        op.batch, op.strideA, op.out_table, op.wdiv, op.strideW, op.strideB = Pn, M * K, d["table"].data_ptr(), S, N * K, N
        _lib.check(L().must3r_hip_op_gemm_ex(C.byref(op), ST()))
    return Spec(inputs, run, outs=("out",), bufs=dict(out=((Pn, M, N), f16)), prepare=prepare)


ATT_VIEWS = [[0, 70, 0, 200, 0, 0], [70, 70, 200, 200, 10, 50]]
ATT_RQ, ATT_RK, ATT_H = 140, 400, 2


def _att_inputs(salt):
    def inputs(s):
        g = gen(s, salt)
        D = ATT_H * 64
        return dict(Q=rn(g, ATT_RQ, D).half(), K=rn(g, ATT_RK, D).half(), V=rn(g, ATT_RK, D).half(), views=torch.tensor(ATT_VIEWS, dtype=i32))
    return inputs


@case("op_attention", ["op_attention"], "model.hip")
def _op_attention():
    """the single pass, then split-KV with nsplit = 3: (m, l) pre-fill, the partial kernels and attn_combine_kernel"""
    D = ATT_H * 64

    def run(d):
        lib = L()
        a = (P(d["Q"]), P(d["K"]), P(d["V"]))
        _lib.check(lib.must3r_hip_op_attention(1, *a, P(d["O1"]), D, D, D, D, ATT_H, P(d["views"]), 2, 70, 1, None, ATT_RQ, ST()))
        _lib.check(lib.must3r_hip_op_attention(1, *a, P(d["O3"]), D, D, D, D, ATT_H, P(d["views"]), 2, 70, 3, P(d["scratch"]), ATT_RQ, ST()))
    return Spec(_att_inputs(75), run, outs=("O1", "O3"), shared=("views",), ranges=views_ranges("views", ATT_RQ, ATT_RK),
                bufs=dict(O1=((ATT_RQ, D), f16), O3=((ATT_RQ, D), f16), scratch=nbytes(lambda: L().must3r_hip_attention_scratch_bytes(3, ATT_RQ, ATT_H))))


@case("op_attention_ex", ["op_attention_ex"], "model.hip")
def _op_attention_ex():
    """one context-parallel slot: the local partial (stage 1, nsplit = 2) into the slot, then the final merge (stage 3) into O"""
    D = ATT_H * 64

    def op(d):
        o = _lib.AttnOp()
        o.dtype, o.Q, o.K, o.V = 1, d["Q"].data_ptr(), d["K"].data_ptr(), d["V"].data_ptr()
        o.ldq = o.ldk = o.ldv = o.ldo = D
        o.heads, o.views_dev, o.n_views, o.max_nq, o.max_nk, o.q_prescaled = ATT_H, d["views"].data_ptr(), 2, 70, 200, 0
        o.total_q_rows, o.dense_rows = ATT_RQ, 1
        o.slot_o, o.slot_ml = d["slot_o"].data_ptr(), d["slot_ml"].data_ptr()
        return o

    def run(d):
        lib = L()
        o = op(d)
        o.stage, o.nsplit, o.scratch = 1, 2, d["scratch"].data_ptr()
        _lib.check(lib.must3r_hip_op_attention_ex(C.byref(o), ST()))
        o = op(d)
        o.stage, o.O, o.nslots, o.stride_o, o.stride_ml = 3, d["O"].data_ptr(), 1, ATT_RQ * D, ATT_RQ * ATT_H * 2
        _lib.check(lib.must3r_hip_op_attention_ex(C.byref(o), ST()))
    return Spec(_att_inputs(76), run, outs=("O", "slot_o", "slot_ml"), shared=("views",), ranges=views_ranges("views", ATT_RQ, ATT_RK),
                bufs=dict(O=((ATT_RQ, D), f16), slot_o=((ATT_RQ, D), f32), slot_ml=((ATT_RQ, ATT_H, 2), f32),
                          scratch=nbytes(lambda: L().must3r_hip_attention_scratch_bytes(2, ATT_RQ, ATT_H))))


def _ln_inputs(salt, M, Cc, groups):
    def inputs(s):
        g = gen(s, salt)
        return dict(x=rn(g, M, Cc) + rn(g, M, 1), add=rn(g, M // groups, Cc), w=1 + 0.1 * rn(g, groups, Cc), b=0.1 * rn(g, groups, Cc))
    return inputs


@case("op_layernorm", ["op_layernorm"], "model.hip")
def _op_layernorm():
    M, Cc = 70, 768

    def run(d):
        _lib.check(L().must3r_hip_op_layernorm(1, P(d["x"]), P(d["add"]), P(d["w"]), P(d["b"]), P(d["o16"]), P(d["lo"]), P(d["o32"]), P(d["c32"]), M, Cc, 1e-6, ST()))
    return Spec(_ln_inputs(77, M, Cc, 1), run, outs=("o16", "lo", "o32", "c32"), bufs=dict(o16=((M, Cc), f16), lo=((M, Cc), f16), o32=((M, Cc), f32), c32=((M, Cc), f32)))


@case("op_layernorm_ex", ["op_layernorm_ex"], "misc.hip")
def _op_layernorm_ex():
    """the grouped form: two groups of 35 rows with their own weights, add on the first group only, and the row means"""
    M, Cc = 70, 768

    def run(d):
        o = _lib.LnOp()
        o.dtype, o.x, o.add, o.w, o.b = 1, d["x"].data_ptr(), d["add"].data_ptr(), d["w"].data_ptr(), d["b"].data_ptr()
        o.out16, o.out32, o.copy32, o.mean_out = d["o16"].data_ptr(), d["o32"].data_ptr(), d["c32"].data_ptr(), d["mean"].data_ptr()
        o.M, o.C, o.eps, o.rows_per_group, o.add_groups = M, Cc, 1e-6, 35, 1
        _lib.check(L().must3r_hip_op_layernorm_ex(C.byref(o), ST()))
    return Spec(_ln_inputs(78, M, Cc, 2), run, outs=("o16", "o32", "c32", "mean"), bufs=dict(o16=((M, Cc), f16), o32=((M, Cc), f32), c32=((M, Cc), f32), mean=((M,), f32)))


@case("op_im2col", ["op_im2col"], "model.hip")
def _op_im2col():
    V, H, W = 2, 48, 64

    def run(d):
        _lib.check(L().must3r_hip_op_im2col(1, P(d["img"]), P(d["out"]), V, H, W, ST()))
    return Spec(lambda s: dict(img=rn(gen(s, 79), V, 3, H, W)), run, outs=("out",), bufs=dict(out=((V * (H // 16) * (W // 16), 768), f16)))


@case("op_cast", ["op_cast"], "model.hip")
def _op_cast():
    n = 1000

    def run(d):
        _lib.check(L().must3r_hip_op_cast(1, P(d["x"]), P(d["hi"]), P(d["lo"]), n, ST()))
    return Spec(lambda s: dict(x=rn(gen(s, 80), n)), run, outs=("hi", "lo"), bufs=dict(hi=((n,), f16), lo=((n,), f16)))


@case("debug_tr_probe", ["debug_tr_probe"], "model.hip")
def _tr_probe():
    """no input: the decoy is the pattern in the output, which the side-stream run writes again behind the delay"""
    def run(d):
        _lib.check(L().must3r_hip_debug_tr_probe(P(d["out"]), ST()))
    return Spec(lambda s: {}, run, outs=("out",), bufs=dict(out=((256,), i16)), no_inputs=True)


# =====================================================================================================================================================
# model.hip: the two forwards through the modules
# =====================================================================================================================================================
_modules = {}


def tiny_modules():
    """HIP-backed encoder and decoder of the tiny geometry with the seeded synthetic weights (tests/test_model_gpu.py build)"""
    if "m" not in _modules:
        import must3r_amd.model as M
        from must3r_amd import synthetic as S
        from must3r_amd.config import TINY as cfg
        enc = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads)
        dec = M.MUSt3R(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth, num_heads=cfg.dec_heads,
                       feedback_type="single_mlp", memory_mode="kv", landscape_only=False)
        enc.load_state_dict(S.make_encoder_state_dict(cfg, 0), strict=True)
        dec.load_state_dict(S.make_decoder_state_dict(cfg, 0), strict=True)
        _modules["m"] = (enc.cuda().eval(), dec.cuda().eval())
    return _modules["m"]


TINY_V, TINY_H, TINY_W = 4, 48, 64


@case("encode_decode", ["encode", "decode"], "model.hip", control=True)
def _encode_decode():
    """tiny_48x64_v4 through the modules: the encoder, one memory update of two views from an empty memory, one render of all four against it"""
    ts = torch.tensor([[TINY_H, TINY_W]] * TINY_V, dtype=i64)

    def inputs(s):
        from must3r_amd import synthetic as S
        return dict(img=S.make_images(TINY_V, TINY_H, TINY_W, s)[0])

    def run(d):
        enc, dec = tiny_modules()
        x, pos = enc(d["img"], ts)
        mem, upd = dec(x[:2].unsqueeze(0), pos[:2].unsqueeze(0), ts[:2].unsqueeze(0), None)
        _, ren = dec(x.unsqueeze(0), pos.unsqueeze(0), ts.unsqueeze(0), mem, render=True)
        out = dict(x=x, pos=pos, update=upd, render=ren)
        out.update({f"mem{i}": m for i, m in enumerate(mem[0])})
        return out
    return Spec(inputs, run)


# =====================================================================================================================================================
# train_head.hip
# =====================================================================================================================================================
def _head_inputs(s):
    import head_ref
    c = head_ref.make_case(1, 32, 48, D=256, seed=s)
    return {k: c[k] for k in ("x", "gamma", "beta", "W", "b", "G")}


@case("head_forward", ["head_forward"], "train_head.hip", control=True)
def _head_forward():
    from must3r_amd import train_head
    return Spec(_head_inputs, lambda d: dict(pm=train_head.head_forward(d["x"], d["gamma"], d["beta"], d["W"], d["b"], 1, 32, 48)))


@case("op_head_linear", ["op_head_linear"], "train_head.hip")
def _head_linear():
    from must3r_amd import train_head
    return Spec(_head_inputs, lambda d: dict(pm=train_head.head_linear(d["x"], d["W"], d["b"], 1, 32, 48)))


@case("head_grad", ["head_grad"], "train_head.hip")
def _head_grad():
    from must3r_amd import train_head
    import head_ref

    def run(d):
        return dict(zip(head_ref.NAMES, train_head.head_grad(d["x"], d["gamma"], d["beta"], d["W"], d["G"], 1, 32, 48)))
    return Spec(_head_inputs, run)


@case("linear_grad", ["op_linear_dgrad_f32", "op_linear_wgrad_f32"], "train_head.hip")
def _linear_grad():
    """150 x 192 x 128: the data gradient, then the weight gradient with its scratch reduction"""
    from must3r_amd import train_block

    def inputs(s):
        g = gen(s, 90)
        return dict(x=rn(g, 150, 128), W=rn(g, 192, 128) / 11, dy=rn(g, 150, 192))
    return Spec(inputs, lambda d: dict(zip(("dx", "dW", "db"), train_block.linear_grad(d["x"], d["W"], d["dy"]))))


def _lng_inputs(salt):
    def inputs(s):
        g = gen(s, salt)
        return dict(x=rn(g, 70, 128) + rn(g, 70, 1), gamma=1 + 0.1 * rn(g, 128), dy=rn(g, 70, 128), add=rn(g, 70, 128))
    return inputs


@case("op_layernorm_grad", ["op_layernorm_grad"], "train_head.hip")
def _ln_grad():
    from must3r_amd import train_block
    return Spec(_lng_inputs(91), lambda d: dict(zip(("dx", "dgamma", "dbeta"), train_block.layernorm_grad(d["x"], d["gamma"], d["dy"], 1e-6))))


@case("op_layernorm_grad_add", ["op_layernorm_grad_add"], "train_head.hip")
def _ln_grad_add():
    from must3r_amd import train_block
    return Spec(_lng_inputs(92), lambda d: dict(zip(("dx", "dgamma", "dbeta"), train_block.layernorm_grad(d["x"], d["gamma"], d["dy"], 1e-6, add=d["add"]))))


# =====================================================================================================================================================
# train_attention.hip: self_ragged of tests/attn_grad_ref.py (q, k, v the column blocks of one packed tensor; the table goes up through a pinned buffer)
# =====================================================================================================================================================
def attn_train_inputs(s):
    import attn_grad_ref
    c = attn_grad_ref._tensors(210, 210, 2, 11 + 100 * s, 2.0, packed=True)
    return dict(qkv=c["qkv"].contiguous(), dO=c["dO"].contiguous())


def attn_train_table(views=None):
    from must3r_amd.train_attention import self_views
    return torch.tensor(self_views(1, 3, 70) if views is None else views, dtype=i32)


ATTN_TABLES = [[[b * 70, 70, b * 70, 70, 0, 0] for b in range(3)], [[0, 210, 0, 210, 0, 0]], [[0, 70, 0, 140, 0, 0], [70, 140, 0, 140, 20, 60]]]      # three tables over 210 rows


def _qkv(d):
    return d["qkv"][:, :128], d["qkv"][:, 128:256], d["qkv"][:, 256:]


@case("attn_forward_f32", ["attn_forward_f32"], "train_attention.hip", control=True)
def _attn_forward_f32():
    from must3r_amd import train_attention
    tab = attn_train_table()
    check_views(tab, 210, 210)

    def run(d):
        o, lse = train_attention.attention_forward(*_qkv(d), tab, 2, want_lse=True)
        return dict(O=o, lse=lse)
    return Spec(attn_train_inputs, run)


@case("attn_grad", ["attn_grad"], "train_attention.hip")
def _attn_grad():
    from must3r_amd import train_attention
    tab = attn_train_table()

    def run(d):
        return dict(zip(("dQ", "dK", "dV"), train_attention.attention_grad(*_qkv(d), d["dO"], tab, 2)))
    return Spec(attn_train_inputs, run)


# =====================================================================================================================================================
# train_block.hip
# =====================================================================================================================================================
@case("op_linear_f32", ["op_linear_f32"], "train_block.hip", control=True)
def _op_linear_f32():
    """LIN_BIAS_RES with res aliasing out: read and written"""
    from must3r_amd import train_block

    def inputs(s):
        g = gen(s, 100)
        return dict(x=rn(g, 150, 128), W=rn(g, 192, 128) / 11, b=rn(g, 192), res=rn(g, 150, 192))

    def run(d):
        train_block.linear_forward(d["x"], d["W"], d["b"], epi=_lib.LIN_BIAS_RES, res=d["res"], out=d["res"])
    return Spec(inputs, run, outs=("res",))


@case("op_layernorm_f32", ["op_layernorm_f32"], "train_block.hip")
def _op_layernorm_f32():
    from must3r_amd import train_block

    def inputs(s):
        g = gen(s, 101)
        return dict(x=rn(g, 70, 128) + rn(g, 70, 1), gamma=1 + 0.1 * rn(g, 128), beta=0.1 * rn(g, 128))
    return Spec(inputs, lambda d: dict(y=train_block.layernorm_forward(d["x"], d["gamma"], d["beta"], 1e-6)))


@case("op_gelu_f32", ["op_gelu_f32"], "train_block.hip")
def _op_gelu():
    from must3r_amd import train_block
    return Spec(lambda s: dict(z=rn(gen(s, 102), 70, 100, scale=2.0)), lambda d: dict(zip(("g", "dg"), train_block.gelu_eval(d["z"]))))


@case("op_gelu_grad_f32", ["op_gelu_grad_f32"], "train_block.hip")
def _op_gelu_grad():
    """the out=dh form: dh is read and written"""
    from must3r_amd import train_block

    def inputs(s):
        g = gen(s, 103)
        return dict(dh=rn(g, 70, 100), z=rn(g, 70, 100, scale=2.0))

    def run(d):
        train_block.gelu_grad(d["dh"], d["z"], out=d["dh"])
    return Spec(inputs, run, outs=("dh",))


@case("op_rope_f32", ["op_rope_f32"], "train_block.hip")
def _op_rope():
    """in place over the q | k blocks of a packed [70][384]"""
    from must3r_amd import train_block

    def inputs(s):
        g = gen(s, 104)
        return dict(t=rn(g, 70, 384), pos=grid_pos(g, 70, NPOS), tab=rope_tab(NPOS))

    def run(d):
        train_block.rope_rows(d["t"], d["pos"], d["tab"], 256)
    return Spec(inputs, run, outs=("t",), ranges=dict(pos=(0, NPOS)), shared=("tab",))


BLOCK_GEOM = (128, 2, 512, (70, 64, 17), 41)                    # d128_ragged of tests/test_block_grad_gpu.py
NO_VIEW_ROWS, NO_VIEW_TABLE = 80, [[5, 40, 5, 40, 0, 0], [45, 30, 45, 30, 0, 0]]      # test_rows_of_no_view_attend_nothing: rows [0, 5) and [75, 80) of no view


def _block_inputs(which, rows=None):
    import block_ref

    def inputs(s):
        D, heads, hidden, tokens, seed = BLOCK_GEOM
        c = block_ref.make_case(D, heads, hidden, tokens, seed + 1000 * s)
        sl = slice(0, c["M"] if rows is None else rows)
        d = dict(x=c["x"][sl].contiguous(), dy=c["dy"][sl].contiguous())
        d.update({k: c["params"][k] for k in block_ref.WHICH[which]})
        if which == "attn":
            d.update(pos=(c["pos"][sl] + 3 * s).contiguous(), tab=rope_tab(NPOS))      # the decoy's grid lies 3 cells further out
        return d
    return inputs


@case("mlp_sublayer", ["mlp_sublayer_forward", "mlp_sublayer_grad"], "train_block.hip")
def _mlp_sublayer():
    from must3r_amd import train_block
    import block_ref

    def run(d):
        p = [d[k] for k in block_ref.MLP_PARAMS]
        out = dict(out=train_block.mlp_forward(d["x"], *p))
        out.update(zip(train_block.MLP_OUTPUTS, train_block.mlp_grad(d["x"], *p, d["dy"])))
        return out
    return Spec(_block_inputs("mlp"), run)


@case("attn_sublayer", ["attn_sublayer_forward", "attn_sublayer_grad"], "train_block.hip")
def _attn_sublayer():
    """rows of no view in front and behind: both "rows of no view" memsets run.  The forms under check_positions (its .tolist() synchronises)"""
    from must3r_amd import train_block
    import block_ref
    tab = torch.tensor(NO_VIEW_TABLE, dtype=i32)
    check_views(tab, NO_VIEW_ROWS, NO_VIEW_ROWS)

    def run(d):
        p = [d[k] for k in block_ref.ATTN_PARAMS]
        out = dict(out=train_block.attn_forward(d["x"], d["pos"], tab, d["tab"], *p))
        out.update(zip(train_block.ATTN_OUTPUTS, train_block.attn_grad(d["x"], d["pos"], tab, d["tab"], *p, d["dy"])))
        return out
    return Spec(_block_inputs("attn", NO_VIEW_ROWS), run, ranges=dict(pos=(0, NPOS)), shared=("tab",))


CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
SYNCS = {c.name for c in CASES if c.syncs}
SOURCES = sorted({c.src for c in CASES})
