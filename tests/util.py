import os

import numpy as np
import torch

from conftest import GOLDEN


def rel_inf(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


# Tolerances of the HIP path against the reference / fp32 oracle, relative = ||d||_inf / ||ref||_inf.
#  fp16w2 (fp16 operands, split weights): the north-star tolerance, BASELINE.json "pointmaps within 1e-3 relative of
#          reference" (measured ~4e-4).
#  fp16   (single-pass fp16): measured 0.8-1.5e-3, i.e. AT the target but without margin -> asserted at 2e-3.
#  bf16   (what BASELINE.json's configs name): the reference's OWN bf16-autocast path is 1.05e-2 away from its fp32
#          path on this network; the HIP bf16 path (fp32 residual stream) must stay inside that
#          envelope (+10% for the max-norm's sampling noise; measured 6-11e-3).
#  fp16wa (fp16 operands, split weights everywhere but in the Mlp Linears): the north-star tolerance as well (emulated 6e-4,
#          scripts/emul/gemm_precision.py; measured: profiles/).
TOL = {"fp16w2": 1.0e-3, "fp16wa": 1.0e-3, "fp16": 2.0e-3, "bf16": 1.15e-2}
PRECISIONS = ("fp16w2", "fp16wa", "fp16", "bf16")
# the module default (what bench.py times) against the real-reference fixture of the benched scene, worst single view.
# r05: each view's error over the fixture's stored (every 8th) pixels is normalised by that view's max |value| over ALL its pixels
# and channels (`update_vmax` / `render_vmax`, written by oracle/make_golden.py from the full-resolution reference output) -- the normalisation of
# bench.py's all-pixel `parity_vs_cpu_oracle` figure (6.3-7.2e-4) -- instead of by the max of the sample (r04: 9.45e-4 against 1.0e-3, a 5 % margin that was
# an artefact of the sub-sampled range).  Asserted at 8e-4; measured figures in profiles/r05_test_metrics.jsonl.
# (in r04 units -- error / range of the SAMPLED pixels, which is 1.3-1.7x smaller than the full-resolution range -- this gate sits at ~1.3e-3, i.e. it is NOT
# tighter than r04's 1.0e-3; what makes it a real regression gate is its distance from the measured figures: sampled pixels 5.9-6.0e-4, and since r06 the reference's worst
# update / render views at FULL resolution -- tests/golden/must3r512_v20_fullviews.npz, asserted at the same 8e-4 -- 6.0-7.3e-4: profiles/r06_test_metrics.jsonl.)
TOL_DEFAULT_FIXTURE = 8.0e-4


def rel_inf_view(a_sub, ref_sub, vmax):
    """||a - ref||_inf over the stored pixels of one view / that view's full-resolution max |ref| (fixture key *_vmax)."""
    a, b = torch.as_tensor(a_sub).double(), torch.as_tensor(ref_sub).double()
    return ((a - b).abs().max() / max(float(vmax), 1e-30)).item()


from must3r_amd.synthetic import make_cam_pointmaps as cam_scene  # noqa: E402,F401


# ----------------------------------------------------------------------------------------------------------------------
# The reference's side of tests/test_oracle_vs_reference.py.  Where the reference tree exists (conftest.HAS_REFERENCE) every
# value is computed live, as it always was; with M3R_RECORD_REFERENCE=1 it is also kept, in call order, and the whole set is
# written to tests/golden/reference_values.pt.xz (torch.save, xz-compressed).  Elsewhere the tests read those values back, so
# the restatements are checked against the reference's own outputs without its source.  To keep the file small, a value
# recorded with ``sample=True`` keeps each floating-point tensor of more than SAMPLE_MIN elements as every SAMPLE_STRIDE-th
# element of its flattened form (17 is coprime to the 7 pointmap channels and to the 128 / 256 feature widths, so every channel
# of every pixel or token row is reached), and the tests compare ``ref.px(ours)``, the same sample of their own tensor.  Values
# a test only compares for equality are recorded as ``digest(value)``.
# ----------------------------------------------------------------------------------------------------------------------
REFERENCE_VALUES = os.path.join(GOLDEN, "reference_values.pt.xz")
RECORD_REFERENCE = os.environ.get("M3R_RECORD_REFERENCE") == "1"
SAMPLE_STRIDE = 17
SAMPLE_MIN = 1024
_recorded = None


def _stored(v):
    """a copy of v that later in-place updates of the live objects cannot change"""
    if torch.is_tensor(v):
        return v.detach().clone()
    if isinstance(v, np.ndarray):
        return v.copy()
    if isinstance(v, dict):
        return {k: _stored(u) for k, u in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_stored(u) for u in v)
    return v


def _sample(v):
    if torch.is_tensor(v) and v.is_floating_point() and v.numel() > SAMPLE_MIN:
        return v.detach().reshape(-1)[::SAMPLE_STRIDE]
    if isinstance(v, dict):
        return {k: _sample(u) for k, u in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_sample(u) for u in v)
    return v


def digest(v):
    """v with every tensor / array replaced by (kind, shape, dtype, sha256 of its bytes): equal digests = bit-equal values"""
    import hashlib
    if isinstance(v, dict):
        return {k: digest(u) for k, u in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(digest(u) for u in v)
    if torch.is_tensor(v):
        t = v.detach().contiguous()
        return ("tensor", tuple(t.shape), str(t.dtype), hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest())
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return ("ndarray", a.shape, str(a.dtype), hashlib.sha256(a.tobytes()).hexdigest())
    return v


def _load_reference_values():
    import io
    import lzma
    with open(REFERENCE_VALUES, "rb") as f:
        return torch.load(io.BytesIO(lzma.decompress(f.read())), weights_only=False)


def reference_values():
    global _recorded
    if _recorded is None:
        _recorded = {} if RECORD_REFERENCE else _load_reference_values()
    return _recorded


def save_reference_values():
    if RECORD_REFERENCE and _recorded:
        import io
        import lzma
        vals = _load_reference_values() if os.path.exists(REFERENCE_VALUES) else {}
        vals.update(_recorded)
        buf = io.BytesIO()
        torch.save(dict(sorted(vals.items())), buf)
        with open(REFERENCE_VALUES, "wb") as f:
            f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))


class Reference:
    """``ref(lambda: <reference expression>)`` is the expression's value: computed live where the reference tree exists (and
    recorded with M3R_RECORD_REFERENCE=1), read back in call order elsewhere.  ``ref.live(lambda: ...)`` builds a reference
    object only the live runs use (None otherwise)."""

    def __init__(self, key):
        from conftest import HAS_REFERENCE
        self.is_live = HAS_REFERENCE
        self.i = 0
        if RECORD_REFERENCE:
            self.vals = reference_values()[key] = []
        elif not self.is_live:
            vals = reference_values()
            assert key in vals, f"{key}: not in {os.path.relpath(REFERENCE_VALUES)}; record it with M3R_RECORD_REFERENCE=1"
            self.vals = vals[key]

    def live(self, fn):
        return fn() if self.is_live else None

    def px(self, t):
        """our side of a comparison with a value recorded with ``sample=True``"""
        return t if self.is_live else _sample(t)

    def __call__(self, fn, sample=False):
        if self.is_live:
            try:
                v = fn()
            except Exception as e:
                if RECORD_REFERENCE:
                    self.vals.append({"__raised__": type(e).__name__})
                raise
            if RECORD_REFERENCE:
                self.vals.append(_stored(_sample(v) if sample else v))
            return v
        v = self.vals[self.i]
        self.i += 1
        if isinstance(v, dict) and "__raised__" in v:
            import builtins
            raise getattr(builtins, v["__raised__"])(f"{v['__raised__']} raised by the reference (recorded)")
        return v
