"""CPU: the host side of the mixed-orientation head -- the yardstick tests/head_ar_ref.py against the reference's own ``transpose_to_landscape(LinearHead(...),
activate=True)`` (live where the reference tree exists, from the recorded fixture tests/golden/head_many_ar_d64.npz elsewhere), the indexing of a portrait
view element by element, the LDS map and the index arithmetic of csrc/train_head.hip's head_turn_kernel replayed, the ABI surface of the two new entry points
and their refusals, and the Python refusals (no compute calls: no GPU here)."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import head_ar_ref as HAR
import head_ref as HR
from conftest import GOLDEN, HAS_REFERENCE, ROOT
from must3r_amd import _lib, train_decoder as TD, train_dropout as TDrop, train_head as TH

FIXTURE = os.path.join(GOLDEN, "head_many_ar_d64.npz")
V, H, W, D = 2, 32, 48, 64
FLAGS = (False, True)


@functools.lru_cache(maxsize=None)
def _case():
    """D 64, two views stored 32 x 48 of which the second is a portrait view: the mixed branch of wrapper_yes.  The fixture holds dW in fp64, 1792 x 64 x 8 bytes
    = 0.875 MiB of the 1 MiB a committed file may have; the pointmaps of two such views are what fits beside it."""
    return HAR.make_case(V, H, W, FLAGS, D=D, seed=11, g_scale=1.0)


@functools.lru_cache(maxsize=None)
def _mine():
    case = _case()
    return dict(out=HAR.forward(case, torch.float64), **HAR.grads(case, torch.float64))


def _reference(case):
    """Pointmaps and gradients of the reference's own wrapper over nn.LayerNorm + LinearHead (fp64, CPU) on the case"""
    from oracle import ref_shims
    ref_shims.install()
    from must3r.model.blocks.head import LinearHead, transpose_to_landscape
    Dm = case["D"]
    norm = torch.nn.LayerNorm(Dm, eps=1e-6).double()
    lin = LinearHead(Dm, HR.OUT, HR.PATCH).double()
    with torch.no_grad():
        norm.weight.copy_(case["gamma"])
        norm.bias.copy_(case["beta"])
        lin.proj.weight.copy_(case["W"])
        lin.proj.bias.copy_(case["b"])
    wrapper = transpose_to_landscape(lin, activate=True)
    x = case["x"].double().clone().requires_grad_(True)
    n = case["n_views"]
    out = wrapper([norm(x.view(n, -1, Dm))], HAR.true_shape(case["flags"], case["H"], case["Wd"]))
    out.backward(case["G"].double())
    return dict(out=out.detach(), dx=x.grad, dgamma=norm.weight.grad, dbeta=norm.bias.grad, dW=lin.proj.weight.grad, db=lin.proj.bias.grad)


def _keep_40_bits(a):
    """fp64 rounded to nearest at 40 of its 52 mantissa bits: a relative 2^-41 = 4.5e-13, far inside the rtol of 1e-10 the fixture is read with.  The zeroed
    bits are what lets the file fit: dW alone is 1792 x 64 doubles = 0.875 MiB, the pointmaps of the two views 0.16 MiB, and random mantissas do not compress."""
    bits = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    return ((bits + (1 << 11)) & ~np.int64((1 << 12) - 1)).view(np.float64)


def test_yardstick_matches_the_reference_wrapper():
    case, mine = _case(), _mine()
    assert set(mine) == {"out", *HAR.NAMES} and mine["out"].shape == (V, H, W, 7)
    sources = []
    if HAS_REFERENCE:
        ref = _reference(case)
        sources.append(ref)
        if os.environ.get("M3R_WRITE_HEAD_AR_GOLDEN"):
            np.savez_compressed(FIXTURE, **{k: _keep_40_bits(v.numpy()) for k, v in ref.items()})
    rec = np.load(FIXTURE)
    assert set(rec.files) == set(mine)
    sources.append({k: torch.from_numpy(rec[k]) for k in mine})
    for source in sources:
        for k, t in mine.items():
            r = source[k]
            assert r.dtype == torch.float64 and r.shape == t.shape and torch.isfinite(r).all(), k
            assert float(r.abs().max()) > 0, k
            assert torch.allclose(t, r, rtol=1e-10, atol=1e-12 * float(r.abs().max())), (k, float((t - r).abs().max()), float(r.abs().max()))


def test_fixture_is_a_committable_file():
    assert os.path.getsize(FIXTURE) <= 1 << 20


def test_portrait_view_is_the_landscape_run_on_the_swapped_geometry():
    case = HAR.make_case(3, 48, 80, (False, True, False), D=64, seed=2)
    t = {k: case[k].double() for k in ("x", "gamma", "beta", "W", "b")}
    out = HAR.forward(case, torch.float64)
    N = 15
    z = torch.nn.functional.linear(torch.nn.functional.layer_norm(t["x"], (64,), t["gamma"], t["beta"], 1e-6), t["W"], t["b"])
    # the header's formula, one tile at a time
    assert torch.equal(out, HAR.shuffle_loop(z, case["flags"], 48, 80))
    # the portrait view alone is the plain head on (W, H), swapped; the landscape views are the plain head
    alone = HR.head(t["x"][N:2 * N], t["gamma"], t["beta"], t["W"], t["b"], 1, 80, 48)
    assert alone.shape == (1, 80, 48, 7) and torch.equal(out[1], alone[0].swapaxes(0, 1))
    plain = HR.head(t["x"], t["gamma"], t["beta"], t["W"], t["b"], 3, 48, 80)
    assert torch.equal(out[0], plain[0]) and torch.equal(out[2], plain[2]) and not torch.equal(out[1], plain[1])
    # single elements: view 1 is portrait, its grid 5 rows of 3; token t = py 3 + px, pixel (i, j), channel c
    for tok, c, i, j in ((7, 1, 3, 9), (14, 6, 15, 15), (2, 0, 0, 5), (4, 3, 11, 0)):
        py, px = divmod(tok, 3)
        assert out[1, 16 * px + j, 16 * py + i, c] == z[N + tok, c * 256 + 16 * i + j]
    for v, tok, c, i, j in ((0, 7, 1, 3, 9), (2, 14, 2, 15, 0)):
        gy, gx = divmod(tok, 5)
        assert out[v, 16 * gy + i, 16 * gx + j, c] == z[v * N + tok, c * 256 + 16 * i + j]
    # with no view flagged the yardstick is tests/head_ref.py's
    none = HAR.make_case(3, 48, 80, (False,) * 3, D=64, seed=2)
    assert torch.equal(HAR.forward(none, torch.float64), plain)


# ---------------------------------------------------------------------------------------------------------------------------------
# head_turn_kernel replayed: the LDS map and the index arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
PITCH = 116
at = lambda i, e: PITCH * i + e                                              # element (row i, float e = 7 j + c) of the source tile
WRITE_GROUPS = [range(8 * g, 8 * g + 8) for g in range(8)]                   # ds_write_b128: 8 groups of 8 consecutive lanes
READ_GROUPS = [range(0, 32), range(32, 64)]                                  # ds_read_b32: the two halves of the wave


def _extra_cycles(addresses, groups):
    """addresses: per lane the dwords one instruction touches.  Bank = dword address mod 32; within a group every further distinct address on a bank costs
    one cycle, so a group costs (its busiest bank's distinct addresses - 1) extra."""
    extra = 0
    for g in groups:
        banks = {}
        for lane in g:
            for a in addresses[lane]:
                banks.setdefault(a % 32, set()).add(a)
        extra += max(len(s) for s in banks.values()) - 1
    return extra


def _tile_conflicts(addr):
    writes = reads = 0
    for n in range(7):
        lanes = [divmod(64 * n + l, 28) for l in range(64)]                  # (row, float4 of the row), source side and destination side alike
        writes += _extra_cycles([[addr(i, 4 * f + k) for k in range(4)] for i, f in lanes], WRITE_GROUPS)
        for k in range(4):
            reads += _extra_cycles([[addr((4 * f + k) // 7, 7 * j + (4 * f + k) % 7)] for j, f in lanes], READ_GROUPS)
    return writes, reads


def test_lds_map_of_the_turned_tile_is_injective_and_has_the_stated_conflicts():
    """The layout csrc/train_head.hip states for a tile, replayed by the rules for the widths it uses: A(i, e) = 116 i + e, 7 ds_write_b128 and 28 ds_read_b32 per
    tile; 8 extra cycles over the writes, 96 over the reads, and the counts stated for the pitches that were not taken."""
    cells = {at(i, e) for i in range(16) for e in range(112)}
    assert len(cells) == 1792 and max(cells) < 16 * PITCH and PITCH % 4 == 0
    assert _tile_conflicts(at) == (8, 96)
    assert _tile_conflicts(lambda i, e: 112 * i + e) == (0, 144)
    assert _tile_conflicts(lambda i, e: 124 * i + e) == (8, 120)
    assert _tile_conflicts(lambda i, e: 128 * i + e) == (8, 144)
    # every element that is read was written, once: the reads of a tile cover the 1792 cells exactly
    read = [at((4 * f + k) // 7, 7 * j + (4 * f + k) % 7) for q in range(448) for j, f in [divmod(q, 28)] for k in range(4)]
    assert sorted(read) == sorted(cells)


def _turn(src, flags, Hh, Ww, to_slots):
    """head_turn_kernel in numpy, index for index: flat fp32 [V, H, W, 7] -> the flagged views' tiles moved (the other views are not written)"""
    gh, gw, ntok, row = Hh // 16, Ww // 16, (Hh // 16) * (Ww // 16), Ww * 7
    dst = np.full_like(src, np.nan)
    for v, f in enumerate(flags):
        if not f:
            continue
        for t in range(ntok):
            ly, lx = divmod(t, gw)
            sx, sy = divmod(t, gh)
            at_l, at_s = ((v * Hh + 16 * ly) * Ww + 16 * lx) * 7, ((v * Hh + 16 * sy) * Ww + 16 * sx) * 7
            s0, d0 = (at_s, at_l) if to_slots else (at_l, at_s)
            lds = np.full(16 * PITCH, np.nan, dtype=src.dtype)
            for q in range(448):
                i, f4 = divmod(q, 28)
                lds[PITCH * i + 4 * f4:PITCH * i + 4 * f4 + 4] = src[s0 + i * row + 4 * f4:s0 + i * row + 4 * f4 + 4]
            for q in range(448):
                j, f4 = divmod(q, 28)
                for k in range(4):
                    e = 4 * f4 + k
                    dst[d0 + j * row + e] = lds[PITCH * (e // 7) + 7 * j + e % 7]
    return dst


def test_turn_kernel_arithmetic_moves_the_tiles_of_flagged_views():
    """Forward: the head's output with the landscape geometry -> the stored layout of the portrait view.  Backward: the stored upstream gradient -> the tiles in the
    slot order of the tokens, from which the gather of must3r_hip_head_grad reads the rows of dZ.  Both are permutations, and inverses of each other."""
    flags, Hh, Ww = (False, True), 32, 48
    N = 6
    z = torch.arange(2 * N * HR.OUT, dtype=torch.float32).view(2 * N, HR.OUT)
    landscape_run = HR.pixel_shuffle_loop(z, 2, Hh, Ww)                               # what one launch over all rows writes
    want = HAR.shuffle_loop(z, flags, Hh, Ww)
    got = _turn(landscape_run.numpy().reshape(-1), flags, Hh, Ww, 0).reshape(2, Hh, Ww, 7)
    assert np.isnan(got[0]).all() and np.array_equal(got[1], want[1].numpy())
    back = _turn(want.numpy().reshape(-1), flags, Hh, Ww, 1).reshape(2, Hh, Ww, 7)
    assert np.isnan(back[0]).all() and np.array_equal(back[1], landscape_run[1].numpy())
    assert torch.equal(HR.unshuffle(torch.from_numpy(back[1:2].copy())), z[N:])       # the rows of dZ the gather then reads


# ---------------------------------------------------------------------------------------------------------------------------------
# the ABI surface
# ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        return f.read()


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *more = [n.strip() for n in decl.replace("*", "* ").split(",")]
        ctype, n0 = first.rsplit(None, 1)
        size = 8 if "*" in ctype else {"int32_t": 4, "float": 4, "must3r_hip_head_grad_args": C.sizeof(_lib.HeadGradArgs)}[ctype]
        fields += [(n, size) for n in (n0, *more)]
    return fields


def _check_layout(cls, fields):
    at_ = 0
    for n, size in fields:
        align = min(size, 8)
        at_ = (at_ + align - 1) // align * align
        assert getattr(cls, n).offset == at_ and getattr(cls, n).size == size, n
        at_ += size
    return at_


def test_abi_surface_of_the_many_ar_entry_points():
    lib = _lib.load()
    i32, sz, vp = C.c_int, C.c_size_t, C.c_void_p
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION == 21 and "#define MUST3R_HIP_ABI_VERSION 21" in _header()
    protos = {"must3r_hip_head_forward_many_ar_scratch_bytes": (sz, [i32] * 4),
              "must3r_hip_head_forward_many_ar": (i32, [C.POINTER(_lib.HeadForwardArArgs), vp, sz]),
              "must3r_hip_head_grad_many_ar_scratch_bytes": (sz, [i32] * 4),
              "must3r_hip_head_grad_many_ar": (i32, [C.POINTER(_lib.HeadGradArArgs), vp, sz])}
    for name, proto in protos.items():
        assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == proto, name
        fn = getattr(lib, name)
        assert fn.argtypes == proto[1] and fn.restype == proto[0], name
    fwd = _struct_fields("must3r_hip_head_forward_ar_args")
    assert [n for n, _ in fwd] == ["x", "gamma", "beta", "W", "b", "dtype", "n_views", "H", "Wimg", "D", "eps", "pointmaps", "transposed", "stream"]
    assert [f[0] for f in _lib.HeadForwardArArgs._fields_] == [n for n, _ in fwd]
    assert _check_layout(_lib.HeadForwardArArgs, fwd) == C.sizeof(_lib.HeadForwardArArgs) == 5 * 8 + 6 * 4 + 3 * 8
    grad = _struct_fields("must3r_hip_head_grad_ar_args")
    assert [n for n, _ in grad] == ["g", "transposed", "stream"] == [f[0] for f in _lib.HeadGradArArgs._fields_]
    assert _check_layout(_lib.HeadGradArArgs, grad) == C.sizeof(_lib.HeadGradArArgs) == C.sizeof(_lib.HeadGradArgs) + 16
    # the embedded descriptor is the ABI 19 one, untouched
    assert _lib.HeadGradArArgs.g.offset == 0 and dict(_lib.HeadGradArArgs._fields_)["g"] is _lib.HeadGradArgs
    assert C.sizeof(_lib.HeadGradArgs) == 5 * 8 + 6 * 4 + 5 * 8
    h = _header()
    assert re.search(r"\bint\s+must3r_hip_head_forward_many_ar\s*\(\s*const\s+must3r_hip_head_forward_ar_args\s*\*\s*a\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*\)\s*;", h)
    assert re.search(r"\bint\s+must3r_hip_head_grad_many_ar\s*\(\s*const\s+must3r_hip_head_grad_ar_args\s*\*\s*a\s*,\s*void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes\s*\)\s*;", h)
    for name in ("must3r_hip_head_forward_many_ar_scratch_bytes", "must3r_hip_head_grad_many_ar_scratch_bytes"):
        assert re.search(r"\bsize_t\s+%s\s*\(\s*int\s+n_views\s*,\s*int\s+H\s*,\s*int\s+Wimg\s*,\s*int\s+D\s*\)\s*;" % name, h)


def test_the_stream_travels_in_the_descriptors():
    """tests/stream_forms.py lists the entry points with a trailing ``void* stream``; the two new ones are not among them"""
    from test_stream_order_host import stream_entry_points
    names = stream_entry_points()
    assert "must3r_hip_head_forward_many_ar" not in names and "must3r_hip_head_grad_many_ar" not in names


def test_scratch_queries_answer_without_a_device():
    lib = _lib.load()
    up = lambda n: (n + 255) // 256 * 256
    for shape in ((1, 32, 48, 64), (3, 48, 80, 64), (3, 176, 208, 128), (20, 384, 512, 768)):
        n, Hh, Ww, _ = shape
        extra = up(n * Hh * Ww * 7 * 4)
        assert lib.must3r_hip_head_forward_many_ar_scratch_bytes(*shape) == lib.must3r_hip_head_forward_scratch_bytes(*shape) + extra
        assert lib.must3r_hip_head_grad_many_ar_scratch_bytes(*shape) == lib.must3r_hip_head_grad_scratch_bytes(*shape) + extra
    for bad in ((1, 40, 48, 768), (1, 32, 50, 768), (1, 32, 48, 96), (0, 32, 48, 768)):
        assert lib.must3r_hip_head_forward_many_ar_scratch_bytes(*bad) == 0, bad
        assert lib.must3r_hip_head_grad_many_ar_scratch_bytes(*bad) == 0, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _forward_call(nbytes=1 << 30, **over):
    """A descriptor of fake but aligned addresses: every refusal comes before anything is read or launched"""
    lib = _lib.load()
    a = _lib.HeadForwardArArgs()
    a.x, a.gamma, a.beta, a.W, a.b, a.pointmaps, a.transposed = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
    a.dtype, a.n_views, a.H, a.Wimg, a.D, a.eps = _lib.F16, 3, 48, 80, 64, 1e-6
    for k, v in over.items():
        setattr(a, k, v)
    rc = lib.must3r_hip_head_forward_many_ar(C.byref(a), C.c_void_p(0x800000), nbytes)
    return rc, lib.must3r_hip_last_error().decode()


def _grad_call(nbytes=1 << 30, transposed=0x700000, **over):
    lib = _lib.load()
    a = _lib.HeadGradArArgs()
    a.g.x, a.g.gamma, a.g.beta, a.g.W, a.g.G, a.g.dx = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    a.g.n_views, a.g.H, a.g.Wimg, a.g.D, a.g.eps = 3, 48, 80, 64, 1e-6
    a.transposed = transposed
    for k, v in over.items():
        setattr(a.g, k, v)
    rc = lib.must3r_hip_head_grad_many_ar(C.byref(a), C.c_void_p(0x800000), nbytes)
    return rc, lib.must3r_hip_last_error().decode()


def test_entry_points_refuse_before_touching_anything():
    lib = _lib.load()
    assert lib.must3r_hip_head_forward_many_ar(None, None, 0) != 0 and "null" in lib.must3r_hip_last_error().decode()
    assert lib.must3r_hip_head_grad_many_ar(None, None, 0) != 0 and "null" in lib.must3r_hip_last_error().decode()
    small = lib.must3r_hip_head_forward_many_ar_scratch_bytes(3, 48, 80, 64) - 1
    for over, word in ((dict(x=None), "null"), (dict(H=40), "multiples of 16"), (dict(Wimg=88), "multiples of 16"), (dict(D=96), "multiple of 64"),
                       (dict(n_views=0), "positive"), (dict(H=80, Wimg=48), "stored landscape"), (dict(transposed=0x700002), "4-byte"),
                       (dict(nbytes=small), "scratch"), (dict(dtype=7), "dtype"), (dict(W=None), "null"), (dict(pointmaps=0x600008), "aligned")):
        rc, msg = _forward_call(**over)
        assert rc != 0 and word in msg, (over, msg)
    small = lib.must3r_hip_head_grad_many_ar_scratch_bytes(3, 48, 80, 64) - 1
    for over, word in ((dict(G=None), "null"), (dict(x=None), "null"), (dict(H=40), "multiples of 16"), (dict(D=96), "multiple of 64"),
                       (dict(H=80, Wimg=48), "stored landscape"), (dict(transposed=0x700002), "4-byte"), (dict(nbytes=small), "scratch"),
                       (dict(dx=0x600004), "aligned")):
        rc, msg = _grad_call(**over)
        assert rc != 0 and word in msg, (over, msg)
    # without flags a portrait-shaped batch is the plain entry point's business: the shape is not refused (the scratch is)
    rc, msg = _grad_call(transposed=None, H=80, Wimg=48, nbytes=16)
    assert rc != 0 and "scratch" in msg


def _params(Dm=64):
    return torch.ones(Dm), torch.zeros(Dm), torch.zeros(HR.OUT, Dm), torch.zeros(HR.OUT)


def test_python_refusals():
    tok = torch.zeros(2, 6, 64)
    flags = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        TH.prediction_head(tok, (32, 48), *_params(), transposed=flags)
    assert list(inspect.signature(TH.prediction_head).parameters)[-1] == "transposed"
    assert inspect.signature(TH.prediction_head).parameters["transposed"].default is None
    with pytest.raises(RuntimeError, match="GPU"):
        TH._check_transposed(flags, 2, 32, 48, "prediction_head")
    head = TH.PredictionHead(64, landscape_only=True)
    assert head.landscape_only is True and TH.PredictionHead(64).landscape_only is False
    # without img_shape the rows are checked on the host: one stored size, each row (H, W) or (W, H)
    with pytest.raises(ValueError, match="one stored size"):
        head(tok, torch.tensor([[32, 48], [48, 48]]))
    with pytest.raises(ValueError, match="one stored size"):
        head(tok, torch.tensor([[32, 48], [32, 32]]))
    # a stored size that is not landscape
    with pytest.raises(ValueError, match="stored landscape"):
        head(tok, torch.tensor([[32, 48], [48, 32]]), img_shape=(48, 32))
    # valid mixed rows get as far as the device check, with and without img_shape
    with pytest.raises(RuntimeError, match="GPU"):
        head(tok, torch.tensor([[32, 48], [48, 32]]))
    with pytest.raises(RuntimeError, match="GPU"):
        head(tok, torch.tensor([[32, 48], [48, 32]]), img_shape=(32, 48))
    # the token count is held against the stored size
    with pytest.raises(ValueError, match="do not match"):
        head(torch.zeros(2, 5, 64), torch.tensor([[32, 48], [48, 32]]), img_shape=(32, 48))


def test_default_head_still_refuses_a_mixed_true_shape():
    tok = torch.zeros(2, 6, 64)
    head = TH.PredictionHead(64)
    with pytest.raises(ValueError, match="share"):
        head(tok, torch.tensor([[32, 48], [48, 32]]))
    with pytest.raises(ValueError, match="share"):
        head(tok, torch.tensor([[32, 48], [48, 32]]), img_shape=(32, 48))
    with pytest.raises(RuntimeError, match="GPU"):
        head(tok, torch.tensor([[32, 48], [32, 48]]))


def test_decoders_take_landscape_only_and_img_shape():
    kw = dict(enc_embed_dim=64, embed_dim=64, depth=2, num_heads=1)
    for cls in (TD.MUSt3R, TD.CausalMUSt3R, TDrop.CausalMUSt3R):
        assert cls(**kw).landscape_only is False and cls(landscape_only=True, **kw).landscape_only is True
        assert inspect.signature(cls.forward).parameters["img_shape"].default is None
        with pytest.raises(TypeError, match="list inputs"):
            cls(landscape_only=True, **kw)([torch.zeros(1, 1, 6, 64)], [torch.zeros(6, 2)], None)

    # from_decoder does not pick the value up from the source's attribute (the native decoder's defaults to True)
    src = TD.MUSt3R(**kw)
    src.landscape_only = True
    assert TD.MUSt3R.from_decoder(src).landscape_only is False
    assert TD.MUSt3R.from_decoder(src, landscape_only=True).landscape_only is True
    assert TDrop.CausalMUSt3R.from_decoder(src, landscape_only=True).landscape_only is True
    assert list(TD.MUSt3R(landscape_only=True, **kw).state_dict()) == list(src.state_dict())


def test_driver_hands_the_stored_size_to_a_landscape_only_decoder():
    """``train_encoder.inference`` on stub modules: a decoder built with landscape_only=True receives img_shape = imgs.shape[-2:] in every call, any other
    decoder is called as before"""
    from must3r_amd import train_encoder as TE
    seen = []

    class Enc(torch.nn.Module):
        def forward(self, img, true_shape):
            return torch.zeros(img.shape[0], 15, 8), torch.zeros(img.shape[0], 15, 2, dtype=torch.int64)

    class Dec(TH.PredictionHead):
        def forward(self, x, pos, true_shape, mem=None, render=False, **kw):
            seen.append((render, kw))
            return (([x], None, 0, 0, 0), torch.zeros(x.shape[0], x.shape[1], 48, 80, 7))

    imgs = torch.zeros(1, 3, 3, 48, 80)
    ts = torch.tensor([[[48, 80], [80, 48], [48, 80]]])
    TE.inference(Enc(), Dec(64, landscape_only=True), imgs, ts, [2, 1])
    assert seen == [(False, dict(img_shape=(48, 80))), (False, dict(img_shape=(48, 80))), (True, dict(img_shape=(48, 80)))]
    seen.clear()
    TE.inference(Enc(), Dec(64), imgs, ts, [2, 1])
    assert seen == [(False, {}), (False, {}), (True, {})]
