"""CPU: the host side of the decoder block's training path -- the yardstick tests/decblock_ref.py against the reference's own CachedDecoderBlock class in its
three memory modes (live where the reference tree exists, from the recorded fixture tests/golden/decblock_ref_d64.npz elsewhere), the additive ABI 21 surface
of csrc/train_cross.hip, its scratch query and its refusals (no compute calls: no GPU here).

The yardstick's tolerance is that of tests/test_block_grad_host.py (rtol 1e-10, atol 1e-12 max|r|) for every tensor but one: the gradient of
cross_attn.projk.bias is exactly zero in the update form (every key of a view carries the bias, and a common shift of the keys does not move a softmax), so
max|r| is rounding noise of two different summation orders (measured 7.9e-22 against 7.6e-22 between the two sides).  For that tensor the magnitude is that of
what cancels, max_c sum_r |dK_rc| of the fp64 yardstick, and the reference's value itself must lie below 1e-12 of it."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import decblock_ref as DR
from conftest import GOLDEN, HAS_REFERENCE, ROOT
from must3r_amd import _lib, train_cross as TC

FIXTURE = os.path.join(GOLDEN, "decblock_ref_d64.npz")
NEW = ("must3r_hip_cross_sublayer_scratch_bytes", "must3r_hip_cross_sublayer_forward", "must3r_hip_cross_sublayer_grad")
NM, N_TOK, VIEWS = 24, 35, 2


def _tiny(mode):
    """D 64, 1 head, hidden 256: one scene of 2 views of a 5 x 7 grid over 24 memory rows, a view does not attend its own tokens."""
    return DR.make_block_case(64, 1, 256, 1, VIEWS, N_TOK, NM, 61, mode=mode, width=7)


def _reference_block(case):
    """Output and gradients of the reference's own CachedDecoderBlock (fp64, CPU): the views are its batch entries, and each view is handed the key rows it may
    see -- the memory followed by the other view's prepare_y rows -- gathered with a boolean mask as MUSt3R.forward does.  The memory and the block input are
    leaves: autograd sums over the views."""
    from oracle import ref_shims
    ref_shims.install()
    from must3r.model.blocks.layers import CachedDecoderBlock
    from croco.models.pos_embed import RoPE2D
    D, n, V, Nm = case["D"], case["n"], case["V"], case["Nm"]
    blk = CachedDecoderBlock(D, case["heads"], pos_embed=RoPE2D(*case["rope"]), mlp_ratio=case["hidden"] / D, qkv_bias=True,
                             norm_layer=functools.partial(torch.nn.LayerNorm, eps=case["eps"]), memory_mode=case["mode"]).double()
    blk.load_state_dict({k: v.double() for k, v in case["params"].items()}, strict=True)
    x = case["x"].double().view(V, n, D).clone().requires_grad_(True)
    mem = case["mem"].double().clone().requires_grad_(True)
    W = mem.shape[1]
    rows = torch.cat([mem, blk.prepare_y(x).reshape(V * n, W)])
    mask = torch.ones((V, Nm + V * n), dtype=torch.bool)
    for j in range(V):
        mask[j, Nm + j * n:Nm + (j + 1) * n] = False
    y = rows.unsqueeze(0).expand(V, -1, -1)[mask].reshape(V, Nm + (V - 1) * n, W)
    out = blk(x, y, case["pos"].view(V, n, 2))
    out.backward(case["dy"].double().view(V, n, D))
    res = dict(out=out.detach().reshape(-1, D), dx=x.grad.reshape(-1, D), dmem=mem.grad)
    res.update({k: t.grad for k, t in blk.named_parameters()})
    return res


def _checked(mode):
    """norm_y: every gradient; raw and kv: the output and the two data gradients"""
    return ("out", "dx", "dmem") + (DR.PARAMS if mode == "norm_y" else ())


def test_yardstick_matches_the_reference_decoder_block():
    cases = {mode: _tiny(mode) for mode in DR.MODES}
    extra = {mode: {} for mode in DR.MODES}
    mine = {mode: DR.grads(c, torch.float64, "block", extra[mode]) for mode, c in cases.items()}
    assert set(mine["norm_y"]) == {"out", "dx", "dmem", *DR.PARAMS}
    ref = None
    if HAS_REFERENCE:
        ref = {mode: _reference_block(c) for mode, c in cases.items()}
        if os.environ.get("M3R_WRITE_DECBLOCK_GOLDEN"):
            np.savez_compressed(FIXTURE, x=cases["norm_y"]["x"].numpy(), mem_kv=cases["kv"]["mem"].numpy(),
                                **{f"{mode}__{k}": ref[mode][k].numpy() for mode in DR.MODES for k in _checked(mode)})
    rec = np.load(FIXTURE)
    for mode, c in cases.items():
        assert np.array_equal(rec["x"], c["x"].numpy()), "the seeded case is not the one the fixture was recorded on"
    assert np.array_equal(rec["mem_kv"], cases["kv"]["mem"].numpy())
    sources = ([ref] if ref is not None else []) + [{mode: {k: torch.from_numpy(rec[f"{mode}__{k}"]) for k in _checked(mode)} for mode in DR.MODES}]
    for source in sources:
        for mode in DR.MODES:
            for k in _checked(mode):
                t, r = mine[mode][k], source[mode][k]
                assert r.dtype == torch.float64 and torch.isfinite(r).all(), (mode, k)
                assert float(r.abs().max()) > 0, (mode, k)
                m = float(r.abs().max())
                if k == "cross_attn.projk.bias":
                    # a shift common to every key a view sees does not move its softmax: the true gradient is zero and both sides hold fp64 rounding
                    # noise (7e-22 here).  The magnitude of what cancels in it is the largest column 1-norm of dK, as in tests/test_cross_grad_gpu.py
                    m = extra[mode]["dK_colsum"]
                    assert float(r.abs().max()) < 1e-12 * m
                assert torch.allclose(t, r, rtol=1e-10, atol=1e-12 * m), (mode, k, float((t - r).abs().max()), m)


def test_sublayers_compose_and_modes_agree():
    """The three memory modes are one function of the tokens: the block's output in the update form does not depend on what the memory stores, given a memory
    that holds prepare_y of the same earlier tokens."""
    case = _tiny("raw")
    p = {k: v.double() for k, v in case["params"].items()}
    x, earlier = case["x"].double(), case["mem"].double()
    outs = {}
    for mode in DR.MODES:
        c = dict(case, mode=mode)
        outs[mode] = DR.block_forward(c, x, DR.prepare_y(earlier, p, mode), p)
    assert torch.allclose(outs["raw"], outs["norm_y"], rtol=0, atol=1e-12) and torch.allclose(outs["raw"], outs["kv"], rtol=0, atol=1e-12)
    # a row of no view: out = x + proj.bias
    got = DR.cross_sublayer(x, earlier, [[0, 30, 0, 24, 0, 0]], 1, p)
    assert torch.equal(got[30:], x[30:] + p["cross_attn.proj.bias"])


def test_additive_abi_21_symbols_signatures_and_descriptor():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION == 21
    for name in NEW:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == _lib.PROTOTYPES[name][0], name
    assert _lib.PROTOTYPES[NEW[0]] == (C.c_size_t, [C.c_int] * 5)
    for name in NEW[1:]:
        assert _lib.PROTOTYPES[name] == (C.c_int, [C.POINTER(_lib.CrossSublayerArgs), C.c_void_p, C.c_size_t])
    A = _lib.CrossSublayerArgs
    assert C.sizeof(A) == 27 * 8 + 8 * 4 + 8
    assert A.x.offset == 0 and A.mem.offset == 8 and A.dy.offset == 96 and A.views.offset == 104 and A.out.offset == 112 and A.dx.offset == 120
    assert A.dmem.offset == 128 and A.dbproj.offset == 208 and A.M.offset == 216 and A.Rm.offset == 220 and A.ldmem.offset == 232 and A.lddmem.offset == 236
    assert A.eps.offset == 240 and A.stream.offset == 248
    assert [f[0] for f in A._fields_[15:27]] == list(TC.CROSS_OUTPUTS)
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        header = f.read()
    assert "#define MUST3R_HIP_ABI_VERSION 21" in header and "ABI 21, additive" in header
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        decl = re.findall(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;{}]*)\)\s*;", plain)
        assert len(decl) == 1, name
        assert not re.search(r"void\*\s*stream\s*$", decl[0]), f"{name}: the stream travels in the descriptor"
    assert re.search(r"void\*\s*stream;", plain[plain.index("typedef struct must3r_hip_cross_sublayer_args"):plain.index("} must3r_hip_cross_sublayer_args;")])
    # the descriptor of the header, field by field
    body = plain[plain.index("typedef struct must3r_hip_cross_sublayer_args {"):plain.index("} must3r_hip_cross_sublayer_args;")].split("{", 1)[1]
    names = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            names += [n.strip().lstrip("*").strip() for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", stmt, count=1).split(",")]
    assert names == [f[0] for f in A._fields_], names


def test_scratch_query_matches_the_documented_sum():
    lib = _lib.load()
    cross = lib.must3r_hip_cross_sublayer_scratch_bytes
    wg, ln, core = lib.must3r_hip_op_linear_wgrad_scratch_bytes, lib.must3r_hip_op_layernorm_grad_scratch_bytes, lib.must3r_hip_attn_train_scratch_bytes
    up = lambda v: (v + 255) // 256 * 256
    for M, Rm, D in ((140, 280, 128), (192, 288, 768), (15360, 30720, 768)):
        n = 4
        tail = up(ln(M, D)) + up(core(n, M, Rm, D // 64))
        assert cross(M, Rm, D, n, 0) == 5 * up(4 * M * D) + 2 * up(8 * Rm * D) + up(max(wg(M, D, D), wg(Rm, D, D))) + tail, (M, Rm, D)
        assert cross(M, Rm, D, n, 1) == 5 * up(4 * M * D) + up(wg(M, D, D)) + tail, (M, Rm, D)
        assert cross(M, Rm, D, n, 7) == cross(M, Rm, D, n, 1)
    for bad in ((0, 10, 128, 1), (-3, 10, 128, 1), (10, 0, 128, 1), (10, -1, 128, 1), (10, 10, 96, 1), (10, 10, 0, 1), (10, 10, 1088, 1), (10, 10, 128, 0),
                (10, 10, 128, 70000)):
        assert cross(*bad, 0) == 0 and cross(*bad, 1) == 0, bad


FIELDS = ("x", "mem", "gamma", "beta", "Wq", "bq", "Wk", "bk", "Wv", "bv", "Wproj", "bproj", "dy", "out") + TC.CROSS_OUTPUTS


def _call(fn, views=((0, 6, 0, 12, 0, 0), (6, 4, 12, 8, 2, 5)), nbytes=0, scratch=None, kv=False, **over):
    """A descriptor of fake but aligned addresses: every refusal comes before anything is read or launched."""
    lib = _lib.load()
    t = torch.tensor([list(v) for v in views], dtype=torch.int32).contiguous()
    a = _lib.CrossSublayerArgs()
    for i, n in enumerate(FIELDS):
        setattr(a, n, C.c_void_p(0x100000 * (i + 1)))
    if kv:
        for n in ("Wk", "bk", "Wv", "bv", "dWk", "dbk", "dWv", "dbv"):
            setattr(a, n, None)
    a.views, a.M, a.Rm, a.D, a.n_views, a.eps = C.c_void_p(t.data_ptr()), 10, 20, 128, len(views), 1e-6
    a.ldmem = a.lddmem = 256 if kv else 128
    a.stream = None
    for k, v in over.items():
        setattr(a, "views" if k == "table" else k, v)
    rc = getattr(lib, fn)(C.byref(a), scratch, nbytes)
    return rc, lib.must3r_hip_last_error().decode()


@pytest.mark.parametrize("kv", [False, True], ids=["tokens", "kv"])
@pytest.mark.parametrize("fn", NEW[1:])
def test_cross_sublayer_refuses_before_touching_anything(fn, kv):
    lib = _lib.load()
    grad = fn.endswith("_grad")
    assert getattr(lib, fn)(None, None, 0) != 0 and "null" in lib.must3r_hip_last_error().decode()
    refusals = [(dict(D=96), "multiple of 64"), (dict(D=0), "multiple of 64"), (dict(D=2048), "1024"), (dict(M=0), "M must"), (dict(M=-1), "M must"),
                (dict(Rm=0), "Rm must"), (dict(Rm=-5), "Rm must"),
                (dict(x=None), "null"), (dict(mem=None), "null"), (dict(gamma=None), "null"), (dict(beta=None), "null"), (dict(Wq=None), "null"),
                (dict(Wproj=None), "null"), (dict(table=None), "views"), (dict(n_views=0), "n_views"), (dict(dy=None) if grad else dict(out=None), "null"),
                (dict(ldmem=(256 if kv else 128) - 4), "leading dimension"), (dict(ldmem=(256 if kv else 128) + 2), "leading dimension"),
                (dict(lddmem=(256 if kv else 128) - 4), "leading dimension"), (dict(lddmem=(256 if kv else 128) + 6), "leading dimension"),
                (dict(x=C.c_void_p(0x100008)), "aligned"), (dict(mem=C.c_void_p(0x200004)), "aligned"), (dict(Wq=C.c_void_p(0x500008)), "aligned"),
                (dict(bproj=C.c_void_p(0xc00004)), "aligned"), (dict(dmem=C.c_void_p(0x1000008)), "aligned"), (dict(dbq=C.c_void_p(0x1400004)), "aligned")]
    if kv:
        refusals += [(dict(Wk=C.c_void_p(0x700000)), "Wk and Wv"), (dict(Wv=C.c_void_p(0x900000)), "Wk and Wv"), (dict(bk=C.c_void_p(0x800000)), "need Wk"),
                     (dict(dWv=C.c_void_p(0x1700000)), "need Wk"), (dict(ldmem=128), "leading dimension")]
    else:
        refusals += [(dict(Wk=None), "Wk and Wv"), (dict(Wv=None), "Wk and Wv"), (dict(Wk=C.c_void_p(0x700004)), "aligned")]
    for over, word in refusals:
        rc, msg = _call(fn, kv=kv, **over)
        assert rc != 0 and word in msg, (over, msg)
    for views, word in ((((0, 6, 0, 12, 0, 0), (6, 5, 12, 8, 0, 0)), "past the M query rows"), (((0, 6, 0, 21, 0, 0),), "past the Rm key rows"),
                        (((0, 6, 13, 8, 0, 0),), "past the Rm key rows"), (((0, -6, 0, 6, 0, 0),), "negative"), (((0, 6, 0, 6, -1, 0),), "negative"),
                        (((0, 6, 0, 12, 5, 4),), "skip"), (((0, 6, 0, 12, 3, 13),), "skip")):
        rc, msg = _call(fn, views=views, kv=kv)
        assert rc != 0 and word in msg, (views, msg)
    # everything else in order: the scratch is what is missing
    rc, msg = _call(fn, kv=kv)
    assert rc != 0 and "scratch" in msg, msg
    need = lib.must3r_hip_cross_sublayer_scratch_bytes(10, 20, 128, 2, 1 if kv else 0)
    assert need > 0
    for scratch, nbytes in ((C.c_void_p(0x9000000), need - 1), (C.c_void_p(0x9000008), need), (None, need)):
        rc, msg = _call(fn, scratch=scratch, nbytes=nbytes, kv=kv)
        assert rc != 0 and "scratch" in msg, msg


def test_overlapping_key_groups_are_refused_by_the_backward():
    views = ((0, 6, 0, 12, 0, 0), (6, 4, 6, 12, 0, 0))
    rc, msg = _call("must3r_hip_cross_sublayer_grad", views=views)
    assert rc != 0 and "overlapping" in msg, msg
    rc, msg = _call("must3r_hip_cross_sublayer_forward", views=views)          # the forward alone sums nothing over views
    assert rc != 0 and "scratch" in msg, msg
    # views that share kv_row0 are one group: causal prefixes
    rc, msg = _call("must3r_hip_cross_sublayer_grad", views=((0, 6, 0, 12, 0, 0), (6, 4, 0, 20, 0, 0)))
    assert rc != 0 and "scratch" in msg, msg


def test_python_refusals_and_memory_rows():
    x, mem = torch.zeros(6, 128), torch.zeros(9, 128)
    w = lambda *s: torch.zeros(s)
    params = (w(128), w(128), w(128, 128), w(128), w(128, 128), w(128), w(128, 128), w(128), w(128, 128), w(128))
    with pytest.raises(RuntimeError, match="GPU"):
        TC.cross_attention_sublayer(x, mem, [[0, 6, 0, 9, 0, 0]], 2, *params)
    with pytest.raises(ValueError, match="memory_mode"):
        TC.CachedDecoderBlock(128, 2, memory_mode="keys")
    with pytest.raises(ValueError, match="num_heads"):
        TC.CachedDecoderBlock(128, 3)
    # memory_rows: per scene [Nm | V n], under autograd
    cur = torch.arange(2 * 3 * 4, dtype=torch.float32).view(6, 4).requires_grad_(True)
    new = (100 + torch.arange(2 * 2 * 4, dtype=torch.float32)).view(4, 4).requires_grad_(True)
    y = TC.memory_rows(cur, new, 2)
    assert y.shape == (10, 4) and torch.equal(y, DR.memory_rows(cur, new, 2))
    assert torch.equal(y[:3], cur[:3]) and torch.equal(y[3:5], new[:2]) and torch.equal(y[5:8], cur[3:]) and torch.equal(y[8:], new[2:])
    (y * torch.arange(10.0)[:, None]).sum().backward()
    assert torch.equal(cur.grad[:, 0], torch.tensor([0.0, 1, 2, 5, 6, 7])) and torch.equal(new.grad[:, 0], torch.tensor([3.0, 4, 8, 9]))
    assert torch.equal(TC.memory_rows(None, new, 2), new) and torch.equal(TC.memory_rows(cur[:0], new, 2), new)
    assert torch.equal(TC.memory_rows(cur.view(2, 3, 4), new.view(2, 2, 4), 2), y)
    with pytest.raises(ValueError, match="scenes"):
        TC.memory_rows(cur, new, 3)


def test_block_keeps_the_reference_state_dict_keys_and_copies():
    from must3r_amd.model.blocks import DecBlockParams
    src = DecBlockParams(128, 4.0, "kv").half()
    blk = TC.CachedDecoderBlock.from_params(src)
    assert blk.memory_mode == "kv" and TC.CachedDecoderBlock.from_params(src, memory_mode="raw").memory_mode == "raw"
    assert list(blk.state_dict()) == list(src.state_dict()) and set(blk.state_dict()) == set(DR.PARAMS)
    assert all(v.dtype == torch.float32 for v in blk.state_dict().values()) and all(v.dtype == torch.float16 for v in src.state_dict().values())
    assert blk.num_heads == 2 and blk.mlp.fc1.weight.shape == (512, 128) and blk.eps == 1e-6
    assert torch.equal(blk.cross_attn.projk.weight, src.cross_attn.projk.weight.float())
    assert blk.cross_attn.projk.weight.data_ptr() != src.cross_attn.projk.weight.data_ptr()
