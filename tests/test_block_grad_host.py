"""CPU: the host side of the block training path -- the yardstick tests/block_ref.py against the reference's own Block class (live where the reference
tree exists, from the recorded fixture tests/golden/block_ref_d64.npz elsewhere), the ABI 21 surface, the scratch queries and the refusals of the
operator forms and the sublayer entry points (no compute calls: no GPU here)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import block_ref as BR
from conftest import GOLDEN, HAS_REFERENCE
from must3r_amd import _lib, train_block as TB

FIXTURE = os.path.join(GOLDEN, "block_ref_d64.npz")
NEW = ("must3r_hip_op_linear_f32", "must3r_hip_op_layernorm_f32", "must3r_hip_op_gelu_f32", "must3r_hip_op_gelu_grad_f32", "must3r_hip_op_rope_f32",
       "must3r_hip_op_layernorm_grad_add", "must3r_hip_mlp_sublayer_scratch_bytes", "must3r_hip_mlp_sublayer_forward", "must3r_hip_mlp_sublayer_grad",
       "must3r_hip_attn_sublayer_scratch_bytes", "must3r_hip_attn_sublayer_forward", "must3r_hip_attn_sublayer_grad")


def _tiny():
    """D 64, 1 head, hidden 256, 2 views of a 5 x 7 grid."""
    return BR.make_case(64, 1, 256, [35, 35], 31, width=7)


def _reference_block(case):
    """Output and gradients of the reference's own Block (fp64, CPU) on the case: the views are its batch entries."""
    from oracle import ref_shims
    ref_shims.install()
    from must3r.model.blocks.layers import Block
    from croco.models.pos_embed import RoPE2D
    D, n = case["D"], case["tokens"][0]
    blk = Block(D, case["heads"], pos_embed=RoPE2D(*case["rope"]), mlp_ratio=case["hidden"] / D, qkv_bias=True,
                norm_layer=functools.partial(torch.nn.LayerNorm, eps=case["eps"])).double()
    blk.load_state_dict({k: v.double() for k, v in case["params"].items()}, strict=True)
    x = case["x"].double().view(-1, n, D).clone().requires_grad_(True)
    out = blk(x, case["pos"].view(-1, n, 2))
    out.backward(case["dy"].double().view(-1, n, D))
    res = dict(out=out.detach().reshape(-1, D), dx=x.grad.reshape(-1, D))
    res.update({k: t.grad for k, t in blk.named_parameters()})
    return res


def test_yardstick_matches_the_reference_block():
    case = _tiny()
    mine = BR.grads(case, torch.float64, "block")
    assert set(mine) == {"out", "dx", *BR.PARAMS}
    if HAS_REFERENCE:
        ref = _reference_block(case)
        if os.environ.get("M3R_WRITE_BLOCK_GOLDEN"):
            np.savez_compressed(FIXTURE, x=case["x"].numpy(), **{k: v.numpy() for k, v in ref.items()})
    else:
        ref = None
    rec = np.load(FIXTURE)
    assert np.array_equal(rec["x"], case["x"].numpy()), "the seeded case is not the one the fixture was recorded on"
    for source in ([ref] if ref is not None else []) + [{k: torch.from_numpy(rec[k]) for k in mine}]:
        for k, t in mine.items():
            r = source[k]
            assert r.dtype == torch.float64 and torch.isfinite(r).all(), k
            assert float(r.abs().max()) > 0, k
            assert torch.allclose(t, r, rtol=1e-10, atol=1e-12 * float(r.abs().max())), (k, float((t - r).abs().max()), float(r.abs().max()))


def test_rope_rows_is_the_oracle_rope2d():
    g = torch.Generator().manual_seed(5)
    t, pos = torch.randn((9, 128), generator=g, dtype=torch.float64), torch.randint(0, 30, (9, 2), generator=g)
    ref = BR.R.rope2d(t.view(1, 9, 2, 64).permute(0, 2, 1, 3), pos.view(1, 9, 2)).permute(0, 2, 1, 3).reshape(9, 128)
    assert torch.equal(BR.rope_rows(t, pos, 2, (100.0, 1.0)), ref)


def test_sublayers_compose_to_the_block():
    case = _tiny()
    p = {k: v.double() for k, v in case["params"].items()}
    x = case["x"].double()
    a = BR.attention_sublayer(x, case["pos"], case["views"], 1, p)
    assert torch.equal(BR.mlp_sublayer(a, p), BR.block(x, case["pos"], case["views"], 1, p))
    # a view's rows do not depend on the other view
    one = BR.block(x[:35], case["pos"][:35], case["views"][:1], 1, p)
    assert torch.allclose(one, BR.block(x, case["pos"], case["views"], 1, p)[:35], rtol=0, atol=1e-13)


def test_abi_21_symbols_signatures_and_descriptors():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION >= 21
    for name in NEW:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == _lib.PROTOTYPES[name][0], name
    A, B = _lib.MlpSublayerArgs, _lib.AttnSublayerArgs
    assert C.sizeof(A) == 8 * 8 + 4 * 4 + 8 * 8 and A.M.offset == 64 and A.out.offset == 80 and A.db2.offset == 136
    assert C.sizeof(B) == 11 * 8 + 6 * 4 + 8 * 8 and B.views.offset == 80 and B.M.offset == 88 and B.out.offset == 112 and B.dbproj.offset == 168
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "must3r_hip.h")) as f:
        header = f.read()
    assert "#define MUST3R_HIP_ABI_VERSION 21" in header
    for name in NEW:
        assert name + "(" in header, name


def test_scratch_queries_answer_without_a_device():
    lib = _lib.load()
    mlp, attn = lib.must3r_hip_mlp_sublayer_scratch_bytes, lib.must3r_hip_attn_sublayer_scratch_bytes
    wg, ln, core = lib.must3r_hip_op_linear_wgrad_scratch_bytes, lib.must3r_hip_op_layernorm_grad_scratch_bytes, lib.must3r_hip_attn_train_scratch_bytes
    up = lambda v: (v + 255) // 256 * 256
    for M, D, Hd in ((151, 128, 512), (192, 768, 3072), (15360, 1024, 4096)):
        assert mlp(M, D, Hd) == up(4 * M * D) + 2 * up(4 * M * Hd) + up(max(wg(M, D, Hd), wg(M, Hd, D))) + up(ln(M, D)), (M, D, Hd)
        n = 3
        assert attn(M, D, n) == 3 * up(4 * M * D) + 2 * up(12 * M * D) + up(max(wg(M, 3 * D, D), wg(M, D, D))) + up(ln(M, D)) + up(core(n, M, M, D // 64))
    # the attention core's part is asked for M query and M key rows: a table inside the M rows never needs more (its own query is monotonic in the rows)
    assert all(core(3, r, r, 2) <= core(3, 151, 151, 2) for r in (1, 17, 70, 150, 151)) and core(3, 151, 9999, 2) == core(3, 151, 151, 2)
    for bad in ((0, 128, 512), (-4, 128, 512), (10, 100, 512), (10, 0, 512), (10, 2048, 8192), (10, 128, 0), (10, 128, 100)):
        assert mlp(*bad) == 0, bad
    for bad in ((0, 128, 1), (10, 96, 1), (10, 1088, 1), (10, 128, 0), (10, 128, 70000)):
        assert attn(*bad) == 0, bad


def _mlp_call(fn, nbytes=0, scratch=None, **over):
    """A descriptor of fake but aligned addresses: every refusal comes before anything is read or launched."""
    lib = _lib.load()
    a = _lib.MlpSublayerArgs()
    for i, n in enumerate(("x", "gamma", "beta", "W1", "b1", "W2", "b2", "dy", "out", "dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2")):
        setattr(a, n, C.c_void_p(0x100000 * (i + 1)))
    a.M, a.D, a.hidden, a.eps = 10, 128, 512, 1e-6
    for k, v in over.items():
        setattr(a, k, v)
    rc = getattr(lib, fn)(C.byref(a), scratch, nbytes, None)
    return rc, lib.must3r_hip_last_error().decode()


def _attn_call(fn, views=((0, 6, 0, 6, 0, 0), (6, 4, 6, 4, 0, 0)), nbytes=0, scratch=None, **over):
    lib = _lib.load()
    t = torch.tensor([list(v) for v in views], dtype=torch.int32).contiguous()
    a = _lib.AttnSublayerArgs()
    for i, n in enumerate(("x", "gamma", "beta", "Wqkv", "bqkv", "Wproj", "bproj", "dy", "pos", "rope_tab", "out", "dx", "dgamma", "dbeta", "dWqkv", "dbqkv",
                           "dWproj", "dbproj")):
        setattr(a, n, C.c_void_p(0x100000 * (i + 1)))
    a.views, a.M, a.D, a.n_views, a.rope_npos, a.eps = C.c_void_p(t.data_ptr()), 10, 128, len(views), 256, 1e-6
    for k, v in over.items():
        setattr(a, "views" if k == "table" else k, v)
    rc = getattr(lib, fn)(C.byref(a), scratch, nbytes, None)
    return rc, lib.must3r_hip_last_error().decode()


@pytest.mark.parametrize("fn", ["must3r_hip_mlp_sublayer_forward", "must3r_hip_mlp_sublayer_grad"])
def test_mlp_sublayer_refuses_before_touching_anything(fn):
    lib = _lib.load()
    assert getattr(lib, fn)(None, None, 0, None) != 0 and "null" in lib.must3r_hip_last_error().decode()
    for over, word in ((dict(D=100), "multiple of 64"), (dict(D=1088), "1024"), (dict(D=0), "multiple of 64"), (dict(M=0), "M must"), (dict(hidden=100), "hidden"),
                       (dict(x=None), "null"), (dict(W2=None), "null"), (dict(x=C.c_void_p(0x100008)), "aligned"), (dict(W1=C.c_void_p(0x400004)), "aligned"),
                       (dict(b1=C.c_void_p(0x500004)), "aligned")):
        rc, msg = _mlp_call(fn, **over)
        assert rc != 0 and word in msg, (over, msg)
    rc, msg = _mlp_call(fn)
    assert rc != 0 and "scratch" in msg, msg
    need = lib.must3r_hip_mlp_sublayer_scratch_bytes(10, 128, 512)
    for scratch, nbytes in ((C.c_void_p(0x9000000), need - 1), (C.c_void_p(0x9000008), need)):
        rc, msg = _mlp_call(fn, scratch=scratch, nbytes=nbytes)
        assert rc != 0 and "scratch" in msg, msg


@pytest.mark.parametrize("fn", ["must3r_hip_attn_sublayer_forward", "must3r_hip_attn_sublayer_grad"])
def test_attn_sublayer_refuses_before_touching_anything(fn):
    lib = _lib.load()
    assert getattr(lib, fn)(None, None, 0, None) != 0 and "null" in lib.must3r_hip_last_error().decode()
    for over, word in ((dict(D=96), "multiple of 64"), (dict(D=2048), "1024"), (dict(M=-1), "M must"), (dict(x=None), "null"), (dict(pos=None), "pos"),
                       (dict(rope_tab=None), "rope_tab"), (dict(rope_npos=0), "position"), (dict(table=None), "views"), (dict(n_views=0), "n_views"),
                       (dict(Wqkv=C.c_void_p(0x400008)), "aligned"), (dict(pos=C.c_void_p(0x900008)), "aligned")):
        rc, msg = _attn_call(fn, **over)
        assert rc != 0 and word in msg, (over, msg)
    for views, word in ((((0, 6, 0, 6, 0, 0), (6, 5, 6, 4, 0, 0)), "reaches past"), (((0, 6, 0, 11, 0, 0),), "reaches past"), (((0, -6, 0, 6, 0, 0),), "negative"),
                        (((0, 6, 0, 6, 3, 7),), "skip")):
        rc, msg = _attn_call(fn, views=views)
        assert rc != 0 and word in msg, (views, msg)
    rc, msg = _attn_call(fn)
    assert rc != 0 and "scratch" in msg, msg
    rc, msg = _attn_call(fn, scratch=C.c_void_p(0x9000000), nbytes=lib.must3r_hip_attn_sublayer_scratch_bytes(10, 128, 2) - 1)
    assert rc != 0 and "scratch" in msg, msg


def test_overlapping_key_groups_are_refused_by_the_backward():
    views = ((0, 6, 0, 6, 0, 0), (6, 4, 3, 6, 0, 0))
    rc, msg = _attn_call("must3r_hip_attn_sublayer_grad", views=views)
    assert rc != 0 and "overlapping" in msg, msg
    rc, msg = _attn_call("must3r_hip_attn_sublayer_forward", views=views)          # the forward alone sums nothing over views
    assert rc != 0 and "scratch" in msg, msg


def test_operator_forms_refuse_before_launching():
    lib = _lib.load()
    P = lambda v: C.c_void_p(v)
    err = lambda: lib.must3r_hip_last_error().decode()
    lin = lambda epi=0, A=0x10000, lda=64, W=0x20000, b=0x30000, res=None, ldres=0, out=0x40000, ldc=64, z=None, ldz=0, M=6, N=64, K=64: \
        lib.must3r_hip_op_linear_f32(epi, P(A), lda, P(W), P(b), res, ldres, P(out), ldc, z, ldz, M, N, K, None)
    for kw, word in ((dict(K=40, lda=40), "multiple of 16"), (dict(N=62, ldc=64), "multiple of 16"), (dict(lda=66), "leading dimension"), (dict(lda=48), "leading dimension"),
                     (dict(ldc=60), "leading dimension"), (dict(A=0x10004), "aligned"), (dict(out=0x40008), "aligned"), (dict(b=0x30004), "aligned"),
                     (dict(epi=1), "null"), (dict(epi=1, res=P(0x50000), ldres=62), "leading dimension"), (dict(epi=1, res=P(0x50004), ldres=64), "aligned"),
                     (dict(epi=2, z=P(0x60000), ldz=8), "leading dimension"), (dict(epi=3), "epilogue"), (dict(N=0), "bad shape")):
        assert lin(**kw) != 0 and word in err(), (kw, err())
    assert lin(M=0) == 0
    rope = lambda t=0x10000, ld=384, pos=0x20000, tab=0x30000, npos=256, R=6, cols=256, d=1: lib.must3r_hip_op_rope_f32(P(t), ld, P(pos), P(tab), npos, R, cols, d, None)
    for kw, word in ((dict(cols=96), "multiple of 64"), (dict(d=0), "direction"), (dict(d=2), "direction"), (dict(ld=200), "leading dimension"), (dict(ld=386), "leading dimension"),
                     (dict(npos=0), "position"), (dict(t=0x10008), "aligned"), (dict(tab=0), "null")):
        assert rope(**kw) != 0 and word in err(), (kw, err())
    assert rope(cols=0) == 0 and rope(R=0) == 0
    gg = lambda dh=0x10000, ldh=64, z=0x20000, ldz=64, dz=0x10000, lddz=64, M=6, N=64: lib.must3r_hip_op_gelu_grad_f32(P(dh), ldh, P(z), ldz, P(dz), lddz, M, N, None)
    for kw, word in ((dict(N=62), "multiple of 4"), (dict(ldz=60), "leading dimension"), (dict(lddz=66), "leading dimension"), (dict(z=0x20004), "aligned"), (dict(z=0), "null")):
        assert gg(**kw) != 0 and word in err(), (kw, err())
    lng = lambda D=128, scratch=None, nb=0: lib.must3r_hip_op_layernorm_grad_add(P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x50000), None, None, 6, D, 1e-6,
                                                                              scratch, nb, None)
    assert lng(D=100) != 0 and "multiple of 64" in err()
    assert lng(D=1088) != 0 and "1024" in err()
    assert lng() != 0 and "scratch" in err()
    assert lng(scratch=P(0x900000), nb=lib.must3r_hip_op_layernorm_grad_scratch_bytes(6, 128) - 1) != 0 and "scratch" in err()


def test_python_refusals():
    x = torch.zeros(6, 128)
    w = lambda *s: torch.zeros(s)
    with pytest.raises(RuntimeError, match="GPU"):
        TB.mlp_sublayer(x, w(128), w(128), w(512, 128), w(512), w(128, 512), w(128))
    with pytest.raises(RuntimeError, match="GPU"):
        TB.attention_sublayer(x, torch.zeros(6, 2, dtype=torch.int64), [[0, 6, 0, 6, 0, 0]], 2, w(128), w(128), w(384, 128), w(384), w(128, 128), w(128))
    with pytest.raises(RuntimeError, match="GPU"):
        TB.linear(x, w(64, 128), w(64))
    with pytest.raises(RuntimeError, match="GPU"):
        TB.layer_norm(x, w(128), w(128))
    with pytest.raises(ValueError, match="heads"):
        TB.Block(128, 3)
    # a position at or past the table
    pos = BR.grid_positions(6, 3)
    assert TB.check_positions(pos, 3) is pos
    for bad in (torch.tensor([[0, 2]]), torch.tensor([[256, 0]]), torch.tensor([[-1, 0]])):
        with pytest.raises(ValueError, match="position"):
            TB.check_positions(bad, 2 if int(bad.max()) < 256 else 256)
    with pytest.raises(ValueError, match="int64"):
        TB.check_positions(pos.to(torch.int32), 256)
    # a tensor that passed is read again once it has changed, or for another table
    assert TB.check_positions(pos, 3) is pos
    pos[5, 1] = 3
    with pytest.raises(ValueError, match="position"):
        TB.check_positions(pos, 3)
    assert TB.check_positions(pos, 4) is pos
    with pytest.raises(ValueError, match="position"):
        TB.check_positions(pos, 3)


def test_block_keeps_the_reference_state_dict_keys_and_copies():
    from must3r_amd.model.blocks import EncBlockParams
    src = EncBlockParams(128, 4.0).half()
    blk = TB.Block.from_params(src)
    assert set(blk.state_dict()) == set(BR.PARAMS) == set(src.state_dict())
    assert all(v.dtype == torch.float32 for v in blk.state_dict().values()) and all(v.dtype == torch.float16 for v in src.state_dict().values())
    assert blk.num_heads == 2 and blk.mlp.fc1.weight.shape == (512, 128) and blk.eps == 1e-6
    assert torch.equal(blk.attn.qkv.weight, src.attn.qkv.weight.float()) and blk.attn.qkv.weight.data_ptr() != src.attn.qkv.weight.data_ptr()
