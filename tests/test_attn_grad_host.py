"""CPU: the host side of the attention training path -- the ABI 20 surface, the scratch queries, the refusals and the key-group rule of
must3r_hip_attn_grad, the two table helpers of must3r_amd.train_attention, and the yardstick tests/attn_grad_ref.py against torch's own
scaled_dot_product_attention (no compute calls: no GPU here)."""
import ctypes as C

import pytest
import torch

import attn_grad_ref as AR
from must3r_amd import _lib, train_attention as TA


def _tab(views):
    return torch.tensor(views, dtype=torch.int32).contiguous()


def _groups(views):
    t = _tab(views)
    lib = _lib.load()
    return lib.must3r_hip_attn_train_groups(C.c_void_p(t.data_ptr()), len(views)), lib.must3r_hip_last_error().decode()


def test_abi_20_symbols_signatures_and_descriptor():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION >= 20
    for name in ("must3r_hip_attn_train_scratch_bytes", "must3r_hip_attn_train_groups", "must3r_hip_attn_forward_f32", "must3r_hip_attn_grad"):
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == _lib.PROTOTYPES[name][0], name
    A = _lib.AttnTrainArgs
    assert [f[0] for f in A._fields_] == ["q", "k", "v", "dO", "ldq", "ldk", "ldv", "lddo", "heads", "n_views", "views", "O", "lse", "dQ", "dK", "dV",
                                          "ldo", "lddq", "lddk", "lddv"]
    assert C.sizeof(A) == 4 * 8 + 6 * 4 + 6 * 8 + 4 * 4 and A.views.offset == 56 and A.ldo.offset == 104


def test_scratch_queries_answer_without_a_device():
    lib = _lib.load()
    q = lib.must3r_hip_attn_train_scratch_bytes
    small, big = q(1, 6, 6, 2), q(560, 560 * 768, 560 * 768, 12)
    assert 0 < small and small % 256 == 0
    # the tables and two floats per (row, head): far below one operand
    assert 2 * 560 * 768 * 12 * 4 <= big < 560 * 768 * 768 * 4 // 8
    assert q(3, 100, 50, 2) == q(3, 100, 5000, 2)          # the key rows are not part of the layout
    assert q(3, 200, 50, 2) > q(3, 100, 50, 2) and q(3, 100, 50, 4) > q(3, 100, 50, 2)
    for bad in ((0, 6, 6, 2), (-1, 6, 6, 2), (1, -6, 6, 2), (1, 6, -6, 2), (1, 6, 6, 0), (70000, 6, 6, 2)):
        assert q(*bad) == 0, bad
    assert b"heads" in lib.must3r_hip_last_error()


def _call(fn_name, views=((0, 6, 0, 6, 0, 0),), nbytes=0, scratch=None, **over):
    """A descriptor of fake but aligned addresses: every refusal comes before anything is read or launched."""
    lib = _lib.load()
    t = _tab([list(v) for v in views])
    a = _lib.AttnTrainArgs()
    a.q, a.k, a.v, a.dO, a.O, a.dQ, a.dK, a.dV = (C.c_void_p(0x10000 * (i + 1)) for i in range(8))
    a.ldq = a.ldk = a.ldv = a.lddo = a.ldo = a.lddq = a.lddk = a.lddv = 128
    a.heads, a.n_views, a.views = 2, len(views), C.c_void_p(t.data_ptr())
    for k, v in over.items():
        setattr(a, "views" if k == "table" else k, v)
    rc = getattr(lib, fn_name)(C.byref(a), scratch, nbytes, None)
    return rc, lib.must3r_hip_last_error().decode()


@pytest.mark.parametrize("fn", ["must3r_hip_attn_forward_f32", "must3r_hip_attn_grad"])
def test_entry_points_refuse_before_touching_anything(fn):
    lib = _lib.load()
    assert getattr(lib, fn)(None, None, 0, None) != 0 and "null" in lib.must3r_hip_last_error().decode()
    for over, word in ((dict(q=None), "null"), (dict(k=None), "null"), (dict(v=None), "null"), (dict(table=None), "null"), (dict(heads=0), "heads"),
                       (dict(heads=-2), "heads"), (dict(ldq=127), "leading dimension"), (dict(ldk=126), "leading dimension"), (dict(ldv=64), "leading dimension"),
                       (dict(q=C.c_void_p(0x10008)), "aligned"), (dict(v=C.c_void_p(0x30004)), "aligned"), (dict(n_views=0), "n_views")):
        rc, msg = _call(fn, **over)
        assert rc != 0 and word in msg, (over, msg)
    for views, word in ((((0, 6, 0, 6, 4, 3),), "skip"), (((0, 6, 0, 6, 2, 7),), "skip"), (((0, -6, 0, 6, 0, 0),), "negative"),
                        (((0, 6, 0, 6, 0, 0), (6, 6, -1, 6, 0, 0)), "negative")):
        rc, msg = _call(fn, views=views)
        assert rc != 0 and word in msg, (views, msg)
    # a good descriptor gets as far as the scratch check
    rc, msg = _call(fn)
    assert rc != 0 and "scratch" in msg, msg
    rc, msg = _call(fn, scratch=C.c_void_p(0x900000), nbytes=lib.must3r_hip_attn_train_scratch_bytes(1, 6, 6, 2) - 1)
    assert rc != 0 and "scratch" in msg, msg


def test_direction_specific_refusals():
    assert "dO" in _call("must3r_hip_attn_grad", dO=None)[1]
    assert "leading dimension" in _call("must3r_hip_attn_grad", lddo=100)[1]
    assert "leading dimension" in _call("must3r_hip_attn_grad", lddk=130)[1]
    assert "aligned" in _call("must3r_hip_attn_grad", dV=C.c_void_p(0x80008))[1]
    assert "scratch" in _call("must3r_hip_attn_grad", dQ=None, dK=None, lddq=0, lddk=0)[1]      # leading dimensions of absent outputs are not read
    assert "(O)" in _call("must3r_hip_attn_forward_f32", O=None)[1]
    assert "leading dimension" in _call("must3r_hip_attn_forward_f32", ldo=64)[1]
    assert "scratch" in _call("must3r_hip_attn_forward_f32", dO=None, lse=None)[1]


def test_key_groups():
    # the decoder's tables: one group per view (self), one per scene (cross, masked or causal with nested prefixes)
    assert _groups(TA.self_views(2, 3, 70))[0] == 6
    assert _groups(TA.memory_views(2, 3, 48, 80))[0] == 2
    assert _groups(TA.memory_views(1, 3, 48, 0, causal=True))[0] == 1
    assert _groups(TA.memory_views(2, 3, 48, 16, causal=True))[0] == 2
    assert _groups([[0, 4, 0, 10, 0, 0], [4, 4, 0, 6, 0, 0], [8, 4, 0, 8, 2, 5]])[0] == 1      # nested prefixes by hand
    # spans that touch are fine, spans that overlap are not -- in either order of the table
    assert _groups([[0, 4, 0, 10, 0, 0], [4, 4, 10, 5, 0, 0]])[0] == 2
    for views in ([[0, 4, 0, 10, 0, 0], [4, 4, 9, 5, 0, 0]], [[4, 4, 9, 5, 0, 0], [0, 4, 0, 10, 0, 0]], [[0, 4, 0, 10, 0, 0], [4, 4, 3, 2, 0, 0]]):
        n, msg = _groups(views)
        assert n == -1 and "overlapping" in msg, (views, msg)
        rc, msg = _call("must3r_hip_attn_grad", views=views)
        assert rc != 0 and "overlapping" in msg, (views, msg)
        with pytest.raises(_lib.HipError, match="overlapping"):
            TA.n_groups(views)
    # a view without keys overlaps nothing
    assert _groups([[0, 4, 0, 10, 0, 0], [4, 4, 5, 0, 0, 0]])[0] == 2
    assert _groups([[0, 4, 0, 10, 0, 0]])[0] == 1
    assert _lib.load().must3r_hip_attn_train_groups(None, 1) == -1


def test_table_helpers_against_hand_written_tables():
    n, Nm = 5, 7
    assert TA.self_views(2, 3, n) == [[0, 5, 0, 5, 0, 0], [5, 5, 5, 5, 0, 0], [10, 5, 10, 5, 0, 0],
                                      [15, 5, 15, 5, 0, 0], [20, 5, 20, 5, 0, 0], [25, 5, 25, 5, 0, 0]]
    # key rows of scene b start at b * (7 + 15) = 22 b
    assert TA.memory_views(2, 3, n, Nm) == [[0, 5, 0, 22, 7, 12], [5, 5, 0, 22, 12, 17], [10, 5, 0, 22, 17, 22],
                                            [15, 5, 22, 22, 7, 12], [20, 5, 22, 22, 12, 17], [25, 5, 22, 22, 17, 22]]
    assert TA.memory_views(2, 3, n, Nm, mask=False) == [[0, 5, 0, 22, 0, 0], [5, 5, 0, 22, 0, 0], [10, 5, 0, 22, 0, 0],
                                                        [15, 5, 22, 22, 0, 0], [20, 5, 22, 22, 0, 0], [25, 5, 22, 22, 0, 0]]
    assert TA.memory_views(2, 3, n, Nm, causal=True) == [[0, 5, 0, 7, 0, 0], [5, 5, 0, 12, 0, 0], [10, 5, 0, 17, 0, 0],
                                                         [15, 5, 22, 7, 0, 0], [20, 5, 22, 12, 0, 0], [25, 5, 22, 17, 0, 0]]
    assert TA.memory_views(2, 3, n, 0, causal=True) == [[0, 5, 0, 10, 0, 5], [5, 5, 0, 5, 0, 0], [10, 5, 0, 10, 0, 0],
                                                        [15, 5, 15, 10, 0, 5], [20, 5, 15, 5, 0, 0], [25, 5, 15, 10, 0, 0]]
    assert TA.memory_views(2, 1, n, Nm) == [[0, 5, 0, 7, 0, 0], [5, 5, 12, 7, 0, 0]]           # a lone view attends the memory alone


def test_row_coverage_decides_between_empty_and_zeros():
    tab = _tab(TA.memory_views(2, 3, 48, 80))
    assert TA._covers(TA.q_spans(tab), 288) and TA._covers(TA.kv_spans(tab), 448)
    assert not TA._covers(TA.q_spans(tab), 289) and not TA._covers(TA.kv_spans(tab), 449)
    causal = _tab(TA.memory_views(1, 3, 48, 0, causal=True))
    assert TA.kv_spans(causal) == [(0, 96)] and not TA._covers(TA.kv_spans(causal), 144)
    assert not TA._covers([(0, 4), (5, 9)], 9) and TA._covers([(4, 9), (0, 4)], 9)


def test_python_refusals():
    q = torch.zeros(6, 128)
    with pytest.raises(RuntimeError, match="GPU"):
        TA.attention(q, q, q, TA.self_views(1, 1, 6), 2)
    with pytest.raises(ValueError, match="expected"):
        TA._table([[0, 6, 0, 6, 0]])
    with pytest.raises(ValueError, match="reaches past"):
        TA._check_table(_tab([[0, 7, 0, 6, 0, 0]]), 6, 6)
    with pytest.raises(ValueError, match="reaches past"):
        TA._check_table(_tab([[0, 6, 1, 6, 0, 0]]), 6, 6)
    with pytest.raises(ValueError, match="skip"):
        TA._check_table(_tab([[0, 6, 0, 6, 3, 7]]), 6, 6)
    with pytest.raises(ValueError, match="negative"):
        TA._check_table(_tab([[0, 6, 0, 6, -1, 2]]), 6, 6)


@pytest.mark.parametrize("name", ["self_ragged", "cross_shared", "cross_whole_tile", "causal"])
def test_yardstick_matches_torch_sdpa(name):
    """Every row of these cases has a key: the branch the reference takes (F.scaled_dot_product_attention with a boolean mask), forward and
    backward under CPU autograd in fp64."""
    case = AR.make_case(name)
    heads = case["heads"]
    mine = AR.grads(case, torch.float64)
    q, k, v = (case[n].double().clone().requires_grad_(True) for n in ("q", "k", "v"))
    o = torch.zeros_like(q)
    for view in case["views"]:
        q0, nq, k0, nk, _, _ = view
        split = lambda t, r0, n: t[r0:r0 + n].reshape(n, heads, 64).transpose(0, 1)
        oh = torch.nn.functional.scaled_dot_product_attention(split(q, q0, nq), split(k, k0, nk), split(v, k0, nk), attn_mask=AR.bool_mask(view))
        o[q0:q0 + nq] = oh.transpose(0, 1).reshape(nq, heads * 64)
    o.backward(case["dO"].double())
    for n, t in (("O", o.detach()), ("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
        assert torch.isfinite(t).all()
        assert torch.allclose(mine[n], t, rtol=1e-10, atol=1e-12 * float(t.abs().max())), n


def test_yardstick_degenerate_views_give_zeros_not_nan():
    case = AR.make_case("degenerate")
    alone = dict(case, views=case["views"][:1])
    for dt in (torch.float64, torch.float32):
        g, ga = AR.grads(case, dt), AR.grads(alone, dt)
        assert all(bool(torch.isfinite(t).all()) for t in g.values())
        assert bool((g["O"][40:] == 0).all()) and bool((g["dQ"][40:] == 0).all())
        assert torch.equal(g["dK"], ga["dK"]) and torch.equal(g["dV"], ga["dV"]) and float(g["dK"].abs().max()) > 0
