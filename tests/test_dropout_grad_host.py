"""CPU: the host side of memory dropout -- the restated selectors of must3r_amd/train_dropout.py against the reference's (blocks/dropout.py) under the same
CPU seed, the yardstick tests/dropout_ref.py against the reference's own CausalMUSt3R(mem_dropout=0.3) in fp64 (live where the reference tree exists, from the
recorded fixture tests/golden/decoder_dropout_d64.npz everywhere), pack_key_mask against numpy's packbits, and the additive ABI 21 surface of the masked
attention and cross-sublayer entry points: symbols, descriptor offsets, scratch queries and refusals (no compute calls: no GPU here).

The case is dropout_ref.make_case: B 2, n 35, Denc 128, D 64 / 1 head, depth 3, single_mlp, causal, schedule (2, 3, 1, 2 views, then a render of 2), with
mem_dropout 0.3, protected_imgs 1 and torch.manual_seed(5) before the first call, selectors on the CPU.  The reference's selector outputs are recorded per
call and handed to the yardstick, so both sides drop the same rows.  Tolerance and the treatment of cross_attn.projk.bias: those of
tests/test_decoder_grad_host.py (rtol 1e-10, atol 1e-12 max|r|; the fixture holds 32 seeded +-1 projections per tensor and is only written after the live
comparison has passed).  Every mask the reference applies must drop at least one key and keep at least one: a degenerate draw cannot pass silently."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

import decoder_ref as DF
import dropout_ref as DO
from conftest import GOLDEN, HAS_REFERENCE, ROOT
from must3r_amd import _lib, train_attention as TA, train_dropout as TDO
from test_decoder_grad_host import KBIAS, _close, _digest

FIXTURE = os.path.join(GOLDEN, "decoder_dropout_d64.npz")
NEW_ATTN = ("must3r_hip_attn_masked_scratch_bytes", "must3r_hip_attn_masked_forward", "must3r_hip_attn_masked_grad")
NEW_CROSS = ("must3r_hip_cross_sublayer_masked_scratch_bytes", "must3r_hip_cross_sublayer_masked_forward", "must3r_hip_cross_sublayer_masked_grad")
# (dropout_mode, use_mem_mask, memory mode): norm_y with every gradient in all four classes; kv and raw with outputs and data gradients
KINDS = [(d, m, "norm_y") for d in ("temporary", "permanent") for m in (False, True)] + [(d, False, mode) for d in ("temporary", "permanent") for mode in ("kv", "raw")]
# the issue's log of the reference's run: (kept, dropped) per masked-or-not view of every call, and the memory after each permanent update
TEMPORARY_LOG = [([35, 70], [0, 0]), ([92, 119, 141], [13, 21, 34]), ([157], [53]), ([174, 213], [71, 67]), ([206], [74])]
PERMANENT_ROWS = [57, 98, 102, 92]
# the selectors alone: name -> (class, p, (Nm, nimgs, N, protected))
SELECTOR_CASES = {"temp_p03_prot0": ("T", 0.3, (70, 3, 35, 0)), "temp_p03_prot35": ("T", 0.3, (70, 3, 35, 35)), "temp_keep40": ("T", 40, (70, 3, 35, 0)),
                  "temp_keep40_prot35": ("T", 40, (70, 2, 35, 35)), "perm_p03_prot0": ("P", 0.3, (70, 3, 35, 0)), "perm_p03_prot35": ("P", 0.3, (70, 3, 35, 35)),
                  "perm_keep40": ("P", 40, (70, 3, 35, 0)), "perm_keep40_prot35": ("P", 40, (0, 2, 35, 35)), "temp_nothing_to_draw": ("T", 0.3, (0, 2, 35, 35)),
                  "temp_all_protected": ("T", 0.3, (35, 1, 35, 80))}


@functools.lru_cache(maxsize=None)
def _case(mode):
    return DO.make_case(mode)


def _reference_module():
    from oracle import ref_shims
    ref_shims.import_reference_model()
    return importlib.import_module("must3r.model.decoder"), importlib.import_module("must3r.model.blocks.dropout")


def _reference(case, dropout_mode, use_mem_mask):
    """Outputs, gradients and the selector outputs per call of the reference's own class in fp64 on the CPU (its head in fp32, unused)."""
    dmod, _ = _reference_module()
    dec = dmod.CausalMUSt3R(protected_imgs=DO.PROTECTED_IMGS, mem_dropout=DO.P_DROP, dropout_mode=dropout_mode, use_mem_mask=use_mem_mask,
                            img_size=(case["H"], case["W"]), enc_embed_dim=case["Denc"], patch_size=16, embed_dim=case["D"], output_dim=1792,
                            depth=case["depth"], num_heads=case["heads"], mlp_ratio=case["hidden"] / case["D"], feedback_type=case["feedback_type"],
                            memory_mode=case["mode"], landscape_only=False)
    dec.load_state_dict(case["params"], strict=True)
    dec.double()
    dec.head_dec.float()
    drawn = []
    inner = dec.mem_dropout.forward

    def recording(*a, **kw):
        out = inner(*a, **kw)
        drawn.append(out)
        return out
    dec.mem_dropout.forward = recording
    B, n = case["scenes"], case["n"]
    mem, loss, res, xs, selections = None, 0, {}, [], []
    torch.manual_seed(DO.SEED)
    for i, c in enumerate(case["calls"]):
        x = c["x"].double().clone().requires_grad_(True)
        xs.append(x)
        pos = case["pos"].view(1, 1, n, 2).expand(B, c["V"], n, 2).contiguous()
        ts = torch.tensor([case["H"], case["W"]]).view(1, 1, 2).expand(B, c["V"], 2).contiguous()
        before = len(drawn)
        mem, _, feats = dec(x, pos, ts, mem, render=c["render"], return_feats=True)
        assert len(drawn) - before <= 1
        selections.append(drawn[-1] if len(drawn) > before else None)
        f = feats[-1].reshape(-1, case["D"])
        res[f"feats{i}"] = f.detach()
        loss = loss + (f * c["T"].double()).sum()
    loss.backward()
    res.update({f"mem{l}": m.detach() for l, m in enumerate(mem[0])})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    res.update({k: t.grad for k, t in dec.named_parameters() if t.grad is not None})
    res["tail"] = torch.tensor([float(mem[2]), float(mem[3]), float(mem[4])], dtype=torch.float64)
    res["labels"] = mem[1]
    return res, selections


def _checked(case):
    n = len(case["calls"])
    names = [f"feats{i}" for i in range(n)] + [f"mem{l}" for l in range(case["depth"])] + [f"dx{i}" for i in range(n)]
    if case["mode"] == "norm_y":
        names += [k for k in DF.param_names(case["depth"], case["feedback_type"]) if not k.startswith("head_dec.")]
    return names


def _pack_selections(dropout_mode, selections):
    out = {}
    for c, s in enumerate(selections):
        out[f"drawn__{dropout_mode}__{c}"] = np.array(0 if s is None else len(s[0]))
        if s is not None:
            for i, (a, b) in enumerate(zip(*s)):
                out[f"sel__{dropout_mode}__{c}__{i}"], out[f"notsel__{dropout_mode}__{c}__{i}"] = a.numpy().astype(np.int32), b.numpy().astype(np.int32)
    return out


def _recorded_selections(rec, dropout_mode, n_calls):
    out = []
    for c in range(n_calls):
        k = int(rec[f"drawn__{dropout_mode}__{c}"])
        out.append(None if k == 0 else ([torch.from_numpy(rec[f"sel__{dropout_mode}__{c}__{i}"]).long() for i in range(k)],
                                        [torch.from_numpy(rec[f"notsel__{dropout_mode}__{c}__{i}"]).long() for i in range(k)]))
    return out


def _check_selection_log(case, dropout_mode, selections):
    """what the issue quotes of the reference's run, and: every applied mask drops at least one key and keeps at least one"""
    n, state, applied = case["n"], DO.new_state(), 0
    Nm = 0
    for ci, (c, s) in enumerate(zip(case["calls"], selections)):
        V, render = c["V"], c["render"]
        if dropout_mode == "temporary":
            kept, dropped = TEMPORARY_LOG[ci]
            assert [len(a) for a in s[0]] == kept and [len(b) for b in s[1]] == dropped, (ci, [len(a) for a in s[0]], [len(b) for b in s[1]])
        Nk = Nm if render else Nm + V * n
        if s is not None and (render or Nm > 0 or V > 1):
            for j, keep in enumerate(DO.view_keeps(s, 1, V, Nk, render)):
                if keep is None:
                    continue
                view = DF.cross_table(1, V, n, Nm, render, True)[j]
                valid, plain = DO.valid_keys(view, keep), DO.valid_keys(view)
                assert 0 < int(valid.sum()) < int(plain.sum()), (dropout_mode, ci, j)
                applied += 1
        if not render:
            Nm = Nk if dropout_mode == "temporary" else len(s[0][-1])
            if dropout_mode == "permanent":
                assert Nm == PERMANENT_ROWS[ci], (ci, Nm)
                assert bool((s[0][-1][1:] > s[0][-1][:-1]).all()), "the kept rows stay in ascending order"
    # temporary: views 0 and 1 of the 3-view call, view 0 of the 2-view call, both views of the render; permanent: views 1 and 2, and view 1
    assert applied == (5 if dropout_mode == "temporary" else 3), (dropout_mode, applied)


def _my_selections(case, dropout_mode, recorded):
    """the restated selectors under the seed, over the calls of the schedule (the memory's size in the permanent mode follows the draw)"""
    sel = (TDO.TemporaryMemoryDropoutSelector if dropout_mode == "temporary" else TDO.MemoryDropoutSelector)(DO.P_DROP)
    n, state, Nm, out = case["n"], DO.new_state(), 0, []
    torch.manual_seed(DO.SEED)
    for c in case["calls"]:
        V, render = c["V"], c["render"]
        prot = DO.protected_tokens(state, V, n, render)
        if render:
            out.append(sel(Nm, 1, 0, protected=prot, device="cpu") if dropout_mode == "temporary" else None)
            continue
        s = sel(Nm, V, n, protected=prot, device="cpu")
        out.append(s)
        p_imgs = min(DO.PROTECTED_IMGS, state["prot_imgs"] + V)
        state = dict(state, prot_tokens=prot, prot_imgs=p_imgs)
        Nm = Nm + V * n if dropout_mode == "temporary" else len(s[0][-1])
    return out


def _same_lists(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    for x, y in zip(a, b):
        assert len(x) == len(y), what
        for i, (u, v) in enumerate(zip(x, y)):
            assert u.dtype in (torch.int64, torch.int32) and torch.equal(u.long(), v.long()), (what, i)


def _selector_case(mods, name):
    kind, p, args = SELECTOR_CASES[name]
    cls = getattr(mods, "TemporaryMemoryDropoutSelector" if kind == "T" else "MemoryDropoutSelector")
    torch.manual_seed(1234)
    return cls(p)(*args[:3], protected=args[3], device="cpu")


def test_yardstick_and_selectors_match_the_reference():
    rec_out = {}
    if HAS_REFERENCE:
        _, rdrop = _reference_module()
        for name in SELECTOR_CASES:
            ref = _selector_case(rdrop, name)
            _same_lists(_selector_case(TDO, name), ref, name)
            for i, (a, b) in enumerate(zip(*ref)):
                rec_out[f"selcase__{name}__sel{i}"], rec_out[f"selcase__{name}__notsel{i}"] = a.numpy().astype(np.int32), b.numpy().astype(np.int32)
        packed = set()
        for dropout_mode, use_mem_mask, mode in KINDS:
            case = _case(mode)
            ref, selections = _reference(case, dropout_mode, use_mem_mask)
            _check_selection_log(case, dropout_mode, selections)
            for mine, theirs in zip(_my_selections(case, dropout_mode, selections), selections):
                _same_lists(mine, theirs, (dropout_mode, "schedule"))
            if dropout_mode not in packed:
                rec_out.update(_pack_selections(dropout_mode, selections))
                packed.add(dropout_mode)
            extra = {}
            mine = DO.grads(case, torch.float64, selections, dropout_mode, "feats", extra)
            assert ref["tail"].tolist() == mine["tail"].tolist() == [8, 1, 35]
            assert torch.equal(ref["labels"], mine["labels"])
            kind = f"{dropout_mode}__{'memmask' if use_mem_mask else 'plain'}__{mode}"
            for k in _checked(case):
                r, m = ref[k], float(ref[k].abs().max())
                assert m > 0, (kind, k)
                if k.endswith(KBIAS):
                    m = extra[k]
                    assert float(r.abs().max()) < 1e-12 * m, (kind, k)
                _close(mine[k], r, m, (kind, k))
                rec_out[f"{kind}__{k}"] = _digest(r).numpy()
            rec_out[f"{kind}__tail"] = ref["tail"].numpy()
    if HAS_REFERENCE and os.environ.get("M3R_WRITE_DROPOUT_GOLDEN"):
        np.savez_compressed(FIXTURE, x=_case("norm_y")["calls"][1]["x"].numpy(), **rec_out)
    rec = np.load(FIXTURE)
    assert np.array_equal(rec["x"], _case("norm_y")["calls"][1]["x"].numpy()), "the seeded case is not the one the fixture was recorded on"
    for name in SELECTOR_CASES:
        mine = _selector_case(TDO, name)
        k = len(mine[0])
        _same_lists(mine, ([torch.from_numpy(rec[f"selcase__{name}__sel{i}"]) for i in range(k)],
                           [torch.from_numpy(rec[f"selcase__{name}__notsel{i}"]) for i in range(k)]), name)
        assert f"selcase__{name}__sel{k}" not in rec
    for dropout_mode, use_mem_mask, mode in KINDS:
        case = _case(mode)
        selections = _recorded_selections(rec, dropout_mode, len(case["calls"]))
        _check_selection_log(case, dropout_mode, selections)
        for mine, theirs in zip(_my_selections(case, dropout_mode, selections), selections):
            _same_lists(mine, theirs, (dropout_mode, "schedule"))
        extra = {}
        mine = DO.grads(case, torch.float64, selections, dropout_mode, "feats", extra)
        kind = f"{dropout_mode}__{'memmask' if use_mem_mask else 'plain'}__{mode}"
        assert rec[f"{kind}__tail"].tolist() == mine["tail"].tolist() == [8, 1, 35]
        for k in _checked(case):
            r, t = torch.from_numpy(rec[f"{kind}__{k}"]), _digest(mine[k])
            m = float(r.abs().max())
            if k.endswith(KBIAS):
                m = extra[k] * mine[k].numel() ** 0.5
                assert float(r.abs().max()) < 1e-12 * m, (kind, k)
            else:
                assert m > 0, (kind, k)
            _close(t, r, m, (kind, k))


def test_selector_edge_cases():
    """N_x <= 0 draws nothing and consumes nothing; p = 0 returns (None, None); the keep-p form keeps exactly p rows; keep() is sel() as a mask"""
    for cls in (TDO.MemoryDropoutSelector, TDO.TemporaryMemoryDropoutSelector):
        assert cls(0.0)(70, 2, 35, device="cpu") == (None, None)
        torch.manual_seed(3)
        state = torch.get_rng_state()
        s, ns = cls(0.3).sel(35, 35, "cpu")
        assert torch.equal(s, torch.arange(35)) and ns.numel() == 0 and ns.dtype == torch.int and torch.equal(torch.get_rng_state(), state)
        s, ns = cls(0.3).sel(20, 35, "cpu")
        assert torch.equal(s, torch.arange(20)) and ns.numel() == 0
        # the keep-p form: 60 of 100 rows leave sel; the reference's not_sel is the head of the sorted sel (dropout.py:21-22), at most count rows of it
        s, ns = cls(40).sel(100, 0, "cpu")
        assert len(s) == 40 and torch.equal(ns, s[:60]) and bool((s[1:] > s[:-1]).all())
        s, ns = cls(40).sel(100, 35, "cpu")
        assert len(s) == 40 and s[:35].tolist() == list(range(35)) and torch.equal(ns, s[35:])
        s, ns = cls(90).sel(100, 0, "cpu")
        assert len(s) == 90 and torch.equal(ns, s[:10])
        s, ns = cls(40).sel(30, 0, "cpu")          # fewer rows than p: nothing to drop
        assert len(s) == 30 and len(ns) == 0
        g = torch.Generator().manual_seed(9)
        keep = cls(0.3, generator=g).keep(200, 35, "cpu")
        g.manual_seed(9)
        s, ns = cls(0.3, generator=g).sel(200, 35, "cpu")
        assert keep.dtype == torch.bool and bool(keep[:35].all()) and torch.equal(torch.nonzero(~keep).view(-1), ns) and 0 < len(ns) < 165
        assert torch.equal(ns, s[35:35 + len(ns)]) and len(s) + len(ns) == 200
    with pytest.raises(ValueError, match="dropout mode"):
        TDO.CausalMUSt3R(mem_dropout=0.1, dropout_mode="sometimes", enc_embed_dim=128, embed_dim=64, depth=1, num_heads=1)


def test_module_keeps_the_state_dict_and_the_parents_refusal():
    from must3r_amd import train_decoder as TD
    kw = dict(enc_embed_dim=128, embed_dim=64, depth=2, num_heads=1, feedback_type="single_mlp")
    a, b = TD.CausalMUSt3R(**kw), TDO.CausalMUSt3R(mem_dropout=0.1, **kw)
    assert list(a.state_dict()) == list(b.state_dict()) and isinstance(b.mem_dropout, TDO.TemporaryMemoryDropoutSelector) and b.mem_dropout.p == 0.1
    assert isinstance(TDO.CausalMUSt3R(mem_dropout=0.1, dropout_mode="permanent", **kw).mem_dropout, TDO.MemoryDropoutSelector)
    with pytest.raises(NotImplementedError):
        TD.CausalMUSt3R(mem_dropout=0.1, **kw)
    x, pos, ts = torch.zeros(1, 2, 35, 128), torch.zeros(1, 2, 35, 2, dtype=torch.int64), torch.tensor([[[80, 112]] * 2])
    with pytest.raises(RuntimeError, match="GPU"):
        b(x, pos, ts)


@pytest.mark.parametrize("nk", [1, 31, 32, 33, 64, 200])
def test_pack_key_mask_against_packbits(nk):
    g = torch.Generator().manual_seed(nk)
    keep = torch.rand((5, nk), generator=g) < 0.6
    keep[3], keep[4] = True, False
    words = TA.pack_key_mask(keep)
    ld = words.shape[1]
    assert words.dtype == torch.int32 and ld % 2 == 0 and 32 * ld >= nk and 32 * (ld - 2) < max(nk, 1)
    padded = np.zeros((5, 32 * ld), dtype=np.uint8)
    padded[:, :nk] = keep.numpy()
    ref = np.packbits(padded, axis=1, bitorder="little").view("<u4")
    assert np.array_equal(words.numpy().view(np.uint32), ref)
    for j in range(nk):     # the kernels' rule: bit j % 32 of word j // 32
        assert ((words.numpy().view(np.uint32)[:, j // 32] >> (j % 32)) & 1).tolist() == keep[:, j].int().tolist()
    with pytest.raises(ValueError, match="bool"):
        TA.pack_key_mask(keep.int())


def test_additive_abi_21_symbols_and_descriptors():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION == 21
    for name in NEW_ATTN + NEW_CROSS:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == _lib.PROTOTYPES[name][0], name
    assert _lib.PROTOTYPES[NEW_ATTN[0]] == (C.c_size_t, [C.c_int] * 4) and _lib.PROTOTYPES[NEW_CROSS[0]] == (C.c_size_t, [C.c_int] * 5)
    for name in NEW_ATTN[1:]:
        assert _lib.PROTOTYPES[name] == (C.c_int, [C.POINTER(_lib.AttnMaskedArgs), C.c_void_p, C.c_size_t])
    for name in NEW_CROSS[1:]:
        assert _lib.PROTOTYPES[name] == (C.c_int, [C.POINTER(_lib.CrossSublayerMaskedArgs), C.c_void_p, C.c_size_t])
    A, X = _lib.AttnMaskedArgs, _lib.CrossSublayerMaskedArgs
    assert C.sizeof(_lib.AttnTrainArgs) == 120 and C.sizeof(_lib.CrossSublayerArgs) == 256          # the embedded descriptors keep their layout
    assert (A.core.offset, A.mask_bits.offset, A.view_mask.offset, A.mask_rows.offset, A.mask_ld.offset, A.stream.offset, C.sizeof(A)) == (0, 120, 128, 136, 140, 144, 152)
    assert (X.core.offset, X.mask_bits.offset, X.view_mask.offset, X.mask_rows.offset, X.mask_ld.offset, C.sizeof(X)) == (0, 256, 264, 272, 276, 280)
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        header = f.read()
    assert "#define MUST3R_HIP_ABI_VERSION 21" in header
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ATTN + NEW_CROSS:
        decl = re.findall(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;{}]*)\)\s*;", plain)
        assert len(decl) == 1, name
        assert not re.search(r"void\*\s*stream\s*$", decl[0]), f"{name}: the stream travels in the descriptor"
        # the comment block in front of the declaration is marked as additive
        block = header[:header.index(name + "(")]
        assert block[block.rindex("/* ABI"):].startswith("/* ABI 21, additive."), name
    for struct, cls in (("must3r_hip_attn_masked_args", A), ("must3r_hip_cross_sublayer_masked_args", X)):
        body = plain[plain.index("typedef struct " + struct + " {"):plain.index("} " + struct + ";")].split("{", 1)[1]
        names = []
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if stmt:
                names += [n.strip().lstrip("*").strip() for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", stmt, count=1).split(",")]
        assert names == [f[0] for f in cls._fields_], names
    assert re.search(r"void\*\s*stream;", plain[plain.index("typedef struct must3r_hip_attn_masked_args {"):plain.index("} must3r_hip_attn_masked_args;")])


def test_scratch_queries_are_monotone_and_cover_the_unmasked_ones():
    lib = _lib.load()
    qa, qu = lib.must3r_hip_attn_masked_scratch_bytes, lib.must3r_hip_attn_train_scratch_bytes
    xa, xu = lib.must3r_hip_cross_sublayer_masked_scratch_bytes, lib.must3r_hip_cross_sublayer_scratch_bytes
    up = lambda v: (v + 255) // 256 * 256
    shapes = [(1, 1, 1, 1), (6, 420, 400, 2), (6, 420, 400, 12), (64, 420, 400, 2), (65, 420, 400, 2), (400, 15360, 15360, 12)]
    for n, rq, rk, h in shapes:
        assert qa(n, rq, rk, h) == qu(n, rq, rk, h) + up(4 * n) and qa(n, rq, rk, h) % 256 == 0, (n, rq, rk, h)
    last = 0
    for n in (1, 2, 64, 65, 128, 129, 4096):
        v = qa(n, 420, 400, 2)
        assert v >= last
        last = v
    assert qa(6, 840, 400, 2) >= qa(6, 420, 400, 2) and qa(6, 420, 400, 4) >= qa(6, 420, 400, 2)
    for bad in ((0, 10, 10, 1), (65536, 10, 10, 1), (3, -1, 10, 1), (3, 10, -1, 1), (3, 10, 10, 0), (3, 10, 10, 65536)):
        assert qa(*bad) == 0, bad
    for M, Rm, D, n, kv in ((140, 280, 128, 4, 0), (140, 280, 128, 4, 1), (70, 35, 64, 1, 0), (15360, 30720, 768, 20, 1)):
        assert xa(M, Rm, D, n, kv) == xu(M, Rm, D, n, kv) + up(4 * n), (M, Rm, D, n, kv)
    assert xa(280, 280, 128, 4, 0) >= xa(140, 280, 128, 4, 0) and xa(140, 560, 128, 4, 0) >= xa(140, 280, 128, 4, 0)
    for bad in ((0, 10, 64, 1, 0), (10, 0, 64, 1, 0), (10, 10, 96, 1, 0), (10, 10, 1088, 1, 0), (10, 10, 64, 0, 0), (10, 10, 64, 65536, 1)):
        assert xa(*bad) == 0, bad


VIEWS = np.array([[0, 70, 0, 200, 0, 0], [70, 70, 0, 200, 100, 140]], dtype=np.int32)
VMASK = np.array([0, -1], dtype=np.int32)


def _attn_call(fn, views=VIEWS, vmask=VMASK, scratch=0x9000000, nbytes=None, **over):
    """A masked attention descriptor of fake but aligned device addresses over real host tables: every refusal comes before anything is read through a device
    pointer or launched."""
    lib = _lib.load()
    a = _lib.AttnMaskedArgs()
    c = a.core
    c.q, c.k, c.v, c.dO, c.O, c.lse, c.dQ, c.dK, c.dV = (0x1000000 * (i + 1) for i in range(9))
    c.ldq = c.ldk = c.ldv = c.lddo = c.ldo = c.lddq = c.lddk = c.lddv = 128
    c.heads, c.n_views, c.views = 2, len(views), views.ctypes.data
    a.mask_bits, a.view_mask, a.mask_rows, a.mask_ld, a.stream = 0xa000000, (None if vmask is None else vmask.ctypes.data), 2, 8, None
    for k, v in over.items():
        setattr(c if hasattr(c, k) and k not in ("mask_bits", "view_mask", "mask_rows", "mask_ld", "stream") else a, k, v)
    need = lib.must3r_hip_attn_masked_scratch_bytes(len(views), 140, 200, 2)
    rc = getattr(lib, fn)(C.byref(a), scratch, need if nbytes is None else nbytes)
    return rc, lib.must3r_hip_last_error().decode()


MASK_REFUSALS = [(dict(mask_bits=None), "come together"), (dict(vmask=None), "come together"), (dict(mask_ld=7), "even"), (dict(mask_ld=0), "even"),
                 (dict(mask_ld=-2), "even"), (dict(mask_rows=-1), "mask_rows"), (dict(vmask=np.array([2, -1], dtype=np.int32)), "outside"),
                 (dict(vmask=np.array([0, -2], dtype=np.int32)), "outside"), (dict(mask_ld=6), "shorter"), (dict(mask_bits=0xa000004), "8-byte"),
                 (dict(vmask=np.array([0, 0], dtype=np.int32), mask_rows=0), "outside")]


@pytest.mark.parametrize("fn", NEW_ATTN[1:])
def test_masked_attention_refuses_before_touching_anything(fn):
    lib = _lib.load()
    assert getattr(lib, fn)(None, None, 0) != 0 and "null" in lib.must3r_hip_last_error().decode()
    grad = fn.endswith("_grad")
    refusals = list(MASK_REFUSALS) + [(dict(q=None), "null"), (dict(heads=0), "heads"), (dict(ldk=100), "leading dimension"), (dict(v=0x3000004), "aligned"),
                                      (dict(views=np.array([[0, 70, 0, 200, 120, 100]], dtype=np.int32), vmask=np.array([0], dtype=np.int32)), "skip"),
                                      (dict(views=np.array([[0, 70, 0, -1, 0, 0]], dtype=np.int32), vmask=np.array([0], dtype=np.int32)), "negative"),
                                      (dict(scratch=None), "scratch"), (dict(nbytes=256), "scratch"), (dict(scratch=0x9000008), "scratch")]
    refusals += [(dict(dO=None), "null")] if grad else [(dict(O=None), "null")]
    if grad:
        refusals.append((dict(views=np.array([[0, 70, 0, 200, 0, 0], [70, 70, 100, 100, 0, 0]], dtype=np.int32)), "overlapping"))
    for over, word in refusals:
        rc, msg = _attn_call(fn, **over)
        assert rc != 0 and word in msg, (over, msg)
    # a mask row exactly as long as nk passes the mask checks: the next refusal is the scratch
    rc, msg = _attn_call(fn, mask_ld=8, views=np.array([[0, 70, 0, 256, 0, 0]], dtype=np.int32), vmask=np.array([1], dtype=np.int32), scratch=None)
    assert rc != 0 and "scratch" in msg, msg


def _cross_call(fn, views=VIEWS, vmask=VMASK, scratch=0x9000000, nbytes=None, **over):
    lib = _lib.load()
    a = _lib.CrossSublayerMaskedArgs()
    c = a.core
    names = [f[0] for f in _lib.CrossSublayerArgs._fields_ if f[1] is C.c_void_p and f[0] not in ("views", "stream")]
    for i, n in enumerate(names):
        setattr(c, n, 0x1000000 * (i + 1))
    c.views, c.M, c.Rm, c.D, c.n_views, c.ldmem, c.lddmem, c.eps, c.stream = views.ctypes.data, 140, 200, 128, len(views), 128, 128, 1e-6, None
    a.mask_bits, a.view_mask, a.mask_rows, a.mask_ld = 0xa000000, (None if vmask is None else vmask.ctypes.data), 2, 8
    for k, v in over.items():
        setattr(a if k in ("mask_bits", "view_mask", "mask_rows", "mask_ld") else c, k, v)
    need = lib.must3r_hip_cross_sublayer_masked_scratch_bytes(140, 200, 128, len(views), 0)
    rc = getattr(lib, fn)(C.byref(a), scratch, need if nbytes is None else nbytes)
    return rc, lib.must3r_hip_last_error().decode()


@pytest.mark.parametrize("fn", NEW_CROSS[1:])
def test_masked_cross_sublayer_refuses_before_touching_anything(fn):
    lib = _lib.load()
    assert getattr(lib, fn)(None, None, 0) != 0 and "null" in lib.must3r_hip_last_error().decode()
    refusals = list(MASK_REFUSALS) + [(dict(x=None), "null"), (dict(D=96), "multiple of 64"), (dict(ldmem=100), "leading dimension"),
                                      (dict(Wk=None), "come together"), (dict(mem=0x2000004), "aligned"), (dict(Rm=150), "reaches past"),
                                      (dict(scratch=None), "scratch"), (dict(nbytes=256), "scratch")]
    for over, word in refusals:
        rc, msg = _cross_call(fn, **over)
        assert rc != 0 and word in msg, (fn, over, msg)


def test_python_refusals_of_the_masked_operators():
    q = torch.zeros(140, 128)
    with pytest.raises(RuntimeError, match="GPU"):
        TA.attention(q, q, q, TA.self_views(1, 2, 70), 2, key_mask=torch.zeros(1, 4, dtype=torch.int32), view_mask=[0, -1])
    tab = TA._table(VIEWS.tolist())
    bits = torch.zeros(2, 8, dtype=torch.int32)
    for km, vm, word in ((bits, None, "come together"), (None, [0, -1], "come together"), (bits.float(), [0, -1], "packed"), (bits[:, :7], [0, -1], "even"),
                         (bits, [0], "view_mask of shape"), (bits, [2, -1], "outside"), (bits, [0, -2], "outside"), (bits[:, :6], [0, -1], "shorter")):
        with pytest.raises(ValueError, match=word):
            TA._mask(km, vm, tab, torch.device("cpu"))
    assert TA._mask(None, None, tab, torch.device("cpu")) is None
    assert TA._mask(bits[:, :6], [-1, -1], tab, torch.device("cpu")) is not None        # nobody names the short rows
