"""CPU: the host side of the trainable decoder -- the yardstick tests/decoder_ref.py against the reference's own MUSt3R and CausalMUSt3R classes (live where
the reference tree exists, from the recorded fixture tests/golden/decoder_ref_d64.npz everywhere), the additive ABI 21 surface of csrc/train_decoder.hip, its
scratch query and its refusals (no compute calls: no GPU here), and the module's state-dict keys and Python refusals.

The schedule is decoder_ref.SCHEDULE on B = 2 scenes of 5 x 7 token views (n = 35), Denc 128, D 64 / 1 head, hidden 256, depth 3, single_mlp: an init of two
views, a lone view over the memory, two views over Nm = 105 and a render of two views over Nm = 175 (the key span crosses the 64-row key tile of
train_attention.hip).  The reference's head casts to fp32, so the comparison is on what it returns in fp64: feats[-1] (the tokens after norm_dec) per call, the
final memory, and the gradients of sum_c <feats_c, T_c> at every call's x and at the parameters.

Tolerance: that of tests/test_cross_grad_host.py, rtol 1e-10 and atol 1e-12 max|r|, with cross_attn.projk.bias treated as there (every key a view sees
carries the bias, the true gradient is zero: the magnitude is that of what cancels, max_c sum_r |dK_rc| of the fp64 yardstick, and the reference's own value
must lie below 1e-12 of it).  The fixture holds, per tensor, 32 seeded +-1 projections of the reference's fp64 values, not the values (the parameters'
gradients alone would be 2 MB per class): a projection is linear, so the yardstick's projections are held to the same rule against the recorded ones; the
live comparison is on the full tensors, and the fixture is only written after it has passed."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

import decoder_ref as DF
from conftest import GOLDEN, HAS_REFERENCE, ROOT
from must3r_amd import _lib, train_decoder as TD

FIXTURE = os.path.join(GOLDEN, "decoder_ref_d64.npz")
NEW = ("must3r_hip_feedback_prepare_scratch_bytes", "must3r_hip_feedback_prepare_forward", "must3r_hip_feedback_prepare_grad")
# the reference's class -> (causal, constructor arguments)
KINDS = {"must3r": (False, {}), "causal": (True, dict(use_mem_mask=False)), "causal_memmask": (True, dict(use_mem_mask=True))}
KBIAS = "cross_attn.projk.bias"


@functools.lru_cache(maxsize=None)
def _case(mode, causal):
    return DF.make_case(mode=mode, causal=causal)


def _reference(case, kw):
    """Outputs and gradients of the reference's own class in fp64 on the CPU (its head in fp32, unused)."""
    from oracle import ref_shims
    ref_shims.import_reference_model()
    dmod = importlib.import_module("must3r.model.decoder")
    common = dict(img_size=(case["H"], case["W"]), enc_embed_dim=case["Denc"], patch_size=16, embed_dim=case["D"], output_dim=1792, depth=case["depth"],
                  num_heads=case["heads"], mlp_ratio=case["hidden"] / case["D"], feedback_type=case["feedback_type"], memory_mode=case["mode"],
                  landscape_only=False)
    dec = dmod.CausalMUSt3R(protected_imgs=1, mem_dropout=0.0, **kw, **common) if case["causal"] else dmod.MUSt3R(**common)
    dec.load_state_dict(case["params"], strict=True)
    dec.double()
    dec.head_dec.float()
    B, n = case["scenes"], case["n"]
    mem, loss, res, xs = None, 0, {}, []
    for i, c in enumerate(case["calls"]):
        x = c["x"].double().clone().requires_grad_(True)
        xs.append(x)
        pos = case["pos"].view(1, 1, n, 2).expand(B, c["V"], n, 2).contiguous()
        ts = torch.tensor([case["H"], case["W"]]).view(1, 1, 2).expand(B, c["V"], 2).contiguous()
        mem, _, feats = dec(x, pos, ts, mem, render=c["render"], return_feats=True)
        f = feats[-1].reshape(-1, case["D"])
        res[f"feats{i}"] = f.detach()
        loss = loss + (f * c["T"].double()).sum()
    loss.backward()
    res.update({f"mem{l}": m.detach() for l, m in enumerate(mem[0])})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    res.update({k: t.grad for k, t in dec.named_parameters() if t.grad is not None})
    res["tail"] = torch.tensor([float(mem[2]), float(mem[3]), float(mem[4])], dtype=torch.float64)
    return res


def _checked(case):
    """norm_y: the outputs and every gradient; kv and raw: the outputs and the data gradients"""
    n = len(case["calls"])
    names = [f"feats{i}" for i in range(n)] + [f"mem{l}" for l in range(case["depth"])] + [f"dx{i}" for i in range(n)]
    if case["mode"] == "norm_y":
        names += [k for k in DF.param_names(case["depth"], case["feedback_type"]) if not k.startswith("head_dec.")]
    return names


def _digest(t, k=32):
    v = t.detach().double().reshape(-1)
    g = torch.Generator().manual_seed(1000003 + v.numel())
    P = torch.randint(0, 2, (k, v.numel()), generator=g, dtype=torch.int8).double() * 2 - 1
    return P @ v


def _close(t, r, m, what):
    assert r.dtype == torch.float64 and torch.isfinite(r).all(), what
    assert torch.allclose(t, r, rtol=1e-10, atol=1e-12 * m), (what, float((t - r).abs().max()), m)


def test_yardstick_matches_the_reference_decoders():
    rec_out = {}
    for kind, (causal, kw) in KINDS.items():
        for mode in DF.DR.MODES:
            case = _case(mode, causal)
            extra = {}
            mine = DF.grads(case, torch.float64, "feats", extra)
            names = _checked(case)
            assert set(names) <= set(mine)
            mags = {f"blocks_dec.{l}.{KBIAS}": extra[f"blocks_dec.{l}.{KBIAS}"] for l in range(case["depth"])}
            if HAS_REFERENCE:
                ref = _reference(case, kw)
                for k in names:
                    r, m = ref[k], float(ref[k].abs().max())
                    assert m > 0, (kind, mode, k)
                    if k in mags:
                        m = mags[k]
                        assert float(r.abs().max()) < 1e-12 * m, (kind, mode, k)
                    _close(mine[k], r, m, (kind, mode, k))
                # the tuple's bookkeeping: images, protected images, protected tokens
                assert ref["tail"].tolist() == ([5, 5, 175] if not causal else [5, 1, 35]), (kind, ref["tail"])
                rec_out.update({f"{kind}__{mode}__{k}": _digest(ref[k]).numpy() for k in names})
    if HAS_REFERENCE and os.environ.get("M3R_WRITE_DECODER_GOLDEN"):
        np.savez_compressed(FIXTURE, x=_case("norm_y", False)["calls"][0]["x"].numpy(), **rec_out)
    rec = np.load(FIXTURE)
    assert np.array_equal(rec["x"], _case("norm_y", False)["calls"][0]["x"].numpy()), "the seeded case is not the one the fixture was recorded on"
    for kind, (causal, _) in KINDS.items():
        for mode in DF.DR.MODES:
            case = _case(mode, causal)
            extra = {}
            mine = DF.grads(case, torch.float64, "feats", extra)
            for k in _checked(case):
                r = torch.from_numpy(rec[f"{kind}__{mode}__{k}"])
                t = _digest(mine[k])
                m = float(r.abs().max())
                if k.endswith(KBIAS):
                    # projections of rounding noise on both sides: the magnitude is that of what cancels, summed as the projection sums it
                    m = extra[k] * mine[k].numel() ** 0.5
                    assert float(r.abs().max()) < 1e-12 * m, (kind, mode, k)
                else:
                    assert m > 0, (kind, mode, k)
                _close(t, r, m, (kind, mode, k))


def test_memory_modes_give_the_same_tokens():
    """The three memory modes are one function of the inputs: what the memory stores does not change the tokens of any call."""
    outs = {}
    for mode in DF.DR.MODES:
        case = _case(mode, False)
        p = {k: v.double() for k, v in case["params"].items()}
        with torch.no_grad():
            outs[mode] = [tok for tok, _ in DF.run(case, p, [c["x"].double() for c in case["calls"]])[0]]
    for mode in ("kv", "raw"):
        for a, b in zip(outs["norm_y"], outs[mode]):
            assert torch.allclose(a, b, rtol=0, atol=1e-12), (mode, float((a - b).abs().max()))


def test_additive_abi_21_symbols_signatures_and_descriptor():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION == 21
    for name in NEW:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == _lib.PROTOTYPES[name][0], name
    assert _lib.PROTOTYPES[NEW[0]] == (C.c_size_t, [C.c_int] * 3)
    for name in NEW[1:]:
        assert _lib.PROTOTYPES[name] == (C.c_int, [C.POINTER(_lib.FeedbackPrepareArgs), C.c_void_p, C.c_size_t])
    A = _lib.FeedbackPrepareArgs
    assert _lib.FEEDBACK_MAX_LAYERS == 32
    assert C.sizeof(A) == 8 * 32 * 8 + 2 * 8 + 6 * 4 + 8
    assert A.x.offset == 0 and A.gamma.offset == 256 and A.beta.offset == 512 and A.dy.offset == 768 and A.y.offset == 1024 and A.dx.offset == 1280
    assert A.dgamma.offset == 1536 and A.dbeta.offset == 1792 and A.offset.offset == 2048 and A.doffset.offset == 2056 and A.L.offset == 2064
    assert A.add_layers.offset == 2076 and A.eps.offset == 2080 and A.stream.offset == 2088
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        header = f.read()
    assert "#define MUST3R_HIP_ABI_VERSION 21" in header and "#define MUST3R_FEEDBACK_MAX_LAYERS 32" in header
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        decl = re.findall(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;{}]*)\)\s*;", plain)
        assert len(decl) == 1, name
        assert not re.search(r"void\*\s*stream\s*$", decl[0]), f"{name}: the stream travels in the descriptor"
    body = plain[plain.index("typedef struct must3r_hip_feedback_prepare_args {"):plain.index("} must3r_hip_feedback_prepare_args;")].split("{", 1)[1]
    assert re.search(r"void\*\s*stream;", body)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            names += [re.sub(r"\[.*\]", "", n).strip().lstrip("*").strip() for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", stmt, count=1).split(",")]
    assert names == [f[0] for f in A._fields_], names


def test_scratch_query_matches_the_documented_size():
    q = _lib.load().must3r_hip_feedback_prepare_scratch_bytes
    up = lambda v: (v + 255) // 256 * 256
    for L, R, D in ((1, 1, 64), (3, 70, 64), (12, 15360, 768), (32, 17, 1024), (2, 16, 128), (2, 17, 128)):
        assert q(L, R, D) == up(8 * L * ((R + 15) // 16) * D), (L, R, D)
    for bad in ((0, 10, 64), (33, 10, 64), (-1, 10, 64), (3, 0, 64), (3, -2, 64), (3, 10, 96), (3, 10, 0), (3, 10, 1088)):
        assert q(*bad) == 0, bad


FIELDS = ("x", "gamma", "beta", "dy", "y", "dx", "dgamma", "dbeta")


def _call(fn, L=3, nbytes=0, scratch=None, raw=False, **over):
    """A descriptor of fake but aligned addresses: every refusal comes before anything is read or launched."""
    lib = _lib.load()
    a = _lib.FeedbackPrepareArgs()
    for i, n in enumerate(FIELDS):
        if raw and n in ("gamma", "beta", "dgamma", "dbeta"):
            continue
        for l in range(max(L, 0) if L <= 32 else 32):
            getattr(a, n)[l] = 0x1000000 * (i + 1) + 0x1000 * l
    a.offset, a.doffset = C.c_void_p(0x7f000000), C.c_void_p(0x7e000000)
    a.L, a.R, a.D, a.add_layers, a.eps, a.stream = L, 10, 128, max(L - 1, 0), 1e-6, None
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    rc = getattr(lib, fn)(C.byref(a), scratch, nbytes)
    return rc, lib.must3r_hip_last_error().decode()


@pytest.mark.parametrize("raw", [False, True], ids=["norms", "raw"])
@pytest.mark.parametrize("fn", NEW[1:])
def test_feedback_prepare_refuses_before_touching_anything(fn, raw):
    lib = _lib.load()
    grad = fn.endswith("_grad")
    assert getattr(lib, fn)(None, None, 0) != 0 and "null" in lib.must3r_hip_last_error().decode()
    refusals = [(dict(D=96), "multiple of 64"), (dict(D=0), "multiple of 64"), (dict(D=1088), "1024"), (dict(D=2048), "1024"), (dict(L=0), "L must"),
                (dict(L=33), "L must"), (dict(L=-1), "L must"), (dict(R=0), "R must"), (dict(R=-4), "R must"), (dict(add_layers=4), "add_layers"),
                (dict(add_layers=-1), "add_layers"), (dict(offset=None), "offset"), (dict(x=(1, None)), "null"),
                (dict(x=(0, 0x1000008)), "aligned"), (dict(offset=C.c_void_p(0x7f000004)), "aligned"), (dict(doffset=C.c_void_p(0x7e000008)), "aligned"),
                (dict(dx=(2, 0x6000004)), "aligned"), (dict(y=(0, 0x5000008)), "aligned")]
    if grad:
        refusals += [(dict(dy=(2, None)), "null"), (dict(dy=(1, 0x4000004)), "aligned")]
    if raw:
        refusals += [(dict(gamma=(0, 0x2000000)), "come together"), (dict(gamma=(1, 0x2000000), beta=(1, 0x3000000)), "every layer or for none"),
                     (dict(dgamma=(0, 0x7000000)), "need gamma")]
    else:
        refusals += [(dict(gamma=(1, None)), "come together"), (dict(beta=(2, None)), "come together"),
                     (dict(gamma=(1, None), beta=(1, None), dgamma=(1, None), dbeta=(1, None)), "every layer or for none"),
                     (dict(gamma=(0, 0x2000004)), "aligned"), (dict(dbeta=(0, 0x8000008)), "aligned")]
    for over, word in refusals:
        rc, msg = _call(fn, raw=raw, **over)
        assert rc != 0 and word in msg, (over, msg)
    if grad and not raw:
        # everything else in order: the scratch of the column sums is what is missing
        need = lib.must3r_hip_feedback_prepare_scratch_bytes(3, 10, 128)
        assert need > 0
        for scratch, nbytes in ((None, 0), (C.c_void_p(0x9000000), need - 1), (C.c_void_p(0x9000008), need), (None, need)):
            rc, msg = _call(fn, scratch=scratch, nbytes=nbytes)
            assert rc != 0 and "scratch" in msg, msg


def _native(feedback_type, mode="norm_y"):
    import must3r_amd.model as M
    return M.MUSt3R(img_size=(224, 224), enc_embed_dim=128, embed_dim=128, depth=3, num_heads=2, feedback_type=feedback_type, memory_mode=mode)


@pytest.mark.parametrize("feedback_type", ["single_mlp", "single_linear", None])
def test_state_dict_keys_are_the_native_decoders(feedback_type):
    src = _native(feedback_type, "kv")
    with torch.no_grad():
        for p in src.parameters():
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.1)
    before = {k: v.clone() for k, v in src.state_dict().items()}
    for cls in (TD.MUSt3R, TD.CausalMUSt3R):
        dec = cls.from_decoder(src)
        assert list(dec.state_dict()) == list(src.state_dict()) == list(DF.param_names(3, feedback_type))
        assert [k for k, _ in dec.named_parameters()] == [k for k, _ in src.named_parameters()]
        assert all(v.dtype == torch.float32 for v in dec.state_dict().values())
        assert dec.memory_mode == "kv" and all(b.memory_mode == "kv" for b in dec.blocks_dec) and dec.feedback_type == feedback_type
        assert dec.depth == 3 and dec.attn_num_heads == 2 and dec.embed_dim == 128 and dec.enc_embed_dim == 128 and dec.feedback_eps == 1e-5
        assert cls.from_decoder(src, memory_mode="raw").memory_mode == "raw"
        for k, v in dec.state_dict().items():
            assert torch.equal(v, before[k]) and v.data_ptr() != src.state_dict()[k].data_ptr(), k
        # the way back: a fine-tuned model is served by the native decoder
        with torch.no_grad():
            dec.image2_embed.add_(1.0)
        dst = _native(feedback_type)
        dst.load_state_dict(dec.state_dict(), strict=True)
        assert torch.equal(dst.image2_embed, before["image2_embed"] + 1.0)
    assert all(torch.equal(v, before[k]) for k, v in src.state_dict().items())
    # a fresh module starts with an inactive feedback, as the reference's
    fresh = TD.MUSt3R(128, 64, 3, 1, feedback_type=feedback_type)
    if feedback_type == "single_mlp":
        assert not fresh.feedback_layer.fc2.weight.any() and not fresh.feedback_layer.fc2.bias.any() and fresh.feedback_layer.fc1.weight.any()
    elif feedback_type == "single_linear":
        assert not fresh.feedback_layer.weight.any() and not fresh.feedback_layer.bias.any()
    else:
        assert fresh.feedback_layer is None and fresh.feedback_norm is None


def test_freeze_and_memory_mode_follow_the_reference():
    dec = TD.MUSt3R(128, 64, 2, 1, feedback_type="single_mlp")
    dec.set_freeze("none")
    assert all(p.requires_grad for p in dec.parameters())
    dec.set_freeze("not_head")
    assert dec.freeze == "not_head"
    assert {k for k, p in dec.named_parameters() if p.requires_grad} == {"norm_dec.weight", "norm_dec.bias", "head_dec.proj.weight", "head_dec.proj.bias"}
    with pytest.raises(KeyError):
        dec.set_freeze("everything")
    dec.change_memory_mode("raw")
    assert dec.memory_mode == "raw" and all(b.memory_mode == "raw" for b in dec.blocks_dec)
    with pytest.raises(ValueError, match="memory_mode"):
        dec.change_memory_mode("keys")


def test_python_refusals():
    with pytest.raises(NotImplementedError, match="mem_dropout"):
        TD.CausalMUSt3R(mem_dropout=0.1, enc_embed_dim=128, embed_dim=64, depth=2, num_heads=1)
    with pytest.raises(ValueError, match="feedback_type"):
        TD.MUSt3R(128, 64, 2, 1, feedback_type="double_mlp")
    with pytest.raises(ValueError, match="memory_mode"):
        TD.MUSt3R(128, 64, 2, 1, memory_mode="keys")
    with pytest.raises(ValueError, match="depth"):
        TD.MUSt3R(128, 64, 33, 1)
    dec = TD.CausalMUSt3R(protected_imgs=1, enc_embed_dim=128, embed_dim=64, depth=2, num_heads=1, feedback_type="single_linear")
    x, pos, ts = torch.zeros(1, 2, 35, 128), torch.zeros(1, 2, 35, 2, dtype=torch.int64), torch.tensor([[[80, 112]] * 2])
    with pytest.raises(TypeError, match="list"):
        dec([x], [pos], [ts])
    with pytest.raises(RuntimeError, match="GPU"):
        dec(x, pos, ts)
    with pytest.raises(RuntimeError, match="GPU"):
        TD.feedback_prepare([torch.zeros(4, 64)] * 2, torch.zeros(4, 64), [torch.ones(64)] * 2, [torch.zeros(64)] * 2)
    with pytest.raises(RuntimeError, match="GPU"):
        TD.feedback_offset(torch.zeros(4, 64), torch.ones(64), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64))
    with pytest.raises(ValueError, match="layers"):
        TD.feedback_prepare([], None)
    # the tuple's tail (decoder.py:337 and :456-459)
    assert TD.MUSt3R._memory_tail(None, 5, 175, 0, 0, 2, 35) == (5, 175)
    assert dec._memory_tail(2, 70, 0, 0, 2, 35) == (1, 35) and dec._memory_tail(3, 105, 1, 35, 1, 35) == (1, 35)
