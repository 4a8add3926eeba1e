"""No GPU: the host side of the optimizer step (must3r_amd/train_optim.py, csrc/train_optim.hip) -- the additive ABI 21 surface, the scratch query, every refusal
of the two entry points on fake aligned addresses, the parameter groups against the reference's own function (live where its tree exists, from the recorded
fixture tests/golden/optim_groups.json everywhere), the learning-rate schedule, the state-dict layouts, and the error bound of the step itself: the fp32
emulation of the documented sequence is inside it and every planted defect is outside it by at least 100x (tests/optim_ref.py)."""
import contextlib
import ctypes as C
import importlib.util
import io
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import optim_cases as OC
import optim_ref as R
from conftest import GOLDEN, ROOT
from must3r_amd import _lib, train_optim as TO
from oracle.ref_shims import REFERENCE_ROOT

CHUNK = _lib.OPTIM_CHUNK
NAMES = ("must3r_hip_optim_scratch_bytes", "must3r_hip_optim_norm", "must3r_hip_optim_adamw")


def header():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        return f.read()


# -- ABI surface ------------------------------------------------------------------------------------
def test_abi_surface():
    h = header()
    assert "#define MUST3R_HIP_ABI_VERSION 21" in h and _lib.ABI_VERSION == 21
    assert re.search(r"#define MUST3R_OPTIM_CHUNK\s+(\d+)", h).group(1) == str(CHUNK) and CHUNK % 1024 == 0
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for n in NAMES:
        assert n in _lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, code)
        assert decl, n
        assert not re.search(r"void\*\s*stream\s*$", decl.group(1)), "the stream travels in the descriptor"
    i64, sz, i32, vp, P = C.c_int64, C.c_size_t, C.c_int, C.c_void_p, C.POINTER
    assert _lib.PROTOTYPES["must3r_hip_optim_scratch_bytes"] == (sz, [i64, i64])
    assert _lib.PROTOTYPES["must3r_hip_optim_norm"] == (i32, [P(_lib.OptimArgs), vp, sz])
    assert _lib.PROTOTYPES["must3r_hip_optim_adamw"] == (i32, [P(_lib.OptimArgs), vp, sz])
    assert "size_t must3r_hip_optim_scratch_bytes(int64_t n_tensors, int64_t total_elems);" in h
    assert "int must3r_hip_optim_norm(const must3r_hip_optim_args* a, void* scratch, size_t scratch_bytes);" in h
    assert "int must3r_hip_optim_adamw(const must3r_hip_optim_args* a, void* scratch, size_t scratch_bytes);" in h
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.must3r_hip_abi_version() == 21


def test_descriptor_layouts_are_pinned():
    T, G, K, A = _lib.OptimTensor, _lib.OptimGroup, _lib.OptimControl, _lib.OptimArgs
    assert C.sizeof(T) == 56 and [getattr(T, f).offset for f, _ in T._fields_] == [0, 8, 16, 24, 32, 40, 48, 52]
    assert C.sizeof(G) == 40 and [getattr(G, f).offset for f, _ in G._fields_] == [0, 8, 16, 24, 32]
    assert C.sizeof(K) == 16 and [getattr(K, f).offset for f, _ in K._fields_] == [0, 4, 8, 12]
    assert C.sizeof(A) == 72
    assert [(f, getattr(A, f).offset) for f, _ in A._fields_] == [
        ("tensors", 0), ("groups", 8), ("n_tensors", 16), ("n_groups", 20), ("control", 24), ("scale", 32), ("growth_tracker", 40),
        ("max_norm", 48), ("growth_factor", 52), ("backoff_factor", 56), ("growth_interval", 60), ("stream", 64)]
    # the header's field order is the binding's
    h = header()
    body = re.search(r"typedef struct must3r_hip_optim_args \{(.*?)\} must3r_hip_optim_args;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m for m in re.findall(r"[\s*,](\w+)\s*(?=[,;])", body)]
    assert fields == [f for f, _ in A._fields_], fields


# -- scratch query ----------------------------------------------------------------------------------
def up256(v):
    return (v + 255) // 256 * 256


def formula(n, total):
    c = total // CHUNK + n
    return up256(96 * n) + up256(16 * c) + up256(8 * c) + up256(8 * n)


def test_scratch_query():
    lib = _lib.load()
    for n, total in ((1, 1), (3, CHUNK + 1), (400, 130_000_000), (2, 3 * 2 ** 31)):
        assert lib.must3r_hip_optim_scratch_bytes(n, total) == formula(n, total), (n, total)
    for n, total, word in ((0, 1, "n_tensors"), (-1, 5, "n_tensors"), (3, 2, "total_elems"), (1, 0, "total_elems"), (1, 2 ** 47, "total_elems")):
        assert lib.must3r_hip_optim_scratch_bytes(n, total) == 0
        msg = lib.must3r_hip_last_error().decode()
        assert msg.startswith("optim_scratch_bytes: ") and word in msg, msg


# -- refusals ---------------------------------------------------------------------------------------
BASE = 0x7f0000000000


def fake_call(fn, *, n=2, tensors=None, groups=None, scratch=BASE + 0x100000, scratch_bytes=None, **fields):
    """A table of fake but aligned device addresses: every refusal comes before anything on the device is read or launched."""
    lib = _lib.load()
    tab = (_lib.OptimTensor * max(n, 1))()
    for i in range(max(n, 1)):
        t = tab[i]
        t.p, t.g, t.m, t.v, t.step = (BASE + 0x10000 * (5 * i + j) for j in range(5))
        t.n, t.group = 5 + i, i % 2
    for i, kw in (tensors or {}).items():
        for k, val in kw.items():
            setattr(tab[i], k, val)
    grp = (_lib.OptimGroup * 2)()
    for q in grp:
        q.lr, q.weight_decay, q.beta1, q.beta2, q.eps = 1e-3, 0.05, 0.9, 0.95, 1e-8
    for i, kw in (groups or {}).items():
        for k, val in kw.items():
            setattr(grp[i], k, val)
    a = _lib.OptimArgs()
    a.tensors, a.groups, a.n_tensors, a.n_groups = C.cast(tab, C.POINTER(_lib.OptimTensor)), C.cast(grp, C.POINTER(_lib.OptimGroup)), n, 2
    a.control = BASE + 0x200000
    a.growth_factor, a.backoff_factor, a.growth_interval = 2.0, 0.5, 2000
    for k, val in fields.items():
        setattr(a, k, val)
    if scratch_bytes is None:
        scratch_bytes = formula(max(n, 1), sum(tab[i].n for i in range(max(n, 1))) if all(tab[i].n > 0 for i in range(max(n, 1))) else 1)
    rc = getattr(lib, fn)(C.byref(a), C.c_void_p(scratch), scratch_bytes)
    return rc, lib.must3r_hip_last_error().decode()


BOTH = [
    (dict(n=0), "n_tensors"),
    (dict(tensors={1: dict(g=None)}), "null"),
    (dict(tensors={0: dict(g=BASE + 8)}), "aligned"),
    (dict(tensors={1: dict(n=0)}), "positive"),
    (dict(tensors={0: dict(n=-4)}), "positive"),
    (dict(control=BASE + 0x200004), "aligned"),
    (dict(scratch=None), "scratch"),
    (dict(scratch=BASE + 0x100008), "scratch"),
    (dict(scratch_bytes=formula(2, 11) - 1), "scratch too small"),
]
NORM_ONLY = [
    (dict(control=None), "control"),
    (dict(scale=BASE + 0x300000), "come together"),
    (dict(growth_tracker=BASE + 0x300000), "come together"),
    (dict(scale=BASE + 0x300000, growth_tracker=BASE + 0x300010, growth_interval=0), "growth_interval"),
    (dict(scale=BASE + 0x300000, growth_tracker=BASE + 0x300010, backoff_factor=0.0), "backoff_factor"),
    (dict(max_norm=float("nan")), "max_norm"),
]
ADAMW_ONLY = [
    (dict(tensors={0: dict(p=None)}), "null"),
    (dict(tensors={0: dict(m=None)}), "null"),
    (dict(tensors={1: dict(v=None)}), "null"),
    (dict(tensors={1: dict(step=None)}), "null"),
    (dict(tensors={0: dict(p=BASE + 4)}), "aligned"),
    (dict(tensors={0: dict(m=BASE + 0x10008)}), "aligned"),
    (dict(tensors={1: dict(v=BASE + 0x1000c)}), "aligned"),
    (dict(tensors={1: dict(group=2)}), "group index"),
    (dict(tensors={0: dict(group=-1)}), "group index"),
    (dict(groups={0: dict(beta1=1.0)}), "beta"),
    (dict(groups={1: dict(beta2=-0.1)}), "beta"),
    (dict(groups={1: dict(beta2=float("nan"))}), "beta"),
    (dict(groups={0: dict(eps=-1e-8)}), "eps"),
    (dict(groups={0: dict(lr=-1e-3)}), "lr"),
    (dict(groups={1: dict(weight_decay=-0.1)}), "weight_decay"),
    (dict(n_groups=0), "n_groups"),
]


@pytest.mark.parametrize("fn,kw,word", [(f, kw, w) for f in ("must3r_hip_optim_norm", "must3r_hip_optim_adamw") for kw, w in BOTH]
                         + [("must3r_hip_optim_norm", kw, w) for kw, w in NORM_ONLY] + [("must3r_hip_optim_adamw", kw, w) for kw, w in ADAMW_ONLY])
def test_refusals(fn, kw, word):
    rc, msg = fake_call(fn, **kw)
    assert rc != 0 and msg.startswith(fn[len("must3r_hip_"):] + ": ") and word in msg, (rc, msg)


def test_null_descriptor_and_tables_are_refused():
    lib = _lib.load()
    for fn in ("must3r_hip_optim_norm", "must3r_hip_optim_adamw"):
        assert getattr(lib, fn)(None, None, 0) != 0 and "null" in lib.must3r_hip_last_error().decode()
        a = _lib.OptimArgs()
        a.n_tensors, a.n_groups, a.control = 1, 1, BASE
        assert getattr(lib, fn)(C.byref(a), C.c_void_p(BASE), 1 << 20) != 0 and "tensors" in lib.must3r_hip_last_error().decode()


# -- parameter groups -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def group_models():
    return OC.models()


def test_parameter_groups_match_the_recorded_reference(group_models):
    with open(os.path.join(GOLDEN, "optim_groups.json")) as f:
        want = json.load(f)
    cases = OC.cases(*group_models)
    assert set(want) == set(cases)
    for name, c in cases.items():
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            got = OC.record(TO.get_parameter_groups, *c)
        assert got == want[name], name
        assert out.getvalue() == "", "the port does not print the groups"
    assert "raises" in want["decoder_0.75"] and len(want["encoder_0.75"]["groups"]) > 2
    assert any(g["lr_scale"] == 1.0 for g in want["encoder_0.75"]["groups"]) and any(g["lr_scale"] == 0.75 ** 3 for g in want["encoder_0.75"]["groups"])
    frozen = [n for n, p in group_models[0].named_parameters() if not p.requires_grad]
    assert frozen and not any(n in g["params"] for n in frozen for g in want["encoder_1.0"]["groups"])


REF_OPTIMIZER = os.path.join(REFERENCE_ROOT, "must3r", "engine", "optimizer.py")


@pytest.mark.skipif(not os.path.isfile(REF_OPTIMIZER), reason="the reference tree is not on this machine")
def test_parameter_groups_match_the_reference_live(group_models):
    spec = importlib.util.spec_from_file_location("ref_engine_optimizer", REF_OPTIMIZER)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for name, c in OC.cases(*group_models).items():
        with contextlib.redirect_stdout(io.StringIO()):
            want = OC.record(ref.get_parameter_groups, *c)
        assert OC.record(TO.get_parameter_groups, *c) == want, name


# -- learning-rate schedule -------------------------------------------------------------------------
class FakeOptimizer:
    def __init__(self, groups):
        self.param_groups = groups


def test_adjust_learning_rate():
    args = types.SimpleNamespace(lr=2e-4, min_lr=1e-6, warmup_epochs=4, epochs=20)

    def want(e):
        if e < 4:
            return 2e-4 * e / 4
        return 1e-6 + (2e-4 - 1e-6) * 0.5 * (1 + math.cos(math.pi * (e - 4) / 16))

    for e, fixed in ((0, 0.0), (1.5, 0.75e-4), (4, 2e-4), (12, 1e-6 + 0.5 * (2e-4 - 1e-6)), (20, 1e-6), (7.25, None)):
        opt = FakeOptimizer([dict(lr=1.0), dict(lr=1.0, lr_scale=0.75 ** 3), dict(lr=1.0, lr_scale=1.0)])
        lr = TO.adjust_learning_rate(opt, e, args)
        assert lr == pytest.approx(want(e), rel=1e-15, abs=0)
        if fixed is not None:
            assert lr == pytest.approx(fixed, rel=1e-12, abs=1e-20)
        assert [g["lr"] for g in opt.param_groups] == [lr, lr * 0.75 ** 3, lr]
        assert "lr_scale" not in opt.param_groups[0]


# -- state dicts ------------------------------------------------------------------------------------
SHAPES = ((5, 3), (7,), (1,), (4, 4))


def make_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def torch_adamw_after_steps(params, steps=2):
    opt = torch.optim.AdamW([dict(params=params[:2], weight_decay=0.05, lr_scale=0.5), dict(params=params[2:], weight_decay=0.0)], lr=1e-3, betas=(0.9, 0.95))
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_state_dict_layout_is_torch_adamws():
    ref = torch_adamw_after_steps(make_params())
    sd = ref.state_dict()
    mine = TO.AdamW([dict(params=make_params()[:2], weight_decay=0.05, lr_scale=0.5), dict(params=make_params()[2:], weight_decay=0.0)], lr=1e-3,
                    betas=(0.9, 0.95))
    assert mine.state_dict()["state"] == {} and len(mine.state_dict()["param_groups"]) == 2       # lazily, as torch
    mine.load_state_dict(sd)
    got = mine.state_dict()
    assert set(got) == set(sd) and got["param_groups"] == sd["param_groups"]
    assert list(got["state"]) == list(sd["state"])
    for i, st in sd["state"].items():
        assert list(got["state"][i]) == list(st) == ["step", "exp_avg", "exp_avg_sq"]
        for k in st:
            assert got["state"][i][k].shape == st[k].shape and got["state"][i][k].dtype == st[k].dtype == torch.float32
            assert torch.equal(got["state"][i][k].cpu(), st[k].cpu()), (i, k)
    # the moments are views of two flat buffers, the steps of a third
    L = mine._layout
    for (m, v, s), p in zip(L["views"], L["params"]):
        assert mine.state[p]["exp_avg"] is m and m.untyped_storage().data_ptr() == L["m"].untyped_storage().data_ptr()
        assert v.untyped_storage().data_ptr() == L["v"].untyped_storage().data_ptr() and m.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
        assert s.ndim == 0 and s.untyped_storage().data_ptr() == L["steps"].untyped_storage().data_ptr()
    # and back into torch: a checkpoint written by either side resumes on the other
    back = torch.optim.AdamW([dict(params=make_params()[:2]), dict(params=make_params()[2:])])
    back.load_state_dict(got)
    for a, b in zip(back.state_dict()["state"].values(), sd["state"].values()):
        assert all(torch.equal(a[k], b[k]) for k in b)


def test_state_dict_with_a_number_or_device_step_loads():
    sd = torch_adamw_after_steps(make_params()).state_dict()
    for i in sd["state"]:
        sd["state"][i]["step"] = 2.0 if i % 2 else torch.tensor(2.0, dtype=torch.float64)
    mine = TO.AdamW([dict(params=make_params()[:2]), dict(params=make_params()[2:])])
    mine.load_state_dict(sd)
    assert all(float(st["step"]) == 2.0 and st["step"].dtype == torch.float32 and st["step"].ndim == 0 for st in mine.state.values())


def test_unsupported_forms_raise():
    ps = make_params()
    with pytest.raises(NotImplementedError):
        TO.AdamW(ps, amsgrad=True)
    with pytest.raises(NotImplementedError):
        TO.AdamW(ps, maximize=True)
    with pytest.raises(TypeError):
        TO.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(TypeError):
        TO.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    opt = TO.AdamW(ps)
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.grad_norm()
    with pytest.raises(TypeError, match="AdamW"):
        TO.LossScaler()(torch.zeros((), requires_grad=True), torch.optim.AdamW(ps))
    sd = torch.optim.AdamW(make_params(), amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(sd)


def test_loss_scaler_state_dict_has_gradscalers_keys():
    s = TO.LossScaler()
    sd = s.state_dict()
    assert sd == {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 0}
    assert list(sd) == ["scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"]
    t = TO.LossScaler()
    t.load_state_dict({"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 100, "_growth_tracker": 7})
    assert t.state_dict() == {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 100, "_growth_tracker": 7}
    off = TO.LossScaler(enabled=False)
    assert off.state_dict() == {}
    off.load_state_dict({})
    with pytest.raises(RuntimeError):
        t.load_state_dict({})


def test_save_and_load_model_use_the_references_keys(tmp_path):
    enc, dec = torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)
    opt, sc = TO.AdamW(dec.parameters(), lr=1e-3), TO.LossScaler()
    args = types.SimpleNamespace(output_dir=str(tmp_path))
    path = TO.save_model(args, 4, enc, dec, opt, sc, "last")
    assert os.path.basename(path) == "checkpoint-last.pth" and os.path.basename(TO.save_model(args, 4, enc, dec, opt, sc)) == "checkpoint-4.pth"
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck) == ["encoder", "decoder", "optimizer", "scaler", "args", "epoch"] and ck["epoch"] == 4
    # a checkpoint as the reference writes it: torch's optimizer, GradScaler's state
    ref_opt = torch.optim.AdamW(dec.parameters(), lr=5e-4, betas=(0.9, 0.95))
    for p in dec.parameters():
        p.grad = torch.ones_like(p)
    ref_opt.step()
    torch.save({"encoder": enc.state_dict(), "decoder": dec.state_dict(), "optimizer": ref_opt.state_dict(),
                "scaler": {"scale": 512.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 3}, "args": None, "epoch": 9},
               tmp_path / "ref.pth")
    enc2, dec2 = torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)
    opt2, sc2 = TO.AdamW(dec2.parameters(), lr=1e-3), TO.LossScaler()
    TO.load_model(args, str(tmp_path / "ref.pth"), enc2, dec2, opt2, sc2)
    assert args.start_epoch == 10 and opt2.param_groups[0]["lr"] == 5e-4 and opt2.param_groups[0]["betas"] == (0.9, 0.95)
    assert sc2.state_dict()["scale"] == 512.0 and sc2.state_dict()["_growth_tracker"] == 3
    assert all(torch.equal(a, b) for a, b in zip(dec2.state_dict().values(), dec.state_dict().values()))
    for p, q in zip(dec2.parameters(), dec.parameters()):
        assert torch.equal(opt2.state[p]["exp_avg"], ref_opt.state[q]["exp_avg"]) and float(opt2.state[p]["step"]) == 1.0
    TO.load_model(args, None, enc2, dec2, opt2, sc2)
    assert args.start_epoch == 0


# -- the bound itself -------------------------------------------------------------------------------
def test_the_emulation_is_inside_the_bound_and_every_defect_far_outside():
    """|g| log-uniform in 1e-9 .. 1e-1 times the scale 65536, lr 1e-3, wd 0.05, betas (0.9, 0.95), an active clip; three steps, each judged from equal
    states (the yardstick's, rounded).  Measured on these inputs: the emulation at 0.15 of the bound (4.2 u against K = 28), the defects at 3.8e5 and above."""
    assert R.K <= 32
    rng = np.random.default_rng(0)
    N, scale = 200_000, 65536.0
    grp = dict(lr=1e-3, weight_decay=0.05, betas=(0.9, 0.95), eps=1e-8)
    state = dict(p=torch.tensor(rng.standard_normal(N) * 0.02, dtype=torch.float32), m=torch.zeros(N), v=torch.zeros(N), step=0, group=0)
    for it in range(3):
        g = torch.tensor((10 ** rng.uniform(-9, -1, N)) * rng.choice([-1.0, 1.0], N) * scale, dtype=torch.float32)
        total = float((g.double() ** 2).sum())
        max_norm = 0.5 * math.sqrt(total) / scale
        out, norm, found_inf = R.yardstick_step([state], [g], [grp], scale, max_norm)
        assert not found_inf and out[0]["step"] == it + 1
        n32, _, inv_scale, clip = R.coef32(total, scale, max_norm)
        assert abs(float(n32) - norm) <= 2 * R.U * norm and 0.49 < float(clip) < 0.51
        ratios = {}
        for d in (None,) + R.DEFECTS:
            p, m, v = R.emulate32(state["p"].numpy(), g.numpy(), state["m"].numpy(), state["v"].numpy(), state["step"], grp, inv_scale, clip, d)
            ratios[d] = R.bound_ratio(out[0], p, m, v)
        print(f"step {it + 1}: error / bound = " + ", ".join(f"{k}: {v:.3g}" for k, v in ratios.items()))
        assert ratios[None] <= 1.0, ratios
        assert all(ratios[d] >= 100.0 for d in R.DEFECTS), ratios
        state = dict(R.rounded(out[0]), group=0)


def test_the_yardstick_restates_gradscaler():
    assert R.scaler_update(65536.0, 5, True) == (32768.0, 0)
    assert R.scaler_update(65536.0, 0, False, growth_interval=2) == (65536.0, 1)
    assert R.scaler_update(65536.0, 1, False, growth_interval=2) == (131072.0, 0)
    t = dict(p=torch.ones(4), m=torch.zeros(4), v=torch.zeros(4), step=3, group=0)
    out, norm, found_inf = R.yardstick_step([t], [torch.tensor([1.0, float("inf"), 0.0, 0.0])], [dict(lr=1e-3, weight_decay=0.0, betas=(0.9, 0.95), eps=1e-8)], 2.0)
    assert found_inf and math.isnan(norm) and torch.equal(out[0]["p"], t["p"].double()) and out[0]["step"] == 3
