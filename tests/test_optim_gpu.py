"""GPU (-m gpu): the optimizer step -- must3r_amd/train_optim.py on csrc/train_optim.hip (must3r_hip_optim_norm / must3r_hip_optim_adamw) -- against the fp64
yardstick tests/optim_ref.py (torch.optim.AdamW(foreach=False), clip_grad_norm_ and GradScaler's rule) under the bound derived there (K roundings of 2^-24,
counted in optim_ref.bound_ratio): the step over every tail and chunk form, the norm, non-finite gradients, missing gradients, guard zones, repeatability, the
version counters the native modules watch, the stream, and six iterations of the reference's loop on the tiny decoder with a resume in the middle."""
import math
import time
import types

import pytest
import torch

import decoder_ref as DF
import metrics_ref as MR
import optim_ref as R
from must3r_amd import _lib, train_decoder as TD, train_losses as TL, train_optim as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = _lib.OPTIM_CHUNK
NS = (1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, (768, 768))
ODD = (1, 3, 5, 63, 65, CHUNK - 1, CHUNK + 1)
GROUPS = (dict(lr=1e-3, weight_decay=0.05, betas=(0.9, 0.95), eps=1e-8), dict(lr=3e-4, weight_decay=0.0, betas=(0.9, 0.95), eps=1e-8))
GUARD, SENTINEL = 64, 12345.0


def bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


class Rig:
    """Parameters and the optimizer's flat state buffers inside guard zones; tensor i belongs to group i % 2."""

    def __init__(self, shapes, monkeypatch, groups=GROUPS, seed=0):
        self.shapes = [s if isinstance(s, tuple) else (s,) for s in shapes]
        self.guarded = []
        g = torch.Generator().manual_seed(seed)
        self.p0 = [torch.randn(s, generator=g) * 0.02 for s in self.shapes]
        self.params = [torch.nn.Parameter(self.inside(math.prod(s)).view(s)) for s in self.shapes]
        for p, v in zip(self.params, self.p0):
            p.data.copy_(v)
        monkeypatch.setattr(TO, "_flat", lambda numel, device, dtype=torch.float32: self.inside(numel))
        self.groups = [dict(groups[k], params=self.params[k::2]) for k in range(2) if self.params[k::2]]
        self.opt = TO.AdamW(self.groups, lr=1.0)
        self.order = [p for g in self.groups for p in g["params"]]          # the optimizer's table order
        ids = [id(p) for p in self.order]
        self.index = [ids.index(id(p)) for p in self.params]
        self.L = self.opt._ensure_layout()

    def inside(self, numel):
        big = torch.full((numel + 2 * GUARD,), SENTINEL, device=DEV)
        self.guarded.append((big, numel))
        inner = big[GUARD:GUARD + numel]
        inner.zero_()
        assert inner.data_ptr() % 16 == 0
        return inner

    def guards_intact(self):
        return all(bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + n:] == SENTINEL).all()) for big, n in self.guarded)

    def views(self, i):
        return self.L["views"][self.index[i]]

    def set_state(self, states):
        with torch.no_grad():
            for i, st in enumerate(states):
                m, v, step = self.views(i)
                self.params[i].data.copy_(st["p"])
                m.copy_(st["m"])
                v.copy_(st["v"])
                step.fill_(float(st["step"]))

    def set_grads(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else g.to(DEV).view(p.shape).clone()

    def read(self):
        out = []
        for i, p in enumerate(self.params):
            m, v, step = self.views(i)
            out.append(dict(p=p.detach().cpu().clone(), m=m.cpu().clone(), v=v.cpu().clone(), step=float(step)))
        return out

    def state_bits(self):
        return [torch.cat([bits(p).view(-1), bits(self.views(i)[0]).view(-1), bits(self.views(i)[1]).view(-1), bits(self.views(i)[2]).view(-1)])
                for i, p in enumerate(self.params)]

    def start(self):
        return [dict(p=p.clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), step=0, group=i % 2) for i, p in enumerate(self.p0)]


def make_grads(shapes, seed, scale=1.0):
    """|g| log-uniform in 1e-7 .. 1e-2, random signs, times the loss scale"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in shapes:
        mag = 10 ** (torch.rand(s, generator=g) * 5 - 7)
        out.append((mag * (torch.randint(0, 2, s, generator=g) * 2 - 1) * scale).float())
    return out


def check_step(tag, got, want):
    worst = 0.0
    for i, (a, y) in enumerate(zip(got, want)):
        assert a["step"] == y["step"], (tag, i, a["step"], y["step"])
        if "p0" not in y:                                  # not updated: bit-equal to the start
            assert torch.equal(a["p"].double(), y["p"]) and torch.equal(a["m"].double(), y["m"]) and torch.equal(a["v"].double(), y["v"]), (tag, i)
            continue
        r = R.bound_ratio(y, a["p"], a["m"], a["v"])
        worst = max(worst, r)
        assert r <= 1.0, f"{tag}: tensor {i} of {tuple(y['p'].shape)} at {r:.3f} of the bound (K = {R.K})"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the step and the norm against the yardstick
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("control", [False, True], ids=["plain", "scaled_clipped"])
def test_step_matches_the_yardstick(control, monkeypatch):
    rig = Rig(NS, monkeypatch)
    scale = 65536.0 if control else None
    scaler = TO.LossScaler() if control else None
    state = rig.start()
    for k in range(3):
        grads = make_grads(rig.shapes, 10 + k, scale or 1.0)
        total = sum(float((g.double() ** 2).sum()) for g in grads)
        norm64 = math.sqrt(total) / (scale or 1.0)
        max_norm = 0.5 * norm64 if control else None
        want, norm, found_inf = R.yardstick_step(state, grads, GROUPS, scale, max_norm)
        assert not found_inf and abs(norm - norm64) <= 1e-12 * norm64
        rig.set_state(state)
        rig.set_grads(grads)
        before = [bits(p.grad) for p in rig.params]
        if control:
            rec = rig.opt.grad_norm(max_norm=max_norm, scaler=scaler)
            rig.opt.step(control=rec)
            got_norm, coef, flag = float(rec[0]), float(rec[1]), int(rec.view(torch.int32)[2])
            want_coef = R.coef32(total, scale, max_norm)[1]
            print(f"step {k + 1}: norm {got_norm:.9g} (fp64 {norm64:.9g}), coef {coef:.9g} (fp32 emulation {float(want_coef):.9g})")
            assert abs(got_norm - norm64) <= 2 * R.U * norm64 and flag == 0
            assert abs(coef - float(want_coef)) <= 4 * R.U * float(want_coef) and 0.49 / scale < coef < 0.51 / scale
        else:
            rig.opt.step()
        worst = check_step(f"step {k + 1}", rig.read(), want)
        print(f"step {k + 1} ({'control' if control else 'plain'}): worst error / bound = {worst:.3f}")
        assert all(torch.equal(bits(p.grad), b) for p, b in zip(rig.params, before)), "g is never written"
        assert rig.guards_intact()
        state = [dict(R.rounded(y), group=i % 2) for i, y in enumerate(want)]
    if control:
        assert float(scaler._scale) == 65536.0 and int(scaler._tracker) == 3


def test_norm_of_the_table_and_of_400_small_tensors(monkeypatch):
    rig = Rig(NS, monkeypatch)
    grads = make_grads(rig.shapes, 31)
    rig.set_grads(grads)
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    rec = rig.opt.grad_norm()
    assert abs(float(rec[0]) - want) <= 2 * R.U * want and float(rec[1]) == 1.0 and int(rec.view(torch.int32)[2]) == 0
    # 400 tensors of 7 elements: the table loops of the one-block kernels wrap (256 threads)
    g = torch.Generator().manual_seed(5)
    p0 = [torch.randn(7, generator=g) * 0.02 for _ in range(400)]
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    grads = make_grads([(7,)] * 400, 32)
    for p, gr in zip(params, grads):
        p.grad = gr.to(DEV)
    opt = TO.AdamW(params, lr=GROUPS[0]["lr"], betas=GROUPS[0]["betas"], weight_decay=GROUPS[0]["weight_decay"])
    want = math.sqrt(sum(float((gr.double() ** 2).sum()) for gr in grads))
    rec = opt.grad_norm(max_norm=10 * want)
    assert abs(float(rec[0]) - want) <= 2 * R.U * want and float(rec[1]) == 1.0
    opt.step(control=rec)
    state = [dict(p=p, m=torch.zeros(7), v=torch.zeros(7), step=0, group=0) for p in p0]
    ys, _, _ = R.yardstick_step(state, grads, GROUPS[:1])
    got = [dict(p=p.detach().cpu(), m=opt.state[p]["exp_avg"].cpu(), v=opt.state[p]["exp_avg_sq"].cpu(), step=float(opt.state[p]["step"])) for p in params]
    check_step("400 x 7", got, ys)


# ---------------------------------------------------------------------------------------------------------------------------------
# non-finite gradients, missing gradients
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["nan_last", "inf_first"])
def test_a_non_finite_gradient_skips_the_step_and_halves_the_scale(where, monkeypatch):
    rig = Rig((5, 1, CHUNK + 1, 65), monkeypatch)
    scaler = TO.LossScaler(growth_interval=2)
    rig.set_grads(make_grads(rig.shapes, 41, 65536.0))
    rig.opt.step(control=rig.opt.grad_norm(scaler=scaler))              # a clean step: moments and step counts are not zero
    assert float(scaler._scale) == 65536.0 and int(scaler._tracker) == 1
    grads = make_grads(rig.shapes, 42, 65536.0)
    # the table order: group 0 holds tensors 0 and 2, group 1 tensors 1 and 3
    if where == "nan_last":
        grads[3][-1] = float("nan")
    else:
        grads[0][0] = float("inf")
    rig.set_grads(grads)
    assert rig.order[0] is rig.params[0] and rig.order[-1] is rig.params[3]
    before = rig.state_bits()
    rec = rig.opt.grad_norm(max_norm=1.0, scaler=scaler)
    rig.opt.step(control=rec)
    assert all(torch.equal(a, b) for a, b in zip(rig.state_bits(), before)), "every p, m, v and step is bit-unchanged"
    assert not math.isfinite(float(rec[0])) and int(rec.view(torch.int32)[2]) == 1
    assert float(scaler._scale) == 32768.0 and int(scaler._tracker) == 0
    assert all(float(rig.views(i)[2]) == 1.0 for i in range(4)) and rig.guards_intact()
    # two clean steps at growth_interval 2 double the scale
    for k in range(2):
        rig.set_grads(make_grads(rig.shapes, 43 + k, 32768.0))
        rec = rig.opt.grad_norm(scaler=scaler)
        rig.opt.step(control=rec)
        assert math.isfinite(float(rec[0])) and int(scaler._tracker) == (1, 0)[k]
    assert float(scaler._scale) == 65536.0
    assert all(float(rig.views(i)[2]) == 3.0 for i in range(4))
    assert not any(torch.equal(a, b) for a, b in zip(rig.state_bits(), before))


def test_a_parameter_without_a_gradient_is_left_alone(monkeypatch):
    rig = Rig((65, 5, CHUNK + 1, 7, 64), monkeypatch)
    grads = make_grads(rig.shapes, 51)
    grads[2] = None
    grads[3] = None
    state = rig.start()
    rig.set_grads(grads)
    before, versions = rig.state_bits(), [p._version for p in rig.params]
    want, _, _ = R.yardstick_step(state, grads, GROUPS)
    rig.opt.step()
    after = rig.state_bits()
    for i in range(5):
        if grads[i] is None:
            assert torch.equal(after[i], before[i]) and rig.params[i]._version == versions[i] and len(rig.opt.state[rig.params[i]]) == 0
        else:
            assert not torch.equal(after[i], before[i]) and rig.params[i]._version > versions[i]
            assert list(rig.opt.state[rig.params[i]]) == ["step", "exp_avg", "exp_avg_sq"]
    check_step("grad None", rig.read(), want)
    assert rig.guards_intact()
    # the gradients come back: the table is whole again
    rig.set_grads(make_grads(rig.shapes, 52))
    rig.opt.step()
    assert [float(rig.views(i)[2]) for i in range(5)] == [2.0, 2.0, 1.0, 1.0, 2.0] and rig.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds, repeatability
# ---------------------------------------------------------------------------------------------------------------------------------
def test_guards_stay_intact_on_odd_lengths_and_g_is_not_written(monkeypatch):
    rig = Rig(ODD, monkeypatch)
    scaler = TO.LossScaler()
    for k in range(2):
        rig.set_grads(make_grads(rig.shapes, 61 + k, 65536.0))
        before = [bits(p.grad) for p in rig.params]
        rec = rig.opt.grad_norm(max_norm=1e-4, scaler=scaler)
        rig.opt.step(control=rec)
        rig.opt.step()                                      # and a plain step
        assert rig.guards_intact()
        assert all(torch.equal(bits(p.grad), b) for p, b in zip(rig.params, before))
        assert float(rec[1]) < 1.0 / 65536.0
    assert all(float(rig.views(i)[2]) == 4.0 for i in range(len(ODD)))


def test_repeats_bitwise_and_does_not_depend_on_the_rest_of_the_table(monkeypatch):
    shapes = (65, CHUNK + 1, 5, (96, 64), 3, 2 * CHUNK + 3)
    grads = make_grads([s if isinstance(s, tuple) else (s,) for s in shapes], 71)
    rec = torch.tensor([1.0, 0.37, 0.0, 0.0], device=DEV)      # a control record by hand: the same coefficient whatever the table holds

    def run(order, extra=0):
        rig = Rig([shapes[i] for i in order] + [33] * extra, monkeypatch)
        with torch.no_grad():
            for j, i in enumerate(order):
                rig.params[j].copy_(torch.full(rig.shapes[j], 0.01 * (i + 1)))
        rig.set_grads([grads[i] for i in order] + make_grads([(33,)] * extra, 72))
        norms = []
        for _ in range(2):
            norms.append(bits(rig.opt.grad_norm()[:1]))
            rig.opt.step(control=rec)
        state = rig.state_bits()
        # the parity of the position picks the group: compare tensors that keep theirs
        return {i: state[j] for j, i in enumerate(order)}, norms
    a, na = run(range(6))
    b, nb = run(range(6))
    assert all(torch.equal(a[i], b[i]) for i in range(6)) and all(torch.equal(x, y) for x, y in zip(na, nb)), "two runs from equal state"
    c, _ = run([4, 5, 2, 3, 0, 1], extra=3)                # another order (every tensor keeps its group), more tensors
    assert all(torch.equal(a[i], c[i]) for i in range(6)), [i for i in range(6) if not torch.equal(a[i], c[i])]


# ---------------------------------------------------------------------------------------------------------------------------------
# version counters: a native module whose parameters are stepped serves the new weights
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_step_moves_the_version_counters_the_native_decoder_watches():
    import must3r_amd.model as M
    from must3r_amd import synthetic as S
    from must3r_amd.config import SMALL as cfg
    from must3r_amd.engine import run_scene
    enc = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads)
    dec = M.MUSt3R(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth, num_heads=cfg.dec_heads,
                   feedback_type="single_mlp", memory_mode="kv")
    enc.load_state_dict(S.make_encoder_state_dict(cfg, 0))
    dec.load_state_dict(S.make_decoder_state_dict(cfg, 0))
    enc, dec = enc.to(DEV).eval(), dec.to(DEV).eval()
    imgs, ts = S.make_images(2, 224, 224, 0)
    imgs, ts = imgs.to(DEV), ts.to(DEV)
    first = run_scene(enc, dec, imgs, ts)["render"].clone()
    assert torch.equal(run_scene(enc, dec, imgs, ts)["render"], first)
    params = [p for p in dec.parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    versions = [p._version for p in params]
    opt = TO.AdamW(params, lr=1e-2, betas=(0.9, 0.95))
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions))
    second = run_scene(enc, dec, imgs, ts)["render"]
    assert bool(torch.isfinite(second).all()) and not torch.equal(second, first), "the native decoder kept serving the weights from before the step"


# ---------------------------------------------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------------------------------------------
def test_both_entry_points_run_on_the_descriptors_stream(monkeypatch):
    """The protocol of tests/test_decoder_grad_gpu.py::test_both_entry_points_run_on_the_descriptors_stream: reference bits of two input sets A and B on the
    default stream; then, with the buffers holding B, on a side stream the null stream overtakes: a delay, copies of A, the calls, clones of the outputs, B
    back.  The clones must be A's bits and the delay must still be running when the calls have returned.  Control: with the stream forced to NULL the same
    calls reproduce B's bits."""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay, null_stream
    delay = Delay()
    rig = Rig((65, CHUNK + 1, 5, (96, 64)), monkeypatch)
    scaler = TO.LossScaler(growth_interval=3)
    scale, tracker = scaler._state(torch.device(DEV, torch.cuda.current_device()))
    shapes = rig.shapes

    def source(seed):
        g = torch.Generator().manual_seed(seed)
        out = {}
        for i, s in enumerate(shapes):
            out[f"p{i}"] = torch.randn(s, generator=g) * 0.02
            out[f"g{i}"] = make_grads([s], seed + i, 65536.0)[0]
            out[f"m{i}"] = torch.randn(s, generator=g) * 1e-4
            out[f"v{i}"] = torch.rand(s, generator=g) * 1e-8 + 1e-10
            out[f"step{i}"] = torch.tensor(float(3 + seed % 5 + i))
        out["scale"] = torch.tensor([65536.0 if seed % 2 else 16384.0])
        return {k: v.to(DEV) for k, v in out.items()}
    src = {"A": source(81), "B": source(92)}
    bufs = {"scale": scale}
    for i, p in enumerate(rig.params):
        p.grad = torch.empty_like(p)
        m, v, step = rig.views(i)
        bufs.update({f"p{i}": p.data, f"g{i}": p.grad, f"m{i}": m, f"v{i}": v, f"step{i}": step})

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
        tracker.fill_(2)

    def call():
        rec = rig.opt.grad_norm(max_norm=1e-3, scaler=scaler)
        rig.opt.step(control=rec)
        return [bufs[k] for k in sorted(bufs)] + [rec, tracker]
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = call()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        ref[which] = [t.clone() for t in outs]
    assert float(ref["A"][sorted(bufs).index("scale")]) == 131072.0 and int(ref["A"][-1]) == 0       # the scaler update ran: 65536 x 2 at the interval
    assert not torch.equal(ref["A"][0], ref["B"][0])
    ms = min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)
    assert ms < DELAY_CAP_MS or host_ms < DELAY_CAP_MS / 10
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")
        t0 = time.perf_counter()
        outs = call()
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in outs]
        load("B")
    s.synchronize()
    print(f"optim: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the calls took {side_ms:.3f} ms on the host)"
    for i, (g, r) in enumerate(zip(got, ref["A"])):
        assert torch.equal(g, r), f"output {i}: on a side stream the bits differ from the default-stream bits (equal to the decoy's: {torch.equal(g, ref['B'][i])})"
    # the control: the stream forced to NULL reads the decoy
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")                         # queued behind the delay: the buffers still hold the decoy
        with null_stream():
            outs = call()
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.cuda.default_stream().synchronize()
            got = [t.clone() for t in outs]
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"the delay ({ms:.1f} ms) ended before the null stream was idle"
    for i, (g, r) in enumerate(zip(got, ref["B"])):
        assert torch.equal(g, r), f"output {i}: with the stream forced to NULL the calls did not run on the null stream"


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: the reference's loop on the tiny decoder
# ---------------------------------------------------------------------------------------------------------------------------------
ACCUM = 2


def _objects(case):
    dec = TD.MUSt3R(enc_embed_dim=case["Denc"], embed_dim=case["D"], depth=case["depth"], num_heads=case["heads"], mlp_ratio=case["hidden"] / case["D"],
                    feedback_type=case["feedback_type"], memory_mode=case["mode"], rope=case["rope"], eps=case["eps"])
    dec.load_state_dict(case["params"], strict=True)
    dec = dec.to(DEV)
    opt = TO.AdamW(TO.get_parameter_groups(dec, 0, 0.05), lr=1e-3, betas=(0.9, 0.95))
    return dec, opt, TO.LossScaler()


def _iterate(case, gt, crit, args, dec, opt, scaler, its, save_after=None):
    losses = []
    for it in its:
        if it % ACCUM == 0:
            TO.adjust_learning_rate(opt, 1 + it / 6, args)
        mem = None
        for c in case["calls"]:
            B, n = case["scenes"], case["n"]
            pos = case["pos"].to(DEV).view(1, 1, n, 2).expand(B, c["V"], n, 2).contiguous()
            ts = torch.tensor([case["H"], case["W"]]).view(1, 1, 2).expand(B, c["V"], 2).contiguous()
            mem, pts = dec(c["x"].to(DEV), pos, ts, mem, render=c["render"])
        loss, _ = crit(gt, TL.postprocess(pts, "norm_exp"))
        losses.append(float(loss.detach()))
        norm = scaler(loss / ACCUM, opt, clip_grad=None, parameters=dec.parameters(), update_grad=(it + 1) % ACCUM == 0)
        if (it + 1) % ACCUM == 0:
            assert norm.ndim == 0 and norm.is_cuda and math.isfinite(float(norm)) and float(norm) > 0
            opt.zero_grad()
        else:
            assert norm is None
        if save_after == it:
            TO.save_model(args, 0, torch.nn.Identity(), dec, opt, scaler, "last")
    return losses


def test_six_iterations_of_the_training_loop_and_a_resume(tmp_path):
    case = DF.make_case(mode="norm_y", causal=False)
    last = case["calls"][-1]
    assert last["render"]
    gt, _ = MR.make_case(case["scenes"], last["V"], case["H"], case["W"], 7, scale=2.0, sky_frac=0.1, metric=[True, False])
    gt = MR.to_device(gt, {}, DEV)[0]
    crit = TL.ConfLoss(TL.Regr3D(TL.L21, norm_mode="?avg_dis", sky_loss_value=2, loss_in_log=False), alpha=0.2)
    args = types.SimpleNamespace(lr=1e-3, min_lr=1e-5, warmup_epochs=1, epochs=3, output_dir=str(tmp_path))
    dec, opt, scaler = _objects(case)
    losses = _iterate(case, gt, crit, args, dec, opt, scaler, range(6), save_after=3)
    print("losses:", " ".join(f"{l:.6f}" for l in losses))
    assert losses[1] == losses[0], "an accumulating iteration takes no step"
    assert losses[2] < losses[0] and losses[4] < losses[0], "the loss falls"
    assert opt.steps_taken == 3
    stepped = [p for p in dec.parameters() if len(opt.state[p])]
    assert stepped and all(float(opt.state[p]["step"]) == 3.0 for p in stepped)
    assert float(scaler._scale) == 65536.0 and int(scaler._tracker) == 3
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([1e-5 + (1e-3 - 1e-5) * 0.5 * (1 + math.cos(math.pi * (4 / 6) / 2))] * len(opt.param_groups), rel=1e-12)
    # fresh objects resume from the checkpoint written after iteration 3 and finish bit-equal
    dec2, opt2, scaler2 = _objects(case)
    TO.load_model(args, str(tmp_path / "checkpoint-last.pth"), torch.nn.Identity(), dec2, opt2, scaler2)
    assert args.start_epoch == 1
    again = _iterate(case, gt, crit, args, dec2, opt2, scaler2, range(4, 6))
    assert again == losses[4:]
    for (k, a), b in zip(dec.state_dict().items(), dec2.state_dict().values()):
        assert torch.equal(a, b), k
    for p, q in zip(dec.parameters(), dec2.parameters()):
        assert len(opt.state[p]) == len(opt2.state[q])
        assert all(torch.equal(opt.state[p][k], opt2.state[q][k]) for k in opt.state[p])
    assert int(scaler2._tracker) == 3
