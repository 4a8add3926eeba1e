"""GPU (-m gpu): a batch stored landscape with portrait views through the trainable decoders -- ``train_decoder.MUSt3R`` / ``CausalMUSt3R`` built with
``landscape_only=True`` and, from the images on, ``train_encoder.inference`` -- against a yardstick composed of tests/decoder_ref.py (the tokens: the blocks
see a view's orientation through its positions alone) and tests/head_ar_ref.py (the head), under CPU autograd in fp64 and fp32.

The case: D 64, depth 2, B = 2 scenes of three views stored 48 x 80 (3 x 5 tokens); the second view of scene 0 and the first of scene 1 are portrait views
(5 x 3 tokens).  Schedule: an update of views 0 and 1, an update of view 2, a render of all three.  Every dx and every parameter gradient is held to the rule of
tests/grad_parity.py as tests/test_decoder_grad_gpu.py applies it (cross_attn.projk.bias with the magnitude of what cancels in it), and so are the pointmaps,
which go through the head's split-precision forward and are also held to the bound that file and tests/test_head_grad_gpu.py use for it (rtol 1e-5,
atol 1e-4).  Rows go to the file M3R_DECODER_MANY_AR_TABLE names."""
import functools
import os
import time

import pytest
import torch

import block_ref as BR
import decoder_ref as DF
import encoder_ref as ER
import grad_parity as GP
import head_ar_ref as HAR
import metrics_ref as MR
from must3r_amd import train_decoder as TD, train_dropout as TDrop, train_encoder as TE, train_losses as T, train_optim as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, W, GRID = 2, 48, 80, (3, 5)
FLAGS = ((0, 1, 0), (1, 0, 0))                       # per scene and view
SCHEDULE = ((0, 2, False), (2, 3, False), (0, 3, True))
KBIAS = "cross_attn.projk.bias"
_rows = []


class _Pos:
    """decoder_ref.call takes one view's positions and repeats them over the views of the call; here they differ from view to view"""

    def __init__(self, pos):
        self.pos = pos

    def repeat(self, views, _one):
        assert self.pos.shape[0] % views == 0
        return self.pos


def _positions(lo, hi):
    """int64 [B, V, n, 2]: the row-major grid of the view's own orientation"""
    n = GRID[0] * GRID[1]
    land, port = BR.grid_positions(n, GRID[1]), BR.grid_positions(n, GRID[0])
    return torch.stack([torch.stack([port if FLAGS[b][v] else land for v in range(lo, hi)]) for b in range(B)])


def _true_shape(lo, hi):
    return torch.stack([HAR.true_shape(FLAGS[b][lo:hi], H, W) for b in range(B)])


@functools.lru_cache(maxsize=None)
def _case(mode, causal):
    return DF.make_case(Denc=128, D=64, heads=1, hidden=256, depth=2, feedback_type="single_mlp", mode=mode, causal=causal, scenes=B, grid=GRID, seed=171,
                        schedule=tuple((hi - lo, render) for lo, hi, render in SCHEDULE))


def _head(case, p, tok, lo, hi):
    flags = [FLAGS[b][v] for b in range(B) for v in range(lo, hi)]
    pts = HAR.head(tok, p["norm_dec.weight"], p["norm_dec.bias"], p["head_dec.proj.weight"], p["head_dec.proj.bias"], flags, H, W, case["eps"])
    return pts.view(B, hi - lo, H, W, 7)


@functools.lru_cache(maxsize=None)
def _reference(mode, causal, dtype):
    """decoder_ref.grads with the positions of each view's orientation and head_ar_ref's head: pointmaps{c}, dx{c}, one entry per parameter; and the
    magnitudes of what cancels in the key biases.  Computed once, shared, never modified."""
    case = _case(mode, causal)
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in case["params"].items()}
    xs = [c["x"].to(dtype).clone().requires_grad_(True) for c in case["calls"]]
    keeps, mem, loss, res = [], None, 0, {}
    for i, (c, x, (lo, hi, render)) in enumerate(zip(case["calls"], xs, SCHEDULE)):
        cc = dict(case, pos=_Pos(_positions(lo, hi).reshape(-1, 2)))
        mem, tok, _ = DF.call(cc, p, x, mem, render, keeps)
        pts = _head(case, p, tok, lo, hi)
        res[f"pointmaps{i}"] = pts.detach()
        loss = loss + (pts * c["G"].to(dtype)).sum()
    loss.backward()
    D = case["D"]
    mags = {}
    for l in range(case["depth"]):
        cols = sum(t.grad.reshape(-1, t.shape[-1])[:, :D].abs().sum(dim=0) for ll, t in keeps if ll == l and t.grad is not None)
        mags[f"blocks_dec.{l}.{KBIAS}"] = float(cols.max())
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    res.update({k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in p.items()})
    return res, mags


def _module(case, cls=None, **kw):
    cls = cls or (TD.CausalMUSt3R if case["causal"] else TD.MUSt3R)
    dec = cls(enc_embed_dim=case["Denc"], embed_dim=case["D"], depth=case["depth"], num_heads=case["heads"], mlp_ratio=case["hidden"] / case["D"],
              feedback_type=case["feedback_type"], memory_mode=case["mode"], rope=case["rope"], eps=case["eps"], landscape_only=True, **kw)
    dec.load_state_dict(case["params"], strict=True)
    return dec.to(DEV)


def _run(case, dec, img_shape=(H, W), backward=True):
    dec.zero_grad(set_to_none=True)
    xs = [c["x"].to(DEV).requires_grad_(True) for c in case["calls"]]
    mem, loss, res = None, 0, {}
    for i, (c, x, (lo, hi, render)) in enumerate(zip(case["calls"], xs, SCHEDULE)):
        mem, pts = dec(x, _positions(lo, hi).to(DEV), _true_shape(lo, hi).to(DEV), mem, render=render, img_shape=img_shape)
        assert pts.shape == (B, hi - lo, H, W, 7) and pts.dtype == torch.float32
        res[f"pointmaps{i}"] = pts.detach()
        loss = loss + (pts * c["G"].to(DEV)).sum()
    if backward:
        loss.backward()
        res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
        res.update({k: t.grad for k, t in dec.named_parameters()})
    torch.cuda.synchronize()
    return res


def _hold_pointmaps(tag, got, g64, g32, names):
    for k in names:
        p, r = got[k].cpu().double(), g64[k]
        assert torch.allclose(p, r, rtol=1e-5, atol=1e-4), (tag, k, float((p - r).abs().max()))
    GP.compare(_rows, tag, got, {k: g64[k] for k in names}, g32)


_HEADER = (
    "# tests/test_decoder_many_ar_gpu.py: per case and tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in units of 2^-24 m;",
    "# bound = 4 e_ref + 32; ratio = e_gpu / bound.  m = max|g64|, except for cross_attn.projk.bias (the true gradient is zero): the largest column 1-norm of",
    "# the fp64 dK over the schedule.  The yardstick is tests/decoder_ref.py's tokens with each view's own positions and tests/head_ar_ref.py's head.",
)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_DECODER_MANY_AR_TABLE"), _HEADER, _rows, (20, 46), magnitude="m")


@pytest.mark.parametrize("mode,causal", [("norm_y", False), ("kv", True)], ids=["must3r-norm_y", "causal-kv"])
def test_decoder_matches_autograd_on_the_mixed_batch(mode, causal):
    case = _case(mode, causal)
    (g64, mags), (g32, _) = _reference(mode, causal, torch.float64), _reference(mode, causal, torch.float32)
    dec = _module(case)
    got = _run(case, dec)
    tag = f"{'causal' if causal else 'must3r'} {mode}"
    points = [k for k in g64 if k.startswith("pointmaps")]
    _hold_pointmaps(tag, got, g64, g32, points)
    names = [k for k in g64 if k not in points]
    assert set(names) <= set(got) and all(got[k] is not None for k in names)
    GP.compare(_rows, tag, got, {k: g64[k] for k in names}, g32, mags)
    # the portrait views are not the landscape run: without the flags the pointmaps of those views differ, the others' agree
    plain = _module(case)
    plain.landscape_only = False
    with torch.no_grad():
        lo, hi, _ = SCHEDULE[0]
        ts = torch.tensor([H, W]).view(1, 1, 2).expand(B, hi - lo, 2).contiguous()
        _, pts = plain(case["calls"][0]["x"].to(DEV), _positions(lo, hi).to(DEV), ts)
    for b in range(B):
        for v in range(lo, hi):
            assert torch.equal(pts[b, v], got["pointmaps0"][b, v]) == (not FLAGS[b][v]), (b, v)
    # without img_shape (H, W from the host's min / max of true_shape) the same bits
    again = _run(case, dec, img_shape=None)
    assert all(torch.equal(again[k], got[k]) for k in got), [k for k in got if not torch.equal(again[k], got[k])]


def test_dropout_decoder_passes_the_orientation_through():
    """``train_dropout.CausalMUSt3R`` at dropout 0 is ``train_decoder.CausalMUSt3R``: the same bits on the mixed batch, keyword included"""
    case = _case("kv", True)
    a = _run(case, _module(case), backward=False)
    b = _run(case, _module(case, TDrop.CausalMUSt3R), backward=False)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_forward_with_img_shape_returns_while_a_delay_ahead_of_it_is_running():
    """The delay method of tests/test_encoder_grad_gpu.py: with img_shape given the decoder's forward (true_shape on the device, mixed orientations) reads nothing
    back -- queued behind a delay on a side stream it returns before the delay ends, and its results are the default stream's bits: the head's new entry
    point ran wholly on the caller's stream.  Without img_shape the head reads true_shape on the host, which is what the reference does."""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay
    delay = Delay()
    case = _case("norm_y", False)
    dec = _module(case)
    c = case["calls"][0]
    lo, hi, _ = SCHEDULE[0]
    x, pos, ts = c["x"].to(DEV), _positions(lo, hi).to(DEV).reshape(-1, 2), _true_shape(lo, hi).to(DEV)
    for _ in range(2):                                  # the second call has the RoPE table, the checked positions and the allocator's blocks
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            _, ref = dec(x, pos, ts, img_shape=(H, W))
        host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    ms = min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)
    assert ms < DELAY_CAP_MS or host_ms < DELAY_CAP_MS / 10
    s = delay.side_stream()
    done = torch.cuda.Event()
    xg = x.clone().requires_grad_(True)
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        t0 = time.perf_counter()
        _, pts = dec(xg, pos, ts, img_shape=(H, W))     # with grad: the autograd Functions' forwards
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
    s.synchronize()
    print(f"decoder forward, mixed orientations: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the forward took {side_ms:.3f} ms on the host)"
    assert torch.equal(pts.detach(), ref)


def test_head_backward_runs_on_the_callers_stream():
    """The backward of the head with flags, queued behind a delay on a side stream after device-to-device copies of its inputs: it returns before the delay
    ends and its gradients are those of the copied inputs, not of the decoy the buffers held when it was called"""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay
    from must3r_amd import train_head as TH
    delay = Delay()
    V, D = 3, 64
    src = {w: {k: v.to(DEV) for k, v in HAR.make_case(V, H, W, (0, 1, 0), D=D, seed=s).items() if isinstance(v, torch.Tensor)} for w, s in (("A", 5), ("B", 6))}
    flags = {"A": torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV), "B": torch.tensor([1, 0, 0], dtype=torch.int32, device=DEV)}
    bufs = {k: torch.empty_like(v) for k, v in src["A"].items()}
    t = torch.empty_like(flags["A"])

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
        t.copy_(flags[which])

    def call():
        out = TH.head_forward(bufs["x"], bufs["gamma"], bufs["beta"], bufs["W"], bufs["b"], V, H, W, transposed=t)
        return [out, *TH.head_grad(bufs["x"], bufs["gamma"], bufs["beta"], bufs["W"], bufs["G"], V, H, W, transposed=t)]
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = call()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        ref[which] = [o.clone() for o in outs]
    assert all(not torch.equal(a, b) for a, b in zip(ref["A"], ref["B"]))
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
        got = [o.clone() for o in outs]
        load("B")
    s.synchronize()
    print(f"head forward + backward with flags: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the calls took {side_ms:.3f} ms on the host)"
    for i, (g, r) in enumerate(zip(got, ref["A"])):
        assert torch.equal(g, r), f"output {i}: on a side stream the bits differ from the default-stream bits (equal to the decoy's: {torch.equal(g, ref['B'][i])})"


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: images -> train_encoder.inference -> train_losses -> train_optim.AdamW, one step on the mixed batch
# ---------------------------------------------------------------------------------------------------------------------------------
MEM_BATCHES = [2, 1]


@functools.lru_cache(maxsize=None)
def _e2e_case():
    ts = [(W, H) if FLAGS[b][v] else (H, W) for b in range(B) for v in range(3)]
    enc = ER.make_case(64, 1, 128, 2, B * 3, H, W, true_shape=ts, many_ar=True, seed=195)
    dec = DF.make_case(Denc=64, D=64, heads=1, hidden=256, depth=2, feedback_type="single_mlp", mode="norm_y", scenes=B, grid=GRID, seed=196, schedule=())
    gt, _ = MR.make_case(B, 3, H, W, 7, scale=2.0, sky_frac=0.1, metric=[True, False])
    return dict(enc=enc, dec=dec, gt=gt)


def _e2e_yardstick(dtype, enc_params=None, dec_params=None):
    """encoder_ref (ManyAR) -> decoder_ref's tokens with the encoder's positions -> head_ar_ref -> metrics_ref's ConfLoss(Regr3D): the pointmaps and the loss"""
    c = _e2e_case()
    ec, dc = c["enc"], c["dec"]
    pe = {k: v.to(dtype) for k, v in (enc_params or ec["params"]).items()}
    pd = {k: v.to(dtype) for k, v in (dec_params or dc["params"]).items()}
    with torch.no_grad():
        x, pos = ER.encoder(ec["img"].to(dtype), ER.portrait_flags(ec["true_shape"], True), pe, ec["heads"], ec["depth"], ec["rope"], ec["eps"])
        x, pos = x.view(B, 3, ec["n"], 64), pos.view(B, 3, ec["n"], 2)
        assert torch.equal(pos, _positions(0, 3))
        mem, first, lo = None, [], 0
        for nb in MEM_BATCHES:
            mem, tok, _ = DF.call(dict(dc, pos=_Pos(pos[:, lo:lo + nb].reshape(-1, 2))), pd, x[:, lo:lo + nb], mem, False)
            first.append(_head(dc, pd, tok, lo, lo + nb))
            lo += nb
        _, tok, _ = DF.call(dict(dc, pos=_Pos(pos.reshape(-1, 2))), pd, x, mem, True)
        p0, pts = torch.cat(first, dim=1), _head(dc, pd, tok, 0, 3)
        crit = MR.ConfLoss(MR.Regr3D(MR.L21, norm_mode='?avg_dis', sky_loss_value=2), alpha=0.2)
        gt = MR.to64(c["gt"]) if dtype == torch.float64 else c["gt"]
        loss = crit(gt, HAR.HR.postprocess(p0))[0] + crit(gt, HAR.HR.postprocess(pts))[0]
    return p0, pts, float(loss)


def test_one_training_step_on_the_mixed_batch_from_the_images():
    c = _e2e_case()
    ec, dc = c["enc"], c["dec"]
    p0_64, pts_64, loss64 = _e2e_yardstick(torch.float64)
    p0_32, pts_32, _ = _e2e_yardstick(torch.float32)
    enc = TE.Dust3rEncoder(img_size=(H, W), embed_dim=64, depth=2, num_heads=1, mlp_ratio=2.0, patch_embed="ManyAR_PatchEmbed")
    enc.load_state_dict(ec["params"], strict=True)
    dec = TD.CausalMUSt3R(enc_embed_dim=64, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4.0, feedback_type="single_mlp", memory_mode="norm_y", rope=dc["rope"],
                          eps=dc["eps"], landscape_only=True)
    dec = TD.MUSt3R.from_decoder(dec, landscape_only=True)          # the keyword travels through from_decoder
    dec.load_state_dict(dc["params"], strict=True)
    enc, dec = enc.to(DEV), dec.to(DEV)
    imgs, ts = ec["img"].to(DEV).view(B, 3, 3, H, W), ec["true_shape"].to(DEV).view(B, 3, 2)
    gt = [{k: v.to(DEV) for k, v in g.items()} for g in c["gt"]]
    crit = T.ConfLoss(T.Regr3D(T.L21, norm_mode='?avg_dis', sky_loss_value=2), alpha=0.2)

    def step_loss():
        p0, pts = TE.inference(enc, dec, imgs, ts, MEM_BATCHES, encoder_requires_grad=True)
        return p0, pts, crit(gt, T.postprocess(p0, 'norm_exp'))[0] + crit(gt, T.postprocess(pts, 'norm_exp'))[0]
    p0, pts, loss = step_loss()
    assert p0.shape == pts.shape == (B, 3, H, W, 7)
    _hold_pointmaps("end to end", dict(pointmaps_0=p0.detach(), pointmaps=pts.detach()), dict(pointmaps_0=p0_64, pointmaps=pts_64),
                    dict(pointmaps_0=p0_32, pointmaps=pts_32), ("pointmaps_0", "pointmaps"))
    print(f"end to end: loss {float(loss.detach()):.6f} (fp64 yardstick {loss64:.6f})")
    assert bool(torch.isfinite(loss))
    loss.backward()
    params = list(enc.parameters()) + list(dec.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    before = [p.detach().clone() for p in params]
    TO.AdamW(params, lr=1e-5, weight_decay=0.0).step()
    torch.cuda.synchronize()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, params))
    # the step is downhill: the fp64 yardstick's loss at the stepped parameters
    _, _, after64 = _e2e_yardstick(torch.float64, {k: v.detach().cpu() for k, v in enc.state_dict().items()}, {k: v.detach().cpu() for k, v in dec.state_dict().items()})
    print(f"end to end: fp64 loss {loss64:.6f} -> {after64:.6f} after one AdamW step of lr 1e-5")
    assert after64 < loss64
