"""GPU (-m gpu): the trainable encoder -- must3r_amd/train_encoder.py on csrc/train_encoder.hip (must3r_hip_patch_rows) and the training blocks -- against the
yardstick tests/encoder_ref.py (itself held to the reference's own Dust3rEncoder class by tests/test_encoder_grad_host.py).

The gather is a permutation and is held exactly, canaries around both outputs.  The patch embedding is the gather followed by train_block's Linear and is held
to the bits of that Linear on torch-gathered rows, in both Linear modes.  The encoder is held to the bound of the other training tests (tests/grad_parity.py):
``e_gpu <= 4 e_ref + 32 2^-24 m`` against the fp64 yardstick, e_ref the error of the same formulas under fp32 CPU autograd (under ``precision="bf16"``: under
``torch.autocast("cpu", bfloat16)``, the rule of the linear16 and attn16 decoder tests), m = max|g64|.  Every tensor's row is printed before it is asserted; the
rows go, as a table, to the file M3R_ENCODER_GRAD_TABLE names (kept as profiles/encoder_grad_parity.txt).

Shapes of the gather (V, H, W as stored): (1, 16, 16) one token, a quarter of a block; (3, 48, 80) the mixed case of the host test, 135 tiles: no multiple of
the block's four; (2, 16, 80) and (5, 48, 64): grids of one row and of unequal sides, both ways round; (2, 32, 32) a square, where the two forms differ in
the order of the tokens alone."""
import ctypes as C
import functools
import os
import time

import pytest
import torch

import decoder_ref as DF
import encoder_ref as ER
import grad_parity as GP
from must3r_amd import _lib, train_block as TB, train_decoder as TD, train_encoder as TE, train_optim as TO
import must3r_amd.model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -7.25e11
ICANARY = -(7 << 40)

_HEADER = (
    "# tests/test_encoder_grad_gpu.py: per case and tensor, e_gpu = max |GPU - fp64|, e_ref = max |CPU autograd - fp64| (fp32; under precision bf16: fp32",
    "# under torch.autocast('cpu', bfloat16)), both in units of 2^-24 m; bound = 4 e_ref + 32; ratio = e_gpu / bound; m = max|g64|.  x is the encoder's",
    "# output and is held to the same bound.  Every tensor is held to the bound; a row is the worst tensor of its group (the blocks of one layer, ...).",
)
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    GP.write_table(os.environ.get("M3R_ENCODER_GRAD_TABLE"), _HEADER, list(_worst.values()), (30, 52), magnitude="m")


def _group(name):
    parts = name.split(".")
    return ".".join(parts[:2]) if parts[0] == "blocks_enc" else parts[0]


def _compare(tag, got, g64, g32):
    rows = []
    try:
        GP.compare(rows, tag, got, g64, g32)
    finally:
        for r in rows:
            key = (tag, _group(r[1]))
            if key not in _worst or r[5] > _worst[key][5]:
                _worst[key] = (tag, f"{key[1]}: {r[1]}", *r[2:])


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the gather
# ---------------------------------------------------------------------------------------------------------------------------------
GATHER_SHAPES = [(1, 16, 16), (3, 48, 80), (2, 16, 80), (2, 32, 32), (5, 48, 64)]
FLAGS = ("null", "none", "mixed", "all")


def _flags(kind, V):
    return {"null": None, "none": [0] * V, "mixed": [(v + 1) % 2 for v in range(V)], "all": [1] * V}[kind]


def _arange_img(V, H, W):
    return torch.arange(V * 3 * H * W, dtype=torch.float32).view(V, 3, H, W)


def _direct(img, flags, want_rows=True, want_pos=True):
    """must3r_hip_patch_rows with both outputs inside arenas of canaries, 64 elements of guard on either side; -> (rows arena, pos arena, n_rows)"""
    V, _, H, W = img.shape
    R = V * (H // 16) * (W // 16)
    rows = torch.full((R * 768 + 128,), CANARY, dtype=torch.float32, device=DEV)
    pos = torch.full((R * 2 + 128,), ICANARY, dtype=torch.int64, device=DEV)
    a = _lib.PatchRowsArgs()
    a.img = img.data_ptr()
    a.transposed = None if flags is None else flags.data_ptr()
    a.rows = rows.data_ptr() + 4 * 64 if want_rows else None
    a.pos = pos.data_ptr() + 8 * 64 if want_pos else None
    a.V, a.H, a.W = V, H, W
    a.stream = _lib.stream_ptr(img.device)
    _lib.check(_lib.load().must3r_hip_patch_rows(C.byref(a)))
    torch.cuda.synchronize()
    return rows.cpu(), pos.cpu(), R


@pytest.mark.parametrize("kind", FLAGS)
@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_is_exact_and_writes_nothing_else(shape, kind):
    V, H, W = shape
    img = _arange_img(V, H, W)
    fl = _flags(kind, V)
    ref_rows, ref_pos = ER.patch_rows(img, None if fl is None else torch.tensor(fl, dtype=torch.bool))
    assert ref_rows.unique().numel() == ref_rows.numel() == img.numel()                  # a permutation of distinct values
    d_img, d_fl = img.to(DEV), None if fl is None else torch.tensor(fl, dtype=torch.int32, device=DEV)
    rows, pos, R = _direct(d_img, d_fl)
    assert torch.equal(rows[64:-64].view(R, 768), ref_rows) and torch.equal(pos[64:-64].view(R, 2), ref_pos)
    assert bool((rows[:64] == CANARY).all()) and bool((rows[-64:] == CANARY).all()) and bool((pos[:64] == ICANARY).all()) and bool((pos[-64:] == ICANARY).all())
    # each output alone: the same bits, and the other buffer is not touched
    rows1, pos1, _ = _direct(d_img, d_fl, want_pos=False)
    assert torch.equal(rows1, rows) and bool((pos1 == ICANARY).all())
    rows2, pos2, _ = _direct(d_img, d_fl, want_rows=False)
    assert torch.equal(pos2, pos) and bool((rows2 == CANARY).all())
    # the wrapper
    w_rows, w_pos = TE.patch_rows(d_img, d_fl)
    assert torch.equal(w_rows.cpu(), ref_rows) and torch.equal(w_pos.cpu(), ref_pos) and w_pos.dtype == torch.int64
    assert TE.patch_rows(d_img, d_fl, want=(False, True))[0] is None and TE.patch_rows(d_img, d_fl, want=(True, False))[1] is None


def test_a_nonzero_flag_of_any_value_is_a_portrait_view():
    img = _arange_img(3, 48, 80)
    ref_rows, ref_pos = ER.patch_rows(img, torch.tensor([True, False, True]))
    rows, pos = TE.patch_rows(img.to(DEV), torch.tensor([-1, 0, 1 << 20], dtype=torch.int32, device=DEV))
    assert torch.equal(rows.cpu(), ref_rows) and torch.equal(pos.cpu(), ref_pos)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the patch embedding: the bits of train_block's Linear on torch-gathered rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _embed_case(E, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((3, 3, 48, 80), generator=g) * 2 - 1
    return dict(img=img, ts=torch.tensor(TRUE_SHAPE), w=torch.randn((E, 3, 16, 16), generator=g) * 768 ** -0.5, b=0.1 * torch.randn((E,), generator=g),
                dy=torch.randn((3, 15, E), generator=g) * 1e-7)


TRUE_SHAPE = [(48, 80), (80, 48), (48, 80)]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("E", [64, 128])
def test_patch_embed_has_the_bits_of_linear_on_gathered_rows(E, mode):
    c = _embed_case(E, 90 + E)
    rows, ref_pos = ER.patch_rows(c["img"], ER.portrait_flags(c["ts"], True))
    w2 = c["w"].view(E, 768).to(DEV).requires_grad_(True)
    b2 = c["b"].to(DEV).requires_grad_(True)
    w, b = c["w"].to(DEV).requires_grad_(True), c["b"].to(DEV).requires_grad_(True)
    dy = c["dy"].to(DEV)
    with TB.linear_precision(mode):
        ref = TB.linear(rows.to(DEV), w2, b2)
        x, pos = TE.patch_embed(c["img"].to(DEV), w, b, c["ts"].to(DEV), many_ar=True)
    ref.backward(dy.view(-1, E))                       # after the block has ended: each backward runs in the mode of its forward
    x.backward(dy)
    torch.cuda.synchronize()
    assert x.shape == (3, 15, E) and pos.shape == (3, 15, 2) and not pos.requires_grad
    assert torch.equal(x.view(-1, E), ref) and torch.equal(pos.view(-1, 2).cpu(), ref_pos)
    assert w.grad.shape == (E, 3, 16, 16) and torch.equal(w.grad.view(E, 768), w2.grad) and torch.equal(b.grad, b2.grad)
    assert float(w.grad.abs().max()) > 0 and float(b.grad.abs().max()) > 0
    if mode == "bf16":
        with TB.linear_precision("fp32"):
            x32, _ = TE.patch_embed(c["img"].to(DEV), w, b, c["ts"].to(DEV), many_ar=True)
        assert not torch.equal(x32, x)
    # without many_ar the shapes are ignored: the landscape rows
    rows_l, _ = ER.patch_rows(c["img"])
    with torch.no_grad(), TB.linear_precision(mode):
        xl, _ = TE.patch_embed(c["img"].to(DEV), w, b, c["ts"].to(DEV))
        assert torch.equal(xl.view(-1, E), TB.linear(rows_l.to(DEV), w2, b2)) and not torch.equal(xl, x)


def test_patch_embed_computes_only_what_is_asked_for():
    c = _embed_case(64, 7)
    img, ts, dy = c["img"].to(DEV), c["ts"].to(DEV), c["dy"].to(DEV)
    w, b = c["w"].to(DEV).requires_grad_(True), c["b"].to(DEV).requires_grad_(True)
    x, _ = TE.patch_embed(img, w, b, ts, True)
    x.backward(dy)
    full_w, full_b = w.grad.clone(), b.grad.clone()
    for freeze_w, freeze_b in ((True, False), (False, True)):
        w2, b2 = c["w"].to(DEV).requires_grad_(not freeze_w), c["b"].to(DEV).requires_grad_(not freeze_b)
        x2, _ = TE.patch_embed(img, w2, b2, ts, True)
        x2.backward(dy)
        assert torch.equal(x2, x)
        assert (w2.grad is None) == freeze_w and (b2.grad is None) == freeze_b
        assert freeze_w or torch.equal(w2.grad, full_w)
        assert freeze_b or torch.equal(b2.grad, full_b)
    # both frozen: no graph at all
    x3, _ = TE.patch_embed(img, w.detach(), b.detach(), ts, True)
    assert not x3.requires_grad and torch.equal(x3, x)
    # a half-precision weight: its gradient comes back in its dtype and shape
    wh = c["w"].to(DEV).half().requires_grad_(True)
    xh, _ = TE.patch_embed(img, wh, b, ts, True)
    xh.backward(dy)
    assert wh.grad.dtype == torch.float16 and wh.grad.shape == wh.shape


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the encoder against the yardstick
# ---------------------------------------------------------------------------------------------------------------------------------
GEOMS = {"d64": (64, 1, 128), "d128": (128, 2, 512)}          # d64 with ManyAR is the case of tests/test_encoder_grad_host.py
EMBEDS = {"manyar": dict(V=3, H=48, W=80, true_shape=TRUE_SHAPE, many_ar=True), "dust3r": dict(V=2, H=32, W=48)}


@functools.lru_cache(maxsize=None)
def _case(geom, embed):
    D, heads, hidden = GEOMS[geom]
    return ER.make_case(D, heads, hidden, 2, seed=81 if (geom, embed) == ("d64", "manyar") else 82 + len(geom) + len(embed), **EMBEDS[embed])


@functools.lru_cache(maxsize=None)
def _reference(geom, embed, autocast=False):
    """computed once, shared, never modified: (fp64 results, positions) or the fp32 results (under bf16 CPU autocast with ``autocast``)"""
    case = _case(geom, embed)
    if not autocast:
        return ER.grads(case, torch.float64), ER.grads(case, torch.float32)[0]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        res = ER.grads(case, torch.float32)[0]
    return {k: v.float() for k, v in res.items()}


def _module(case, precision="fp32"):
    enc = TE.Dust3rEncoder(img_size=(case["H"], case["W"]), embed_dim=case["D"], depth=case["depth"], num_heads=case["heads"],
                           mlp_ratio=case["hidden"] / case["D"], patch_embed="ManyAR_PatchEmbed" if case["many_ar"] else "PatchEmbedDust3R", precision=precision)
    enc.load_state_dict(case["params"], strict=True)
    return enc.to(DEV)


def _run(case, enc, img=None, ts=None, backward=True):
    enc.zero_grad(set_to_none=True)
    img = case["img"].to(DEV) if img is None else img
    ts = case["true_shape"].to(DEV) if ts is None else ts
    x, pos = enc(img, ts)
    res = dict(x=x.detach().reshape(-1, case["D"]), pos=pos.detach())
    if backward:
        x.backward(case["dy"].to(DEV).view(x.shape))
        res.update({k: t.grad for k, t in enc.named_parameters()})
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("embed", list(EMBEDS))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_encoder_matches_autograd(geom, embed):
    case = _case(geom, embed)
    (g64, pos64), g32 = _reference(geom, embed)
    got = _run(case, _module(case))
    assert got["pos"].dtype == torch.int64 and torch.equal(got["pos"].cpu().view(-1, 2), pos64)
    assert set(g64) == {"x", *ER.param_names(2)} <= set(got)
    _compare(f"{geom} {embed} fp32", got, g64, g32)


@pytest.mark.parametrize("embed", list(EMBEDS))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_encoder_in_bf16_matches_fp64_like_autocast(geom, embed):
    case = _case(geom, embed)
    (g64, pos64), g32 = _reference(geom, embed)
    got = _run(case, _module(case, "bf16"))
    assert torch.equal(got["pos"].cpu().view(-1, 2), pos64)
    _compare(f"{geom} {embed} bf16", got, g64, _reference(geom, embed, True))
    plain = _run(case, _module(case))
    assert not torch.equal(plain["x"], got["x"])


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) bits
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_calls_repeat_bitwise_and_a_view_alone_has_the_batchs_bits():
    case = _case("d64", "manyar")
    enc = _module(case)
    first, second = _run(case, enc), _run(case, enc)
    assert set(first) == {"x", "pos", *ER.param_names(2)} and not _same(first, second)
    n, D = case["n"], case["D"]
    for v in range(3):
        alone = _run(case, enc, case["img"][v:v + 1].to(DEV), case["true_shape"][v:v + 1].to(DEV), backward=False)
        assert torch.equal(alone["x"], first["x"][v * n:(v + 1) * n]) and torch.equal(alone["pos"][0], first["pos"][v])


def test_portrait_view_has_the_bits_of_the_swapped_image_run_as_landscape():
    case = _case("d64", "manyar")
    many = _module(case)
    plain = TE.Dust3rEncoder(img_size=(80, 48), embed_dim=64, depth=2, num_heads=1, mlp_ratio=2, patch_embed="PatchEmbedDust3R")
    plain.load_state_dict(case["params"], strict=True)
    plain = plain.to(DEV)
    one = case["img"][1:2].to(DEV)
    with torch.no_grad():
        xp, pp = many(one, torch.tensor([[80, 48]], device=DEV))
        xl, pl = plain(one.swapaxes(-1, -2).contiguous(), None)
        xs, ps = many(one, torch.tensor([[48, 80]], device=DEV))          # the same image declared landscape
    assert torch.equal(xp, xl) and torch.equal(pp, pl) and int(pp[..., 0].max()) == 4 and int(pp[..., 1].max()) == 2
    assert not torch.equal(xs, xp) and int(ps[..., 0].max()) == 2


def test_precision_argument_and_ambient_modes():
    case = _case("d64", "manyar")
    fp32, bf16, free = _module(case, "fp32"), _module(case, "bf16"), _module(case, None)
    r32, r16 = _run(case, fp32), _run(case, bf16)
    assert _same(r32, r16)
    with TB.amp("bf16"):
        inside32 = _run(case, fp32)                    # fp32 is entered explicitly: the reference's encoder runs with autocast disabled
        inside_free = _run(case, free)                 # None leaves the caller's modes alone
        assert TB.current_precision() == "bf16" and TB.current_attention_precision() == "bf16"
    assert not _same(r32, inside32) and not _same(r16, inside_free)
    assert not _same(r32, _run(case, free))
    assert TB.current_precision() == "fp32" and TB.current_attention_precision() == "fp32"
    # backward after the block has ended runs in the forward's modes
    free.zero_grad(set_to_none=True)
    with TB.amp("bf16"):
        x, _ = free(case["img"].to(DEV), case["true_shape"].to(DEV))
    x.backward(case["dy"].to(DEV).view(x.shape))
    torch.cuda.synchronize()
    assert not [k for k, t in free.named_parameters() if not torch.equal(t.grad, r16[k])]


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) the caller's stream, and no wait on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def _stream_call(bufs):
    """patch_rows, and patch_embed forward + backward with a device true_shape, on the current stream and the bound input buffers"""
    rows, pos = TE.patch_rows(bufs["img"], bufs["flags"])
    w, b = bufs["w"].detach().requires_grad_(True), bufs["b"].detach().requires_grad_(True)
    x, pos2 = TE.patch_embed(bufs["img"], w, b, bufs["ts"], many_ar=True)
    x.backward(bufs["dy"])
    return [rows, pos, x.detach(), pos2, w.grad, b.grad]


def _stream_inputs(seed, ts):
    c = _embed_case(64, seed)
    t = torch.tensor(ts)
    return {"img": c["img"].to(DEV), "flags": (t[:, 0] > t[:, 1]).to(torch.int32).to(DEV), "ts": t.to(DEV), "w": c["w"].to(DEV), "b": c["b"].to(DEV),
            "dy": c["dy"].to(DEV)}


def test_gather_and_patch_embed_run_on_the_descriptors_stream():
    """The protocol of tests/test_decoder_grad_gpu.py::test_both_entry_points_run_on_the_descriptors_stream: reference bits of two input sets A and B on the
    default stream; then, with the inputs holding B, on a side stream the null stream overtakes: a delay, copies of A, the calls, clones of the outputs, B
    back.  The clones must be A's bits and the delay must still be running when the calls have returned.  Control: the same calls with the null stream as
    the stream of the descriptors AND of the torch operations around them (the flags of patch_embed are computed by torch) reproduce B's bits."""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay, null_stream
    delay = Delay()
    src = {"A": _stream_inputs(21, TRUE_SHAPE), "B": _stream_inputs(22, [(80, 48), (48, 80), (48, 80)])}
    bufs = {k: torch.empty_like(v) for k, v in src["A"].items()}

    def load(which):
        for k, v in src[which].items():
            bufs[k].copy_(v)
    ref = {}
    for which in ("A", "A", "B"):
        load(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = _stream_call(bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        ref[which] = [t.clone() for t in outs]
    assert all(not torch.equal(a, b) for a, b in zip(ref["A"], ref["B"]))
    ms = min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)
    assert ms < DELAY_CAP_MS or host_ms < DELAY_CAP_MS / 10
    # the side stream
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")
        t0 = time.perf_counter()
        outs = _stream_call(bufs)
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in outs]
        load("B")
    s.synchronize()
    print(f"patch_rows + patch_embed: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the calls took {side_ms:.3f} ms on the host)"
    for i, (g, r) in enumerate(zip(got, ref["A"])):
        assert torch.equal(g, r), f"output {i}: on a side stream the bits differ from the default-stream bits (equal to the decoy's: {torch.equal(g, ref['B'][i])})"
    # the control: on the null stream the calls read the decoy
    load("B")
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        load("A")                         # queued behind the delay: the inputs still hold the decoy
        with torch.cuda.stream(torch.cuda.default_stream()), null_stream():
            outs = _stream_call(bufs)
            torch.cuda.default_stream().synchronize()
            got = [t.clone() for t in outs]
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    assert premise, f"the delay ({ms:.1f} ms) ended before the null stream was idle"
    for i, (g, r) in enumerate(zip(got, ref["B"])):
        assert torch.equal(g, r), f"output {i}: with the null stream the calls did not run on the null stream"


def test_encoder_forward_returns_while_a_delay_ahead_of_it_is_running():
    """The whole forward (mixed orientations, D 64, depth 2) reads nothing back: queued behind a delay on a side stream, it returns before the delay ends,
    and its results are the default stream's bits."""
    from test_stream_order_gpu import DELAY_CAP_MS, Delay
    delay = Delay()
    case = _case("d64", "manyar")
    enc = _module(case)
    img, ts = case["img"].to(DEV), case["true_shape"].to(DEV)
    for _ in range(2):                                  # the second call has the RoPE table and the allocator's blocks
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            ref_x, ref_pos = enc(img, ts)
        host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    ms = min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)
    assert ms < DELAY_CAP_MS or host_ms < DELAY_CAP_MS / 10
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        t0 = time.perf_counter()
        x, pos = enc(img, ts)                           # with grad: the autograd Functions' forwards
        side_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
    s.synchronize()
    print(f"encoder forward: delay {ms:.1f} ms, host {side_ms:.3f} ms (default stream {host_ms:.3f} ms), premise {premise}")
    assert premise, f"delay too short or a host synchronisation (delay {ms:.1f} ms, the forward took {side_ms:.3f} ms on the host)"
    assert torch.equal(x.detach(), ref_x) and torch.equal(pos, ref_pos)


# ---------------------------------------------------------------------------------------------------------------------------------
# (f) end to end: images -> train_encoder.inference over train_decoder.MUSt3R -> loss -> gradients -> an optimizer step
# ---------------------------------------------------------------------------------------------------------------------------------
E2E_HELD = ("enc.patch_embed.proj.weight", "enc.blocks_enc.0.attn.qkv.weight", "enc.norm_enc.weight", "dec.blocks_dec.0.cross_attn.projq.weight")
MEM_BATCHES, TO_RENDER = [2, 1], [2, 0]


@functools.lru_cache(maxsize=None)
def _e2e_case():
    """B 2 scenes of 3 views of 32 x 48 (2 x 3 tokens); encoder D 64 / depth 2, decoder D 64 / depth 2 with the single_mlp feedback"""
    enc = ER.make_case(64, 1, 128, 2, 6, 32, 48, seed=95)
    dec = DF.make_case(Denc=64, D=64, heads=1, hidden=256, depth=2, feedback_type="single_mlp", mode="norm_y", scenes=2, grid=(2, 3), seed=96, schedule=())
    g = torch.Generator().manual_seed(97)
    return dict(enc=enc, dec=dec, G0=torch.randn((2, 3, 32, 48, 7), generator=g) * 1e-7, G=torch.randn((2, 2, 32, 48, 7), generator=g) * 1e-7)


@functools.lru_cache(maxsize=None)
def _e2e_reference(dtype):
    """The composition of encoder_ref and decoder_ref under CPU autograd: the gradients of sum <pointmaps_0, G0> + sum <pointmaps, G> at every parameter"""
    c = _e2e_case()
    ec, dc = c["enc"], c["dec"]
    pe = {k: v.to(dtype).clone().requires_grad_(True) for k, v in ec["params"].items()}
    pd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in dc["params"].items()}
    x, _ = ER.encoder(ec["img"].to(dtype), None, pe, ec["heads"], ec["depth"], ec["rope"], ec["eps"])
    x = x.view(2, 3, ec["n"], 64)
    mem, first, lo = None, [], 0
    for nb in MEM_BATCHES:
        mem, _, pts = DF.call(dc, pd, x[:, lo:lo + nb], mem, False)
        first.append(pts)
        lo += nb
    _, _, pts = DF.call(dc, pd, x[:, TO_RENDER], mem, True)
    p0 = torch.cat(first, dim=1)
    ((p0 * c["G0"].to(dtype)).sum() + (pts * c["G"].to(dtype)).sum()).backward()
    res = {f"enc.{k}": t.grad for k, t in pe.items()}
    res.update({f"dec.{k}": t.grad for k, t in pd.items()})
    return res, p0.detach(), pts.detach()


def _e2e_modules():
    c = _e2e_case()
    enc = _module(c["enc"])
    dc = c["dec"]
    dec = TD.MUSt3R(enc_embed_dim=64, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4.0, feedback_type="single_mlp", memory_mode="norm_y", rope=dc["rope"], eps=dc["eps"])
    dec.load_state_dict(dc["params"], strict=True)
    return enc, dec.to(DEV)


def _e2e_inputs():
    c = _e2e_case()
    return c["enc"]["img"].to(DEV).view(2, 3, 3, 32, 48), torch.tensor([32, 48]).view(1, 1, 2).expand(2, 3, 2).contiguous()


def test_end_to_end_gradients():
    c = _e2e_case()
    g64, p0_64, pts_64 = _e2e_reference(torch.float64)
    g32, _, _ = _e2e_reference(torch.float32)
    enc, dec = _e2e_modules()
    imgs, ts = _e2e_inputs()
    p0, pts = TE.inference(enc, dec, imgs, ts, MEM_BATCHES, to_render=TO_RENDER, encoder_requires_grad=True)
    assert p0.shape == (2, 3, 32, 48, 7) and pts.shape == (2, 2, 32, 48, 7)
    for name, got, ref in (("pointmaps_0", p0, p0_64), ("pointmaps", pts, pts_64)):
        err = float((got.detach().cpu().double() - ref).abs().max())
        print(f"end to end {name}: max abs error {err:.3e} of max|out| {float(ref.abs().max()):.3e}")
        assert torch.allclose(got.detach().cpu().double(), ref, rtol=1e-5, atol=1e-4), (name, err)          # the head's split-precision forward (test_head_grad_gpu.py)
    ((p0 * c["G0"].to(DEV)).sum() + (pts * c["G"].to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    got = {f"enc.{k}": t.grad for k, t in enc.named_parameters()}
    got.update({f"dec.{k}": t.grad for k, t in dec.named_parameters()})
    assert all(v is not None for v in got.values())
    _compare("end to end", got, {k: g64[k] for k in E2E_HELD}, g32)


def test_optimizer_step_and_the_native_encoder_serves_the_result():
    """One native AdamW step over encoder and decoder parameters after a backward through the driver; the native encoder, whose widths are multiples of 128,
    loads the result: hence an encoder of D 128 (depth 1) in front of the D 64 decoder."""
    ec = ER.make_case(128, 2, 256, 1, 6, 32, 48, seed=98)
    dc = DF.make_case(Denc=128, D=64, heads=1, hidden=256, depth=2, feedback_type="single_mlp", mode="norm_y", scenes=2, grid=(2, 3), seed=99, schedule=())
    enc = _module(ec)
    dec = TD.MUSt3R(enc_embed_dim=128, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4.0, feedback_type="single_mlp", memory_mode="norm_y")
    dec.load_state_dict(dc["params"], strict=True)
    dec = dec.to(DEV)
    imgs, ts = ec["img"].to(DEV).view(2, 3, 3, 32, 48), _e2e_inputs()[1]
    p0, pts = TE.inference(enc, dec, imgs, ts, MEM_BATCHES, to_render=TO_RENDER, encoder_requires_grad=True)
    (p0.square().mean() + pts.square().mean()).backward()
    params = list(enc.parameters()) + list(dec.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    dec_before = {k: v.clone() for k, v in dec.state_dict().items()}
    TO.AdamW(params, lr=1e-3).step()
    torch.cuda.synchronize()
    assert all(not torch.equal(v, dec_before[k]) for k, v in dec.state_dict().items())
    native = M.Dust3rEncoder(img_size=(32, 48), embed_dim=128, depth=1, num_heads=2, mlp_ratio=2)
    native.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()}, strict=True)
    for k, v in native.state_dict().items():
        assert torch.equal(v, enc.state_dict()[k].cpu()) and not torch.equal(v, before[k].cpu()), k


def test_end_to_end_frozen_encoder_has_no_gradient():
    c = _e2e_case()
    enc, dec = _e2e_modules()
    imgs, ts = _e2e_inputs()
    p0, pts = TE.inference(enc, dec, imgs, ts, MEM_BATCHES, to_render=TO_RENDER, encoder_requires_grad=False)
    ((p0 * c["G0"].to(DEV)).sum() + (pts * c["G"].to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in enc.parameters()) and all(p.grad is not None for p in dec.parameters())
    # the decoder's gradients are those of the run with the encoder in the graph: the encoder's output has the same bits either way
    enc2, dec2 = _e2e_modules()
    q0, qts = TE.inference(enc2, dec2, imgs, ts, MEM_BATCHES, to_render=TO_RENDER, encoder_requires_grad=True)
    assert torch.equal(q0, p0) and torch.equal(qts, pts)


class _Features:
    """an encoder that hands out a leaf: what reaches the views of each batch through the decoder shows in its gradient"""

    def __init__(self, x, pos):
        self.x, self.pos = x, pos

    def __call__(self, img, true_shape):
        return self.x.view(-1, *self.x.shape[2:]), self.pos


def test_skipped_updates_pass_no_gradient_to_their_views():
    c = _e2e_case()
    enc, dec = _e2e_modules()
    imgs, ts = _e2e_inputs()
    with torch.no_grad():
        x, pos = enc(imgs.view(6, 3, 32, 48), ts.view(6, 2))
    grads = {}
    for skip in (0, 1):
        leaf = x.view(2, 3, -1, 64).clone().requires_grad_(True)
        dec.zero_grad(set_to_none=True)
        p0, pts = TE.inference(_Features(leaf, pos), dec, imgs, ts, MEM_BATCHES, train_decoder_skip=skip, to_render=[2], encoder_requires_grad=True)
        assert p0.shape[1] == 3 - 2 * skip and pts.shape[1] == 1
        (p0.sum() + pts.sum()).backward()
        torch.cuda.synchronize()
        grads[skip] = leaf.grad.clone()
    assert float(grads[0][:, :2].abs().max()) > 0 and float(grads[0][:, 2].abs().max()) > 0
    assert float(grads[1][:, :2].abs().max()) == 0 and float(grads[1][:, 2].abs().max()) > 0
