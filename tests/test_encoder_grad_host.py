"""CPU: the host side of the trainable encoder -- the yardstick tests/encoder_ref.py against the reference's own Dust3rEncoder class with ManyAR_PatchEmbed
(live where the reference tree exists, from the recorded fixture tests/golden/encoder_ref_d64.npz elsewhere), the ABI surface of must3r_hip_patch_rows and its
refusals, the Python refusals, the state-dict contract with the native encoder, the parameter groups, and the training form of the ``inference`` driver on
stub modules (no compute calls: no GPU here)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import encoder_ref as ER
import optim_cases as OC
from conftest import GOLDEN, HAS_REFERENCE, ROOT
from must3r_amd import _lib, inference as INF, train_block as TB, train_encoder as TE, train_optim as TO
from must3r_amd.config import TINY
import must3r_amd.model as M

FIXTURE = os.path.join(GOLDEN, "encoder_ref_d64.npz")
TRUE_SHAPE = [(48, 80), (80, 48), (48, 80)]


@functools.lru_cache(maxsize=None)
def _tiny():
    """D 64, 1 head, depth 2, ManyAR_PatchEmbed, three views stored 48 x 80 of which the second is a portrait view.  The MLP is 128 wide (mlp_ratio 2):
    the fixture holds every parameter gradient in fp64, and at mlp_ratio 4 it would be 1.17 MB, above the 1 MiB a committed file may have."""
    return ER.make_case(64, 1, 128, 2, 3, 48, 80, TRUE_SHAPE, True, 81)


@functools.lru_cache(maxsize=None)
def _mine():
    return ER.grads(_tiny(), torch.float64)


def _reference_encoder(case):
    """Output, positions and gradients of the reference's own Dust3rEncoder (fp64, CPU) on the case"""
    from oracle import ref_shims
    ref_shims.install()
    from must3r.model.encoder import Dust3rEncoder
    enc = Dust3rEncoder(img_size=(case["H"], case["W"]), patch_size=16, embed_dim=case["D"], depth=case["depth"], num_heads=case["heads"],
                        mlp_ratio=case["hidden"] / case["D"], patch_embed="ManyAR_PatchEmbed" if case["many_ar"] else "PatchEmbedDust3R", pos_embed="RoPE100").double()
    enc.load_state_dict({k: v.double() for k, v in case["params"].items()}, strict=True)
    x, pos = enc(case["img"].double(), case["true_shape"])
    x.backward(case["dy"].double().view(x.shape))
    res = dict(x=x.detach().reshape(-1, case["D"]))
    res.update({k: t.grad for k, t in enc.named_parameters()})
    return res, pos.reshape(-1, 2)


def test_yardstick_matches_the_reference_encoder():
    case = _tiny()
    mine, pos = _mine()
    assert set(mine) == {"x", *ER.param_names(2)} and pos.dtype == torch.int64
    sources = []
    if HAS_REFERENCE:
        ref, ref_pos = _reference_encoder(case)
        sources.append((ref, ref_pos))
        if os.environ.get("M3R_WRITE_ENCODER_GOLDEN"):
            np.savez_compressed(FIXTURE, pos=ref_pos.numpy(), **{k: v.numpy() for k, v in ref.items()})
    rec = np.load(FIXTURE)
    assert set(rec.files) == {"pos", *mine}
    sources.append(({k: torch.from_numpy(rec[k]) for k in mine}, torch.from_numpy(rec["pos"])))
    for source, source_pos in sources:
        assert torch.equal(pos, source_pos)
        for k, t in mine.items():
            r = source[k]
            assert r.dtype == torch.float64 and r.shape == t.shape and torch.isfinite(r).all(), k
            assert float(r.abs().max()) > 0, k
            assert torch.allclose(t, r, rtol=1e-10, atol=1e-12 * float(r.abs().max())), (k, float((t - r).abs().max()), float(r.abs().max()))


def test_fixture_is_a_committable_file():
    assert os.path.getsize(FIXTURE) <= 1 << 20


def test_portrait_view_is_the_landscape_run_on_the_swapped_image():
    case = _tiny()
    p = {k: v.double() for k, v in case["params"].items()}
    one = case["img"][1:2].double()
    xp, pp = ER.encoder(one, torch.tensor([True]), p, 1, 2)
    xl, pl = ER.encoder(one.swapaxes(-1, -2).contiguous(), None, p, 1, 2)
    assert torch.equal(xp, xl) and torch.equal(pp, pl)
    assert int(pp[:, 0].max()) == 4 and int(pp[:, 1].max()) == 2          # the swapped grid: 5 rows of 3
    # and in the batch it is the view's rows (the other views do not reach it)
    xb, pb = ER.encoder(case["img"].double(), ER.portrait_flags(case["true_shape"], True), p, 1, 2)
    assert torch.equal(pb[15:30], pp) and torch.allclose(xb[15:30], xp, rtol=0, atol=1e-13)
    assert int(pb[:15, 0].max()) == 2 and int(pb[:15, 1].max()) == 4
    # the rows themselves, element by element
    rows, _ = ER.patch_rows(case["img"], torch.tensor([False, True, False]))
    img = case["img"]
    for v, t, c, dy, dx in ((0, 7, 1, 3, 9), (2, 14, 2, 15, 0)):
        assert rows[v * 15 + t, c * 256 + dy * 16 + dx] == img[v, c, 16 * (t // 5) + dy, 16 * (t % 5) + dx]
    for t, c, dy, dx in ((7, 1, 3, 9), (14, 0, 15, 15), (2, 2, 0, 5)):
        assert rows[15 + t, c * 256 + dy * 16 + dx] == img[1, c, 16 * (t % 3) + dx, 16 * (t // 3) + dy]


def test_lds_map_of_the_turned_tile_is_injective_and_free_of_bank_conflicts():
    """The layout csrc/train_encoder.hip states for a portrait tile, replayed: lane (r, q) = (l >> 2, l & 3) writes elements (r, 4 q + j) and reads elements
    (4 q + j, r), j = 0 .. 3, one 4-byte access each; such accesses have 32 banks and the two 32-lane halves of a wave do not meet."""
    at = lambda row, col: 16 * row + 16 * (row >> 2) + (col ^ (((row >> 1) & 3) | (row & 8)))
    cells = {at(r, c) for r in range(16) for c in range(16)}
    assert len(cells) == 256 and max(cells) < 320
    padded = lambda row, col: 17 * row + col

    def worst(addr):
        ways = 0
        for j in range(4):
            for half in range(2):
                lanes = [(l >> 2, l & 3) for l in range(32 * half, 32 * half + 32)]
                for banks in ([addr(r, 4 * q + j) % 32 for r, q in lanes], [addr(4 * q + j, r) % 32 for r, q in lanes]):
                    ways = max(ways, max(banks.count(b) for b in banks))
        return ways
    assert worst(at) == 1 and worst(padded) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the ABI surface
# ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        return f.read()


def test_abi_surface_of_patch_rows():
    lib = _lib.load()
    assert lib.must3r_hip_abi_version() == _lib.ABI_VERSION == 21 and "#define MUST3R_HIP_ABI_VERSION 21" in _header()
    name = "must3r_hip_patch_rows"
    assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == (C.c_int, [C.POINTER(_lib.PatchRowsArgs)])
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == C.c_int
    # the descriptor, field by field, against the header's struct
    body = re.search(r"typedef struct must3r_hip_patch_rows_args \{(.*?)\} must3r_hip_patch_rows_args;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *more = [n.strip() for n in decl.replace("*", "* ").split(",")]
        ctype, n0 = first.rsplit(None, 1)
        size = 8 if "*" in ctype else {"int32_t": 4}[ctype]
        fields += [(n, size) for n in (n0, *more)]
    assert [n for n, _ in fields] == ["img", "transposed", "rows", "pos", "V", "H", "W", "reserved", "stream"]
    at = 0
    for n, size in fields:
        at = (at + size - 1) // size * size
        assert getattr(_lib.PatchRowsArgs, n).offset == at and getattr(_lib.PatchRowsArgs, n).size == size, n
        at += size
    assert C.sizeof(_lib.PatchRowsArgs) == at == 56
    assert re.search(r"\bint\s+must3r_hip_patch_rows\s*\(\s*const\s+must3r_hip_patch_rows_args\s*\*\s*a\s*\)\s*;", _header())


def test_no_new_entry_point_takes_a_trailing_stream():
    """tests/stream_forms.py lists the entry points with a trailing ``void* stream``; the header declares no other one (patch_rows carries its stream in the
    descriptor)"""
    import stream_forms as SF
    from test_stream_order_host import stream_entry_points
    names = stream_entry_points()
    assert "must3r_hip_patch_rows" not in names
    assert set(names) == {e for c in SF.CASES for e in c.entries} | set(SF.EXCLUDED)


def _call(**over):
    """A descriptor of fake but aligned addresses: every refusal comes before anything is read or launched"""
    lib = _lib.load()
    a = _lib.PatchRowsArgs()
    a.img, a.transposed, a.rows, a.pos = 0x100000, 0x200000, 0x300000, 0x400000
    a.V, a.H, a.W = 3, 48, 80
    for k, v in over.items():
        setattr(a, k, v)
    rc = lib.must3r_hip_patch_rows(C.byref(a))
    return rc, lib.must3r_hip_last_error().decode()


def test_patch_rows_refuses_before_touching_anything():
    lib = _lib.load()
    assert lib.must3r_hip_patch_rows(None) != 0 and "null" in lib.must3r_hip_last_error().decode()
    for over, word in ((dict(img=None), "img"), (dict(rows=None, pos=None), "outputs"), (dict(V=0), "V must"), (dict(V=-2), "V must"),
                       (dict(H=0), "multiples of 16"), (dict(H=40), "multiples of 16"), (dict(H=-16), "multiples of 16"), (dict(W=0), "multiples of 16"),
                       (dict(W=88), "multiples of 16"), (dict(W=-32), "multiples of 16"), (dict(img=0x100008), "aligned"), (dict(rows=0x300004), "aligned"),
                       (dict(pos=0x400008), "aligned"), (dict(rows=None, pos=0x400008), "aligned"), (dict(transposed=0x200002), "4-byte"),
                       (dict(V=1 << 20, H=1 << 14, W=1 << 14), "too many rows")):
        rc, msg = _call(**over)
        assert rc != 0 and word in msg, (over, msg)


def test_python_refusals():
    w, b = torch.zeros(64, 3, 16, 16), torch.zeros(64)
    img = torch.zeros(2, 3, 32, 48)
    ts = torch.tensor([[32, 48], [48, 32]])
    with pytest.raises(RuntimeError, match="GPU"):
        TE.patch_rows(img)
    with pytest.raises(RuntimeError, match="GPU"):
        TE.patch_embed(img, w, b, ts, True)
    with pytest.raises(NotImplementedError, match="image"):
        TE.patch_embed(img.clone().requires_grad_(True), w, b)
    with pytest.raises(ValueError, match="landscape"):
        TE.patch_embed(torch.zeros(2, 3, 48, 32), w, b, ts, True)
    with pytest.raises(ValueError, match="true_shape"):
        TE.patch_embed(img, w, b, None, True)
    for bad in (torch.zeros(2, 3, 40, 48), torch.zeros(2, 3, 32, 50), torch.zeros(2, 1, 32, 48), torch.zeros(3, 32, 48)):
        with pytest.raises(ValueError, match="patch_embed"):
            TE.patch_embed(bad, w, b)
    with pytest.raises(ValueError, match="weight"):
        TE.patch_embed(img, torch.zeros(64, 768), b)
    enc = TE.Dust3rEncoder(img_size=(32, 48), embed_dim=64, depth=1, num_heads=1, patch_embed="ManyAR_PatchEmbed")
    with pytest.raises(RuntimeError, match="GPU"):
        enc(img, ts)
    with pytest.raises(ValueError, match="multiples"):
        enc(torch.zeros(2, 3, 40, 48), ts)
    with pytest.raises(ValueError, match="landscape"):
        enc(torch.zeros(2, 3, 48, 32), ts)
    small = TE.Dust3rEncoder(img_size=(16, 80), embed_dim=64, depth=1, num_heads=1, npos=4)
    with pytest.raises(ValueError, match="RoPE table of 4"):
        small(torch.zeros(1, 3, 16, 80))
    with pytest.raises(RuntimeError, match="GPU"):
        small(torch.zeros(1, 3, 16, 64))                    # four positions a side fit the table: the next refusal is the device's
    for kw in (dict(patch_size=8), dict(patch_embed="PatchEmbed"), dict(precision="fp16"), dict(num_heads=3)):
        with pytest.raises(ValueError):
            TE.Dust3rEncoder(**{**dict(img_size=(32, 48), embed_dim=64, depth=1, num_heads=1), **kw})


def test_positions_checked_registers_without_reading():
    pos = torch.tensor([[0, 1], [2, 900]])
    with pytest.raises(ValueError, match="position"):
        TB.check_positions(pos, 256)
    assert TB._positions_checked(pos, 256) is pos
    assert TB.check_positions(pos, 256) is pos              # recognised: not read again
    with pytest.raises(ValueError, match="position"):
        TB.check_positions(pos, 128)                        # for another table it is read
    TB._positions_checked(pos, 256)
    pos[0, 0] = 3                                           # and so it is once it has changed
    with pytest.raises(ValueError, match="position"):
        TB.check_positions(pos, 256)


# ---------------------------------------------------------------------------------------------------------------------------------
# the module: state dict and parameter groups
# ---------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_is_the_native_encoders_and_loads_both_ways():
    cfg = TINY
    native = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads, patch_embed="ManyAR_PatchEmbed")
    g = torch.Generator().manual_seed(3)
    native.load_state_dict({k: torch.randn(v.shape, generator=g) for k, v in native.state_dict().items()}, strict=True)
    mine = TE.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads, patch_embed="ManyAR_PatchEmbed")
    sdn, sdm = native.state_dict(), mine.state_dict()
    assert list(sdn) == list(sdm) and list(sdm)[:2] == ["patch_embed.proj.weight", "patch_embed.proj.bias"]
    assert all(tuple(sdn[k].shape) == tuple(sdm[k].shape) for k in sdn) and tuple(sdm["patch_embed.proj.weight"].shape) == (cfg.enc_dim, 3, 16, 16)
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in native.named_parameters()]
    mine.load_state_dict(sdn, strict=True)
    assert all(torch.equal(mine.state_dict()[k], sdn[k]) for k in sdn)
    with torch.no_grad():
        for p in mine.parameters():
            p.add_(1.0)
    native.load_state_dict(mine.state_dict(), strict=True)
    assert all(torch.equal(native.state_dict()[k], mine.state_dict()[k]) for k in sdn)
    # from_encoder: fp32 copies of a half-precision source, which is left alone
    src = native.half()
    enc = TE.Dust3rEncoder.from_encoder(src)
    assert enc.depth == cfg.enc_depth and enc.embed_dim == cfg.enc_dim and enc.patch_embed.kind == "ManyAR_PatchEmbed" and enc.precision == "fp32"
    assert enc.blocks_enc[0].num_heads == cfg.enc_heads and enc.blocks_enc[0].rope == (float(cfg.rope_freq), float(cfg.rope_f0))
    assert all(v.dtype == torch.float32 for v in enc.state_dict().values()) and all(v.dtype == torch.float16 for v in src.state_dict().values())
    w = enc.patch_embed.proj.weight
    assert torch.equal(w, src.patch_embed.proj.weight.float()) and w.data_ptr() != src.patch_embed.proj.weight.data_ptr()
    # the dust3r checkpoint names
    renamed = {k.replace("blocks_enc", "enc_blocks").replace("norm_enc", "enc_norm"): v for k, v in mine.state_dict().items()}
    fresh = TE.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads)
    fresh.from_dust3r({**renamed, "dec_blocks.0.norm1.weight": torch.zeros(3)}, verbose=False)
    assert all(torch.equal(fresh.state_dict()[k], mine.state_dict()[k]) for k in sdn)


def test_parameter_groups_are_the_native_encoders():
    native, dec = OC.models()
    mine = TE.Dust3rEncoder.from_encoder(native)
    for (_, a), (_, b) in zip(native.named_parameters(), mine.named_parameters()):
        b.requires_grad_(a.requires_grad)
    args = OC.cases(native, dec)["encoder_0.75"][1:]
    want = OC.record(TO.get_parameter_groups, native, *args)
    assert "groups" in want and len(want["groups"]) > 4
    assert OC.record(TO.get_parameter_groups, mine, *args) == want
    args = OC.cases(native, dec)["encoder_1.0"][1:]
    assert OC.record(TO.get_parameter_groups, mine, *args) == OC.record(TO.get_parameter_groups, native, *args)


# ---------------------------------------------------------------------------------------------------------------------------------
# the driver, on CPU stub modules that log what they are called with
# ---------------------------------------------------------------------------------------------------------------------------------
class _StubEncoder:
    def __init__(self, log):
        self.log, self.w = log, torch.tensor(0.5, requires_grad=True)

    def __call__(self, img, true_shape):
        self.log.append(("enc", tuple(img.shape), tuple(true_shape.shape), torch.is_grad_enabled()))
        V, _, H, W = img.shape
        n = (H // 16) * (W // 16)
        x = img.reshape(V, 3, H // 16, 16, W // 16, 16).mean(dim=(3, 5)).reshape(V, 3, n).transpose(1, 2) * self.w
        return x.contiguous(), ER.view_rows(img[0])[1].expand(V, n, 2).contiguous()


class _StubDecoder:
    def __init__(self, log):
        self.log, self.w = log, torch.tensor(2.0, requires_grad=True)

    def __call__(self, x, pos, true_shape, mem, render=False):
        self.log.append(("dec", tuple(x.shape), tuple(pos.shape), tuple(true_shape.shape), None if mem is None else tuple(mem[0][0].shape), render,
                         torch.is_grad_enabled()))
        B, V, n, Cx = x.shape
        old = x.new_zeros((B, 0, Cx)) if mem is None else mem[0][0]
        pts = ((x.sum(dim=2) + old.sum(dim=1, keepdim=True)) * self.w).view(B, V, 1, 1, Cx).expand(B, V, 2, 3, Cx)
        if render:
            return mem, pts
        n_imgs = 0 if mem is None else mem[2]
        return ([torch.cat([old, x.reshape(B, V * n, Cx)], dim=1)], torch.zeros((B, 0), dtype=torch.int64), n_imgs + V, n_imgs + V, 0), pts


def _scene():
    g = torch.Generator().manual_seed(9)
    return torch.rand((2, 5, 3, 32, 48), generator=g), torch.tensor([32, 48]).view(1, 1, 2).expand(2, 5, 2).contiguous()


@pytest.mark.parametrize("kw", [{}, dict(to_render=[4, 0, 2]), dict(train_decoder_skip=1), dict(to_render=[])], ids=["plain", "to_render", "skip", "render_none"])
def test_driver_under_no_grad_is_the_inference_driver(kw):
    imgs, ts = _scene()
    log_a, log_b = [], []
    with torch.no_grad():
        mine = TE.inference(_StubEncoder(log_a), _StubDecoder(log_a), imgs, ts, [2, 1, 1], **kw)
    theirs = INF.inference(_StubEncoder(log_b), _StubDecoder(log_b), imgs, ts, [2, 1, 1], **kw)
    assert len(mine) == len(theirs) == 2
    for a, b in zip(mine, theirs):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    assert log_a == log_b and not any(entry[-1] for entry in log_a)
    skipped = kw.get("train_decoder_skip", 0)
    assert mine[0].shape[1] == 4 - (2 if skipped else 0) and mine[1].shape[1] == len(kw.get("to_render", range(5)))


@pytest.mark.parametrize("skip,enc_grad", [(0, False), (1, False), (2, True), (0, True), (3, False)])
def test_driver_keeps_in_the_graph_what_the_reference_keeps(skip, enc_grad):
    imgs, ts = _scene()
    log = []
    enc, dec = _StubEncoder(log), _StubDecoder(log)
    p0, p = TE.inference(enc, dec, imgs, ts, [2, 1, 1], train_decoder_skip=skip, to_render=[1, 3], encoder_requires_grad=enc_grad)
    assert [e[0] for e in log] == ["enc", "dec", "dec", "dec", "dec"]
    assert log[0] == ("enc", (10, 3, 32, 48), (10, 2), enc_grad)
    assert [e[-1] for e in log[1:]] == [b >= skip for b in range(3)] + [True]
    assert [e[1] for e in log[1:]] == [(2, 2, 6, 3), (2, 1, 6, 3), (2, 1, 6, 3), (2, 2, 6, 3)] and [e[5] for e in log[1:]] == [False, False, False, True]
    assert [e[4] for e in log[1:]] == [None, (2, 12, 3), (2, 18, 3), (2, 24, 3)]
    assert p0.shape[1] == sum([2, 1, 1][skip:]) and p.shape[1] == 2
    (p0.sum() + p.sum()).backward()
    assert dec.w.grad is not None and (enc.w.grad is not None) == enc_grad
    # the caller's no_grad wins over both switches
    with torch.no_grad():
        log.clear()
        TE.inference(enc, dec, imgs, ts, [2, 1, 1], encoder_requires_grad=True)
    assert not any(e[-1] for e in log)


def test_driver_refuses_max_bs_slicing():
    imgs, ts = _scene()
    log = []
    with pytest.raises(NotImplementedError, match="max_bs"):
        TE.inference(_StubEncoder(log), _StubDecoder(log), imgs, ts, [2, 1, 1], max_bs=4)
    assert not log
    TE.inference(_StubEncoder(log), _StubDecoder(log), imgs, ts, [2, 1, 1], max_bs=10)          # everything fits: no slicing
    assert len(log) == 5
    # the forward-only driver keeps its refusal
    with pytest.raises(NotImplementedError):
        INF.inference_encoder(_StubEncoder(log), imgs, ts.view(10, 2), requires_grad=True)
