"""GPU (-m gpu): the launch structure of the two native forwards (csrc/model.hip: encode_chunk, decode_impl), read from the profile records.  No golden file: the
class rows of ``get_profile()`` must carry exactly the call counts that the model's structure dictates, written below as formulas in the depths, the views, the
groups and the call's flags.  A sublayer launched twice, a LayerNorm that the fold should have removed, a projection of the memory issued in the wrong mode: each
moves a count.

Geometry of tests/test_lnfold_model_gpu.py (encoder 256 x 2 blocks, decoder 768 x 3 blocks, 12 heads: the one-view update folds), 48 x 64 images (12 tokens per
view), the schedule [2, 1, 1].  With at most 60 keys per view the cross attention has fewer than 8 key tiles of 64, so attention_pick_split never splits and
``attn_combine`` stays at 0; the e4m3 path is not built, so ``misc`` holds only the encoder's im2col scope and the decoder's token casts."""

import pytest
import torch

from must3r_amd import synthetic as S
from test_edge_gpu import _modules
from test_lnfold_model_gpu import FOLD, MB

pytestmark = pytest.mark.gpu

H, W = 48, 64
ROWS = ("gemm", "attn_self", "attn_cross", "attn_combine", "layernorm", "misc")
_scene = {}


def encoder_counts(depth, chunks=1):
    """per chunk: one scope around fill_pos + im2col; the patch embedding; per block norm1, qkv, attention, proj, norm2, fc1, fc2; norm_enc"""
    return dict(gemm=chunks * (1 + 4 * depth), attn_self=chunks * depth, attn_cross=0, attn_combine=0, layernorm=chunks * (2 * depth + 1), misc=chunks)


def decoder_counts(depth, views, n_mem, render=False, mode="kv", fold=False, groups=1, scenes=1, feedback="single_mlp"):
    """one decode call over ``views`` views per scene against ``n_mem`` memory rows"""
    L, update = depth, not render
    lone_view = update and views == 1 and n_mem > 0          # own tokens excluded: the keys are the old memory alone
    pre_kv = update and not lone_view                        # the pre-feedback K|V of the new tokens are attended
    launches = groups * (1 if groups == 1 else scenes)       # one group: all scenes in one cast / one head launch
    gemm = 1                                                 # enc -> dec embedding
    gemm += 6 * L                                            # qkv, proj, projq, cross proj, fc1, fc2
    ln = 1 if fold else 3 * L                                # norm1 / norm2 / norm3; folded: only block 0's norm1 keeps its kernel
    if pre_kv:                                               # prepare_y of the new rows in front of every block
        gemm += L if mode == "kv" else 0
        ln += L if mode == "kv" else L * scenes              # 'norm_y' / 'raw': the LayerNorm writes each scene's memory rows itself
    if mode != "kv":                                         # kv_source: the attended rows are projected per block, per scene
        gemm += L * scenes
        ln += L * scenes if mode == "raw" else 0
    gemm += launches                                         # head
    ln += 1
    if update:
        if feedback:
            ln += 1
            gemm += 2 if feedback == "single_mlp" else 1
        if mode == "kv":                                     # one grouped LayerNorm and one grouped K|V projection over all layers
            ln += 1
            gemm += 1
        else:
            ln += L * scenes
    return dict(gemm=gemm, attn_self=L, attn_cross=L, attn_combine=0, layernorm=ln, misc=launches)


def _setup(precision):
    if precision not in _scene:
        imgs, ts = S.make_images(sum(MB), H, W, 2)
        enc, dec = _modules(FOLD, S.make_encoder_state_dict(FOLD, 0), S.make_decoder_state_dict(FOLD, 0), precision)
        x, pos = enc(imgs.cuda(), ts)
        _scene[precision] = (enc, dec, imgs.cuda(), ts, x, pos)
    return _scene[precision]


def _profiled(ctx, fn):
    ctx.set_profiling(True)
    try:
        ctx.get_profile()
        out = fn()
        torch.cuda.synchronize()
        prof = ctx.get_profile()
    finally:
        ctx.set_profiling(False)
    got = {k: int(prof[k]["calls"]) for k in ROWS[1:]}
    got["gemm"] = int(prof["gemm128"]["calls"]) + int(prof["gemm64"]["calls"])
    return out, got


def _decode(dec, x, pos, ts, i, n, mem, **kw):
    return dec(x[i:i + n].unsqueeze(0), pos[i:i + n].unsqueeze(0), ts[i:i + n].unsqueeze(0), mem, **kw)


def _check(got, want, what):
    print(what, "launches", got, "expected", want)
    assert got == want, (what, got, want)


def test_encoder_call():
    enc, _, imgs, ts, _, _ = _setup("fp16wa")
    _, got = _profiled(enc._context(), lambda: enc(imgs, ts))
    _check(got, encoder_counts(FOLD.enc_depth), "encoder, 4 views")


@pytest.mark.parametrize("precision", ["fp16wa", "bf16"])
def test_first_decoder_call(precision):
    _, dec, _, ts, x, pos = _setup(precision)
    (mem, pm), got = _profiled(dec._context(), lambda: _decode(dec, x, pos, ts, 0, 2, None))
    assert torch.isfinite(pm).all()
    _check(got, decoder_counts(FOLD.dec_depth, 2, 0), f"first call, 2 views, {precision}")


@pytest.mark.parametrize("lnfold", [1, 0])
def test_one_view_update(lnfold):
    from must3r_amd import _lib
    _, dec, _, ts, x, pos = _setup("fp16wa")
    mem, _ = _decode(dec, x, pos, ts, 0, 2, None)
    try:
        _lib.set_option("LNFOLD", lnfold)
        (_, pm), got = _profiled(dec._context(), lambda: _decode(dec, x, pos, ts, 2, 1, mem))
    finally:
        _lib.set_option("LNFOLD", 1)
    assert torch.isfinite(pm).all()
    _check(got, decoder_counts(FOLD.dec_depth, 1, 24, fold=bool(lnfold)), f"one-view update, LNFOLD={lnfold}")


def test_render():
    _, dec, _, ts, x, pos = _setup("fp16wa")
    mem, i = None, 0
    for n in MB:
        mem, _ = _decode(dec, x, pos, ts, i, n, mem)
        i += n
    (_, pm), got = _profiled(dec._context(), lambda: _decode(dec, x, pos, ts, 0, sum(MB), mem, render=True))
    assert torch.isfinite(pm).all()
    _check(got, decoder_counts(FOLD.dec_depth, sum(MB), 48, render=True), "render, 4 views")


@pytest.mark.parametrize("mode", ["norm_y", "raw"])
def test_one_view_update_in_the_token_memory_modes(mode):
    _, dec, _, ts, x, pos = _setup("fp16wa")
    try:
        dec.change_memory_mode(mode)
        mem, _ = _decode(dec, x, pos, ts, 0, 2, None)
        (_, pm), got = _profiled(dec._context(), lambda: _decode(dec, x, pos, ts, 2, 1, mem))
    finally:
        dec.change_memory_mode("kv")
    assert torch.isfinite(pm).all()
    # (the fold does not depend on the memory mode: a lone view against an existing memory folds here as well)
    _check(got, decoder_counts(FOLD.dec_depth, 1, 24, mode=mode, fold=True), f"one-view update, memory_mode {mode}")
