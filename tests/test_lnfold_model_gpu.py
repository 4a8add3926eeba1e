"""GPU (-m gpu): the LN fold of the one-view update calls on (M3R_LNFOLD = 1, the default) and off against the CPU oracle, on a geometry that folds and on weights that
stress the fold.  The fold needs dec_dim = 768, so the geometry is defined here: a shallow one (encoder 256 x 2 blocks, decoder 768 x 3 blocks, 12 heads) that the oracle
runs in seconds.  run_scene(mem_batches=[2, 1, 1]): the two one-view calls fold.  The profile records prove it: with the fold on, 3 * dec_depth - 1 LayerNorm launches per
one-view call are gone (block 0's norm1 keeps its kernel: its rows come with no estimate of their mean, csrc/model.hip).

Weights: benign; two token-constant massive channels (block 0's MLP bias at 3e3, test_edge_gpu.py); a common offset added to every entry of the enc->dec embed bias, of 10
and of 40 times the sigma of the embedded tokens (computed by the oracle) -- LayerNorm removes a common offset exactly, the fold's fp16 copy of the raw rows does not.
Both settings must meet TOL[precision] wherever the unfolded run does.

Measured on an MI355X (rel-inf of the update pointmaps, 48x64, fp16w2 / fp16wa): unfolded 4.9e-4 / 5.8e-4 at the 40 sigma offset; with block 0's norm1 folded as well
(M3R_LNFOLD = 2, the behaviour before block 0 kept its kernel) 1.39e-3 / 1.27e-3 -- outside the 1e-3 target --, 6.0e-4 / 7.1e-4 at 10 sigma; with the default 4.8e-4 /
5.9e-4 and 5.1e-4 / 5.8e-4.  The massive channels cost nothing in any setting (9e-6)."""

import pytest
import torch

from must3r_amd import synthetic as S
from must3r_amd.config import ModelConfig
from util import TOL, rel_inf
from test_ops_gpu import record
from test_edge_gpu import _modules

pytestmark = pytest.mark.gpu

FOLD = ModelConfig(img_size=224, enc_dim=256, enc_depth=2, enc_heads=4, dec_dim=768, dec_depth=3, dec_heads=12)
MB = [2, 1, 1]
SIZES = {"48x64": (48, 64), "224x224": (224, 224)}
WEIGHTS = ("benign", "massive", "offset10", "offset40")
_oracle = {}


def _state_dicts(weights, imgs, ts):
    from oracle import must3r_ref as R
    sde = {k: v.clone() for k, v in S.make_encoder_state_dict(FOLD, 0).items()}
    sdd = {k: v.clone() for k, v in S.make_decoder_state_dict(FOLD, 0).items()}
    info = {}
    if weights == "massive":
        sde["blocks_enc.0.mlp.fc2.bias"][[5, 77]] = 3.0e3
        sdd["blocks_dec.0.mlp.fc2.bias"][[3, 90]] = 3.0e3
    elif weights.startswith("offset"):
        with torch.no_grad():
            xo, _ = R.encoder_forward(sde, FOLD, imgs, ts)
            emb = xo.double() @ sdd["feat_embed_enc_to_dec.weight"].double().t() + sdd["feat_embed_enc_to_dec.bias"].double()
        sigma = float(emb.std(-1, unbiased=False).mean())
        sdd["feat_embed_enc_to_dec.bias"] += float(weights[len("offset"):]) * sigma
        info = dict(sigma=sigma, kappa=float(weights[len("offset"):]))
    return sde, sdd, info


def _reference(size, weights):
    """the scene, the weights and the oracle's outputs: computed once per (size, weights), shared by the precisions, never modified"""
    key = (size, weights)
    if key not in _oracle:
        from oracle import must3r_ref as R
        H, W = SIZES[size]
        imgs, ts = S.make_images(sum(MB), H, W, 2)
        sde, sdd, info = _state_dicts(weights, imgs, ts)
        with torch.no_grad():
            upd, ren, _ = R.run_scene(sde, sdd, FOLD, imgs, ts, mem_batches=MB)
        _oracle[key] = (imgs, ts, sde, sdd, upd, ren, info)
    return _oracle[key]


def _run(enc, dec, imgs, ts, upd, ren, mode):
    from must3r_amd import _lib
    from must3r_amd.engine import run_scene
    _lib.set_option("LNFOLD", mode)
    ctx = dec._context()
    ctx.set_profiling(True)
    ctx.get_profile()
    out = run_scene(enc, dec, imgs.cuda(), ts.cuda(), mem_batches=MB)
    torch.cuda.synchronize()
    prof = ctx.get_profile()
    ctx.set_profiling(False)
    assert torch.isfinite(out["update"]).all() and torch.isfinite(out["render"]).all()
    return dict(update=rel_inf(out["update"].cpu(), upd), render=rel_inf(out["render"].cpu(), ren)), int(prof["layernorm"]["calls"])


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("precision", ["fp16w2", "fp16wa"])
@pytest.mark.parametrize("size", list(SIZES))
def test_fold_on_and_off_against_the_oracle(size, precision, weights):
    from must3r_amd import _lib
    imgs, ts, sde, sdd, upd, ren, info = _reference(size, weights)
    enc, dec = _modules(FOLD, sde, sdd, precision)
    try:
        on, ln_on = _run(enc, dec, imgs, ts, upd, ren, 1)
        off, ln_off = _run(enc, dec, imgs, ts, upd, ren, 0)
    finally:
        _lib.set_option("LNFOLD", 1)
    record("lnfold_model_ab", size=size, precision=precision, weights=weights, on=on, off=off, ln_calls=(ln_on, ln_off), **info)
    print(size, precision, weights, "LNFOLD=1", on, "LNFOLD=0", off, "LayerNorm launches", ln_on, ln_off, info)
    # the two one-view calls folded: every norm of their blocks but block 0's norm1 is gone -- the test cannot pass without folding
    assert ln_off - ln_on == 2 * (3 * FOLD.dec_depth - 1), (ln_on, ln_off)
    tol = TOL[precision]
    for k in ("update", "render"):
        if off[k] < tol:
            assert on[k] < tol, (k, on, off)
    assert weights == "massive" or max(off.values()) < tol, off     # the unfolded route itself holds the target on these weights
