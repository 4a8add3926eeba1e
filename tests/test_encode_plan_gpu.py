"""GPU: the encoder on the chunk sizes of must3r_amd/csrc/encode_plan.hpp.  Chunks of one call may now differ in size, and the benched step runs 42-view chunks
(126 row blocks of 256) where it ran 40-view ones.  A change of chunk size keeps every k-ascending accumulator chain of every kernel, so tokens and positions are
asserted bit for bit (torch.equal), never by a tolerance."""
import pytest
import torch

from must3r_amd import _lib
from must3r_amd import synthetic as S
from must3r_amd.config import MUST3R_512, SMALL
from test_model_gpu import build

pytestmark = pytest.mark.gpu

ENC_CHUNK_ROWS_DEFAULT = 32768    # misc.hip kOpts
ENC_CHUNK_ROWS_MIN = 256


@pytest.mark.parametrize("precision", ["fp16wa", "bf16"])
def test_ragged_chunks_equal_one_view_per_call(precision):
    """7 views of 96 x 128 (48 tokens each) under the smallest cap the option accepts (256 rows = 5 views): the plan is 4 + 3 (tests/c/encode_plan_check.cpp asserts
    that), two chunks of different size in one call -- each sizes its own workspace, view table and positions.  Against the same views encoded one per call."""
    V, H, W = 7, 96, 128
    enc, _ = build(SMALL, precision)
    imgs, ts = S.make_images(V, H, W, 5)
    imgs_c, ts_c = imgs.cuda(), ts.cuda()
    try:
        _lib.set_option("ENC_CHUNK_ROWS", ENC_CHUNK_ROWS_MIN)
        x, pos = enc(imgs_c, ts_c)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("ENC_CHUNK_ROWS", ENC_CHUNK_ROWS_DEFAULT)
    one = [enc(imgs_c[v:v + 1], ts_c[v:v + 1]) for v in range(V)]
    x1, pos1 = torch.cat([o[0] for o in one]), torch.cat([o[1] for o in one])
    whole, _ = enc(imgs_c, ts_c)      # and the default cap: one chunk of 7 views
    torch.cuda.synchronize()
    assert x.shape == (V, 48, SMALL.enc_dim) and bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
    assert torch.equal(pos, pos1) and pos[V - 1].max(0).values.tolist() == [H // 16 - 1, W // 16 - 1]
    bad = [v for v in range(V) if not torch.equal(x[v], x1[v])]
    assert not bad, f"views {bad} differ between the 4 + 3 chunks and one view per call"
    assert torch.equal(whole, x1)


def _encode(enc, imgs, ts):
    x, pos = enc(imgs, ts)
    torch.cuda.synchronize()
    return x, pos


def test_full_size_42_view_chunk_equals_its_first_views_alone():
    """One 42-view chunk of 384 x 512 at the MUST3R_512 widths (32256 rows = 126 row blocks: the launches the step now runs) against views 0-1 encoded alone
    (1536 rows: the small-M kernels).

    bf16, and fp16wa with SPARSE_LO = 0: every Linear of both calls multiplies the same weight values, so the rows of views 0-1 are equal bit for bit.
    fp16wa at the default options: the chip-filling qkv and proj multiply the 2:4-sparse low part of their split weights and the small-M kernels the dense one
    (gemm_route.hpp; tests/test_model_gpu.py test_sparse_low_part_batch_dependence_is_bounded bounds that difference, which is the precision mode's and not the chunk
    size's), so there the 42-view chunk is held bit for bit to a 40-view chunk, the size of before, which takes the same kernels at 120 row blocks."""
    cfg, H, W, V = MUST3R_512, 384, 512, 42
    imgs, ts = S.make_images(V, H, W, 7)
    imgs_c, ts_c = imgs.cuda(), ts.cuda()
    enc, _ = build(cfg, "bf16")
    x42, p42 = _encode(enc, imgs_c, ts_c)
    x2, p2 = _encode(enc, imgs_c[:2], ts_c[:2])
    assert x42.shape == (V, 768, cfg.enc_dim) and bool(torch.isfinite(x42).all())
    assert torch.equal(p42[:2], p2) and torch.equal(x42[:2], x2), "bf16: views 0-1 of the 42-view chunk differ from the two views alone"
    del x42, x2

    enc, _ = build(cfg, "fp16wa")
    x42, p42 = _encode(enc, imgs_c, ts_c)
    x40, p40 = _encode(enc, imgs_c[:40], ts_c[:40])
    assert bool(torch.isfinite(x42).all()) and torch.equal(p42[:40], p40)
    bad = [v for v in range(40) if not torch.equal(x42[v], x40[v])]
    assert not bad, f"fp16wa: views {bad} of the 42-view chunk differ from the 40-view chunk"
    del x40
    try:
        _lib.set_option("SPARSE_LO", 0)
        d42, _ = _encode(enc, imgs_c, ts_c)
        d2, _ = _encode(enc, imgs_c[:2], ts_c[:2])
    finally:
        _lib.set_option("SPARSE_LO", 1)
    assert torch.equal(d42[:2], d2), "fp16wa, dense low part: views 0-1 of the 42-view chunk differ from the two views alone"
    assert not torch.equal(d42[:2], x42[:2]), "SPARSE_LO = 0 changed nothing: the default run was not on the sparse kernels"
