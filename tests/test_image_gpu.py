"""Native image loaders on the GPU (must3r_amd.image; must3r_hip_resample) against their oracles on the CPU:

* demo path (load_images, get_resize_function's op): ImgNorm + torchvision's centre-crop rule + F.interpolate(antialias=True);
* SLAM path (preproc_frame, preprocess_frames): PIL.Image.resize + crop + ToTensor / Normalize, bit for bit;
* masks: F.interpolate(mode="nearest-exact"), bit for bit;
* batching, end to end through the native forwards, refusals.
"""
import numpy as np
import PIL.Image
import pytest
import torch
import torch.nn.functional as F

from must3r_amd import image as I
from util import TOL, rel_inf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _imgnorm(arr):
    """dust3r ImgNorm on the CPU: ToTensor (x / 255 in fp32) then Normalize(0.5, 0.5)."""
    x = torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return (x - 0.5) / 0.5


def _random(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _smooth(H, W, seed):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = np.random.default_rng(seed).uniform(0, 6.28, 3)
    chans = [127.5 + 127.5 * np.sin(x / (W / (3 + c)) + y / (H / (2 + c)) + ph[c]) for c in range(3)]
    return np.clip(np.rint(np.stack(chans, -1)), 0, 255).astype(np.uint8)


def _demo_cpu(arr, size, is_mask=False):
    """must3r/demo/inference.py:67-71 on the CPU with torchvision >= 0.17's tensor semantics."""
    H, W = arr.shape[:2]
    op, _, _ = I.get_resize_function(size, 16, H, W)
    x = _imgnorm(arr)
    if not isinstance(op, I._ResizeOp):
        return x
    top, left = int(round((H - op.crop_H) / 2.0)), int(round((W - op.crop_W) / 2.0))
    x = x[:, top:top + op.crop_H, left:left + op.crop_W]
    return F.interpolate(x[None], op.target, mode="bilinear", align_corners=False, antialias=True)[0]


def _write_png(tmp_path, name, arr):
    p = tmp_path / name
    PIL.Image.fromarray(arr).save(p, compress_level=1)
    return str(p)


DEMO_CASES = [((3024, 4032), 512), ((1080, 1920), 512), ((1000, 1000), 512), ((4032, 3024), 512), ((240, 320), 512),
              ((601, 1003), 512), ((757, 1000), 512), ((1080, 1920), 224), ((4032, 3024), 224), ((333, 997), 224)]


@pytest.mark.parametrize("shape, size", DEMO_CASES)
def test_load_images_matches_torch(tmp_path, shape, size):
    arr = _random(*shape, seed=shape[0] + size) if shape[0] % 2 else _smooth(*shape, seed=shape[1])
    (res,) = I.load_images([_write_png(tmp_path, "a.png", arr)], size, verbose=False)
    ref = _demo_cpu(arr, size)
    assert res["img"].is_cuda and res["img"].dtype == torch.float32 and tuple(res["img"].shape) == tuple(ref.shape)
    assert np.array_equal(res["true_shape"], np.int32(ref.shape[-2:]))
    assert (res["img"].cpu() - ref).abs().max().item() <= 2e-6


@pytest.mark.parametrize("shape, size", [((384, 512), 512), ((512, 384), 512), ((224, 224), 224), ((288, 512), 512)])
def test_bucket_sized_images_pass_unchanged(tmp_path, shape, size):
    arr = _random(*shape, seed=1)
    (res,) = I.load_images([_write_png(tmp_path, "b.png", arr)], size, verbose=False)
    assert torch.equal(res["img"].cpu(), _imgnorm(arr))
    x = _imgnorm(arr).to(DEV)
    op, _, _ = I.get_resize_function(size, 16, *shape)
    assert op(x) is x


@pytest.mark.parametrize("shape, size", [((1080, 1920), 512), ((601, 1003), 512), ((240, 320), 512), ((1000, 1000), 224)])
def test_resize_op_on_fp32_tensors(shape, size):
    arr = _random(*shape, seed=5)
    op, _, _ = I.get_resize_function(size, 16, *shape)
    ref = _demo_cpu(arr, size)
    got = op(_imgnorm(arr).to(DEV))
    assert (got.cpu() - ref).abs().max().item() <= 2e-6
    both = op(torch.stack([_imgnorm(arr), -_imgnorm(arr)]).to(DEV))   # [B, 3, H, W]
    assert torch.equal(both[0], got) and (both[1].cpu() - _demo_cpu(255 - arr, size)).abs().max().item() <= 2e-6


@pytest.mark.parametrize("shape, size", [((1080, 1920), 512), ((757, 1000), 512), ((240, 320), 512), ((3024, 4032), 224)])
def test_masks_nearest_exact(shape, size):
    H, W = shape
    mask = torch.from_numpy(np.random.default_rng(3).integers(0, 5, (1, H, W)).astype(np.float32))
    op, _, _ = I.get_resize_function(size, 16, H, W, is_mask=True)
    top, left = int(round((H - op.crop_H) / 2.0)), int(round((W - op.crop_W) / 2.0))
    ref = F.interpolate(mask[None, :, top:top + op.crop_H, left:left + op.crop_W], op.target, mode="nearest-exact")[0]
    assert torch.equal(op(mask.to(DEV)).cpu(), ref)


def _slam_cpu(arr, res):
    """must3r/slam/model.py:99-120 with dust3r's _resize_pil_image, on the CPU with Pillow."""
    img = PIL.Image.fromarray(arr)
    W1, H1 = img.size
    longsize = max(W1, H1) / min(W1, H1) * res if res in (224, 336, 448) else res
    S = max(img.size)
    interp = PIL.Image.LANCZOS if S > longsize else PIL.Image.BICUBIC
    img = img.resize(tuple(int(round(x * longsize / S)) for x in img.size), interp)
    W, H = img.size
    cx, cy = W // 2, H // 2
    halfw, halfh = (res // 2, res // 2) if res in (224, 336, 448) else (((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8)
    img = img.crop((cx - halfw, cy - halfh, cx + halfw, cy + halfh))
    return _imgnorm(np.asarray(img))[None], np.int32([[cx - halfw, cy - halfh]]), W1 / W


@pytest.mark.parametrize("res", [512, 224])
@pytest.mark.parametrize("shape", [(1080, 1920), (1920, 1080), (480, 640), (240, 320), (721, 1283)])
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_preproc_frame_bit_exact_with_pil(shape, res, kind):
    arr = (_random if kind == "random" else _smooth)(*shape, seed=shape[1] + res)
    ref, offset, focal = _slam_cpu(arr, res)
    for src in (arr, torch.from_numpy(arr).to(DEV)):
        view, to_orig_focal = I.preproc_frame(src, 7, res=res)
        assert torch.equal(view["img"].cpu(), ref)
        assert np.array_equal(view["true_shape"], np.int32([ref.shape[-2:]])) and np.array_equal(view["offset"], offset)
        assert view["idx"] == 7 and view["instance"] == "7" and to_orig_focal == focal


def test_preproc_frame_with_the_reference_call_signature():
    # slam/model.py:482: preproc_frame(img, frame_id, res=self.res, transform=self.transform), self.transform = dust3r's ImgNorm
    from test_image_host import DUST3R_IMGNORM
    arr = _smooth(1080, 1920, 4)
    ref, offset, focal = _slam_cpu(arr, 512)
    for transform in (DUST3R_IMGNORM, I.ImgNorm, None):
        view, to_orig_focal = I.preproc_frame(arr, 11, res=512, transform=transform)
        assert torch.equal(view["img"].cpu(), ref) and np.array_equal(view["offset"], offset) and to_orig_focal == focal
    with pytest.raises(ValueError, match="ImgNorm"):
        I.preproc_frame(arr, 11, res=512, transform=lambda im: im)


def test_load_images_in_chunks_equals_one_call(tmp_path, monkeypatch):
    shapes = [(3024, 4032), (384, 512), (1080, 1920), (601, 1003), (240, 320)]
    paths = [_write_png(tmp_path, f"c{i}.png", _random(*s, seed=10 + i)) for i, s in enumerate(shapes)]
    together = I.load_images(paths, 512, verbose=False)
    for limit in (1, 8 << 20):   # one file per call; then chunks of 1, 3 and 1 files
        monkeypatch.setattr(I, "LOAD_CHUNK_BYTES", limit)
        chunked = I.load_images(paths, 512, verbose=False)
        assert len(chunked) == len(paths)
        for a, b in zip(together, chunked):
            assert torch.equal(a["img"], b["img"]) and np.array_equal(a["true_shape"], b["true_shape"])


def test_preprocess_frames_batch_equals_single_calls():
    frames = torch.from_numpy(np.stack([_random(1080, 1920, s) if s % 2 else _smooth(1080, 1920, s) for s in range(64)])).to(DEV)
    batch, true_shape = I.preprocess_frames(frames, res=512)
    assert tuple(batch.shape) == (64, 3, 288, 512) and np.array_equal(true_shape, np.int32([[288, 512]] * 64))
    for b in range(64):
        assert torch.equal(batch[b:b + 1], I.preproc_frame(frames[b], b, res=512)[0]["img"]), b
    ref, _, _ = _slam_cpu(frames[5].cpu().numpy(), 512)
    assert torch.equal(batch[5:6].cpu(), ref)


def test_load_images_mixed_sizes_one_call_equals_single_calls(tmp_path):
    shapes = [(3024, 4032), (384, 512), (1080, 1920), (240, 320), (1000, 1000), (4032, 3024), (601, 1003)]
    paths = [_write_png(tmp_path, f"{i}.png", _random(*s, seed=i)) for i, s in enumerate(shapes)]
    together = I.load_images(paths, 512, verbose=False)
    for p, t in zip(paths, together):
        (alone,) = I.load_images([p], 512, verbose=False)
        assert torch.equal(t["img"], alone["img"]) and np.array_equal(t["true_shape"], alone["true_shape"])


def test_end_to_end_png_to_pointmaps(tmp_path):
    from must3r_amd import synthetic as S
    from must3r_amd.config import SMALL
    from must3r_amd.engine import run_scene
    import must3r_amd.model as M
    from oracle import must3r_ref as R

    cfg = SMALL
    arrs = [_smooth(480, 640, 0), _random(700, 700, 1), _smooth(1080, 1920, 2)]
    paths = [_write_png(tmp_path, f"v{i}.png", a) for i, a in enumerate(arrs)]
    views = I.load_images(paths, 224, verbose=False)
    imgs = torch.stack([v["img"] for v in views])
    ts = torch.from_numpy(np.stack([v["true_shape"] for v in views]).astype(np.int64))
    cpu_imgs = torch.stack([_demo_cpu(a, 224) for a in arrs])
    assert (imgs.cpu() - cpu_imgs).abs().max().item() <= 2e-6
    sde, sdd = S.make_encoder_state_dict(cfg, 0), S.make_decoder_state_dict(cfg, 0)
    enc = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads)
    dec = M.MUSt3R(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth,
                   num_heads=cfg.dec_heads, feedback_type="single_mlp", memory_mode="kv")
    enc.load_state_dict(sde)
    dec.load_state_dict(sdd)
    enc, dec = enc.to(DEV).eval(), dec.to(DEV).eval()
    out = run_scene(enc, dec, imgs, ts.to(DEV))
    torch.cuda.synchronize()
    with torch.no_grad():
        upd, ren, _ = R.run_scene(sde, sdd, cfg, cpu_imgs, ts)
    tol = TOL["fp16wa"] if dec.precision == "fp16wa" else TOL["fp16w2"]
    assert rel_inf(out["update"].cpu(), upd) < tol and rel_inf(out["render"].cpu(), ren) < tol


def test_refusals():
    arr = _random(64, 96, 0)
    op, _, _ = I.get_resize_function(512, 16, 64, 96)
    with pytest.raises(RuntimeError, match="CUDA"):
        op(_imgnorm(arr))
    with pytest.raises(ValueError, match="fp32"):
        op(_imgnorm(arr).to(DEV).half())
    with pytest.raises(RuntimeError, match="CUDA"):
        I.preprocess_frames(torch.from_numpy(np.stack([arr])), res=512)
    with pytest.raises(ValueError, match="uint8"):
        I.preprocess_frames(torch.from_numpy(np.stack([arr])).to(DEV).float(), res=512)
    with pytest.raises(ValueError, match="uint8"):
        I.preproc_frame(arr.astype(np.float32), 0)
    with pytest.raises(ValueError, match="empty"):
        I.preprocess_frames(torch.zeros((1, 0, 96, 3), dtype=torch.uint8, device=DEV), res=512)
    with pytest.raises(ValueError, match="HxWx3"):
        I.preproc_frame(np.zeros((0, 96, 3), np.uint8), 0)
    with pytest.raises(ValueError, match="patch size"):
        I.get_resize_function(512, 14, 1080, 1920)
    with pytest.raises(RuntimeError, match="CUDA"):
        I.load_images([], 512, device="cpu")
