"""Image ingestion throughput (must3r_amd.image) on the GPU against the reference's CPU path, in one run.

Workloads
  stream : 200 frames of 1920x1080 uint8 -> preprocess_frames(res=512) in chunks (the SLAM agent's preproc_frame, PIL LANCZOS)
  frame  : the same frames one at a time through preproc_frame(numpy frame) as the SLAM agent calls it, each result waited for
  folder : 20 JPEGs of 4032x3024 -> load_images(size=512) (the demo's loader, antialiased bilinear)

Reported per workload (one JSON line each): frames/s of the native path (H2D upload of the uint8 pixels + resample, device events),
the resample time alone, the upload time alone, the bytes the resampler must move (source bytes it reads + intermediate written and read +
fp32 output) and that over the resample time as a fraction of 6.3 TB/s, and the CPU path (PIL / torch on <= 16 threads) timed in the
same run.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` (a separate run; --quick shortens it).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import PIL.Image
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from must3r_amd import image as I  # noqa: E402

HBM = 6.3e12


def _imgnorm(arr):
    x = torch.from_numpy(arr).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return (x - 0.5) / 0.5


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _resample_bytes(H1, W1, rows, out_h, out_w, inter_bytes):
    """source rows the horizontal pass reads + intermediate (written once, read once) + fp32 output, per image"""
    return rows * W1 * 3 + 2 * 3 * rows * out_w * inter_bytes + 3 * out_h * out_w * 4


def bench_stream(n_frames, chunk, reps, cpu_frames):
    H1, W1 = 1080, 1920
    rng = np.random.default_rng(0)
    host = torch.from_numpy(rng.integers(0, 256, (n_frames, H1, W1, 3), dtype=np.uint8)).pin_memory()
    dev = torch.empty(host.shape, dtype=torch.uint8, device="cuda")
    for c0 in range(0, n_frames, chunk):   # warm-up: every chunk shape of the timed window
        dev[c0:c0 + chunk].copy_(host[c0:c0 + chunk], non_blocking=True)
        I.preprocess_frames(dev[c0:c0 + chunk], res=512)
    torch.cuda.synchronize()
    up_ms = rs_ms = tot_ms = 0.0
    for _ in range(reps):
        for c0 in range(0, n_frames, chunk):
            e0, e1 = _events()
            e2 = torch.cuda.Event(enable_timing=True)
            e0.record()
            dev[c0:c0 + chunk].copy_(host[c0:c0 + chunk], non_blocking=True)
            e1.record()
            out, _ = I.preprocess_frames(dev[c0:c0 + chunk], res=512)
            e2.record()
            torch.cuda.synchronize()
            up_ms += e0.elapsed_time(e1)
            rs_ms += e1.elapsed_time(e2)
            tot_ms += e0.elapsed_time(e2)
    frames = n_frames * reps
    mode, (H, W), (y0, x0, h, w), _ = I._frame_geometry(H1, W1, 512)
    bounds, _ = I.resample_coeffs(mode, H1, H)
    rows = int(bounds[y0 + h - 1].sum() - bounds[y0, 0])
    nbytes = _resample_bytes(H1, W1, rows, h, w, 1) * frames
    # the reference's path on the CPU: PIL LANCZOS resize + crop + ImgNorm, one frame at a time
    t0 = time.perf_counter()
    for i in range(cpu_frames):
        arr = host[i].numpy()
        img = PIL.Image.fromarray(arr).resize((W, H), PIL.Image.LANCZOS).crop((x0, y0, x0 + w, y0 + h))
        _imgnorm(np.asarray(img))
    cpu_s = (time.perf_counter() - t0) / cpu_frames
    return dict(workload="stream_1920x1080_to_512x288", frames=frames, chunk=chunk,
                native_frames_per_s=frames / (tot_ms / 1e3), resample_ms_per_frame=rs_ms / frames, upload_ms_per_frame=up_ms / frames,
                upload_GBps=n_frames * reps * H1 * W1 * 3 / (up_ms / 1e3) / 1e9,
                resample_bytes_per_frame=nbytes / frames, resample_TBps=nbytes / (rs_ms / 1e3) / 1e12,
                fraction_of_6p3TBps=nbytes / (rs_ms / 1e3) / HBM,
                cpu_frames_per_s=1.0 / cpu_s, cpu_threads=1)   # PIL's resize runs on one thread


def bench_frame(n_frames, cpu_frames):
    """preproc_frame per frame from a numpy array (pinned upload + one native call + the result waited for): host wall clock"""
    H1, W1 = 1080, 1920
    frames = np.random.default_rng(2).integers(0, 256, (n_frames, H1, W1, 3), dtype=np.uint8)
    for i in range(4):   # warm-up
        I.preproc_frame(frames[i], i, res=512)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_frames):
        I.preproc_frame(frames[i], i, res=512)
        torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / n_frames
    _, (H, W), (y0, x0, h, w), _ = I._frame_geometry(H1, W1, 512)
    t0 = time.perf_counter()
    for i in range(cpu_frames):
        img = PIL.Image.fromarray(frames[i]).resize((W, H), PIL.Image.LANCZOS).crop((x0, y0, x0 + w, y0 + h))
        _imgnorm(np.asarray(img))
    cpu_s = (time.perf_counter() - t0) / cpu_frames
    return dict(workload="frame_1920x1080_to_512x288_one_at_a_time", frames=n_frames, native_frames_per_s=1.0 / per,
                native_ms_per_frame=per * 1e3, cpu_frames_per_s=1.0 / cpu_s, cpu_threads=1)


def bench_folder(n_files, reps, cpu_files):
    H1, W1 = 3024, 4032
    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp()
    y, x = np.mgrid[0:H1, 0:W1]
    noise = rng.normal(0, 12, (H1, W1, 3)).astype(np.float32)
    paths = []
    for i in range(n_files):   # smooth content plus noise: JPEG sizes close to a photo's
        base = (127 + 100 * np.sin(x / (300 + 17 * i) + y / 500)).astype(np.float32)[..., None] + noise
        p = os.path.join(tmp, f"{i:02d}.jpg")
        PIL.Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).save(p, quality=90)
        paths.append(p)
    I.load_images(paths, 512, verbose=False)   # warm-up
    torch.cuda.synchronize()
    wall = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        I.load_images(paths, 512, verbose=False)
        torch.cuda.synchronize()
        wall += time.perf_counter() - t0
    # the native part alone: uint8 pixels already decoded, upload + one resample call, device events
    arrs = [np.asarray(PIL.Image.open(p).convert("RGB")) for p in paths]
    pinned = [torch.from_numpy(a).pin_memory() for a in arrs]
    dev = [torch.empty(a.shape, dtype=torch.uint8, device="cuda") for a in arrs]
    target, crop_H, crop_W, _, _ = I._geometry(512, 16, H1, W1)
    h, w = target
    top, left = I._center_offsets(H1, W1, crop_H, crop_W)
    out = torch.empty((n_files * 3 * h * w,), dtype=torch.float32, device="cuda")

    def native():
        descs = [I._desc(d, I._lib.IMG_U8_HWC, 3, H1, W1, W1 * 3, 0, (top, left, crop_H, crop_W), (h, w), (0, 0, h, w), i * 3 * h * w)
                 for i, d in enumerate(dev)]
        I._resample(I._lib.RESAMPLE_AA_BILINEAR, descs, out, dev)

    native()
    up_ms = rs_ms = 0.0
    for _ in range(reps):
        e0, e1 = _events()
        e2 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for d, p in zip(dev, pinned):
            d.copy_(p, non_blocking=True)
        e1.record()
        native()
        e2.record()
        torch.cuda.synchronize()
        up_ms += e0.elapsed_time(e1)
        rs_ms += e1.elapsed_time(e2)
    bounds, _ = I.resample_coeffs(I._lib.RESAMPLE_AA_BILINEAR, crop_H, h)
    rows = int(bounds[-1].sum() - bounds[0, 0])
    nbytes = _resample_bytes(H1, crop_W, rows, h, w, 4) * n_files * reps
    frames = n_files * reps
    # the reference's path on the CPU: PIL decode + ImgNorm + centre crop + antialiased interpolate
    t0 = time.perf_counter()
    for p in paths[:cpu_files]:
        xim = _imgnorm(np.asarray(PIL.Image.open(p).convert("RGB")))[:, top:top + crop_H, left:left + crop_W]
        F.interpolate(xim[None], (h, w), mode="bilinear", align_corners=False, antialias=True)
    cpu_s = (time.perf_counter() - t0) / cpu_files
    shutil.rmtree(tmp, ignore_errors=True)
    return dict(workload="folder_20_jpeg_4032x3024_to_512x384", files=n_files, reps=reps,
                load_images_files_per_s=frames / wall, native_files_per_s=frames / ((up_ms + rs_ms) / 1e3),
                resample_ms_per_file=rs_ms / frames, upload_ms_per_file=up_ms / frames,
                resample_bytes_per_file=nbytes / frames, resample_TBps=nbytes / (rs_ms / 1e3) / 1e12, fraction_of_6p3TBps=nbytes / (rs_ms / 1e3) / HBM,
                cpu_files_per_s=1.0 / cpu_s, cpu_threads=torch.get_num_threads())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="short run (for the kernel trace)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image.py needs a GPU")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    reps = 1 if a.quick else 5
    rows = [bench_stream(200, 50, reps, 4 if a.quick else 20), bench_frame(20 if a.quick else 200, 4 if a.quick else 20), bench_folder(20, 1 if a.quick else 3, 2 if a.quick else 5)]
    for r in rows:
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
