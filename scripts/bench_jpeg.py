"""The JPEG decoder on the device (csrc/jpeg.hip; must3r_amd.jpeg) beside Pillow on the host, on one GPU and the same machine in one run.  One JSON line per
file form (append them to profiles/jpeg_bench.jsonl; ``--out`` does).

The workload is ``--frames`` (200) synthetic ``--width`` x ``--height`` (1920 x 1080) frames -- a smooth field plus noise, shifted per frame -- encoded by Pillow
at quality 90, in four forms: 4:2:0 and 4:4:4, each without restart markers and with one per MCU row.  Per form, alternated inside every round:

  (a) ``jpeg.decode_images`` on the 200 byte strings: parse, pinned upload of the compressed bytes, the launches; host clock around a synchronise.
  (b) Pillow, ``Image.open(BytesIO).convert("RGB")`` + ``load()``, on 1 host thread and on ``--threads`` (16), then the upload ``load_images`` uses for every frame
      (pinned, asynchronous) and one synchronise: upload included on both sides.
  (c) one frame alone through (a), its result waited for: the latency.
  (d) ``image.load_images`` on the same frames as files, ``decode="gpu"`` against ``decode="pil"`` (512 buckets).
  (e) one round of (a) under torch's profiler: device time per kernel of the decoder (absent when the profiler gives no device events).

``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402
from must3r_amd import image as IM, jpeg  # noqa: E402

DEV = "cuda:0"
FORMS = (("420", None), ("420", "rows"), ("444", None), ("444", "rows"))


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _pillow_one(data):
    import PIL.Image
    im = PIL.Image.open(io.BytesIO(data)).convert("RGB")
    im.load()
    return np.asarray(im)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg: needs a GPU (no CPU fallback)")
    base = [R.synthetic(args.width, args.height, 10 + i, noise=6.0) for i in range(4)]
    frames = [np.roll(base[i % 4], (7 * i, 13 * i), (0, 1)) for i in range(args.frames)]
    pool = ThreadPoolExecutor(args.threads)
    dev = torch.device(DEV)
    lines = []
    for sampling, restart in FORMS:
        datas = list(pool.map(lambda f: R.encode(f, sampling=sampling, quality=90, restart=restart), frames))
        want = _pillow_one(datas[3])
        jpeg.reset_path_record()
        (got,) = jpeg.decode_images([datas[3]], DEV)
        assert np.array_equal(got.cpu().numpy(), want), "the decoder is not bit-equal to Pillow on this form"

        def native():
            return jpeg.decode_images(datas, DEV)

        def pillow(threads):
            arrs = list(pool.map(_pillow_one, datas)) if threads > 1 else [_pillow_one(d) for d in datas]
            return [IM._upload_u8(a, dev) for a in arrs]

        with tempfile.TemporaryDirectory() as tmp:
            files = []
            for i, d in enumerate(datas):
                files.append(os.path.join(tmp, f"{i:04d}.jpg"))
                with open(files[-1], "wb") as f:
                    f.write(d)
            t = {k: [] for k in ("native", "pillow_1", "pillow_n", "single", "load_gpu", "load_pil")}
            for r in range(args.warmup + args.rounds):
                row = dict(native=_timed(native), pillow_n=_timed(lambda: pillow(args.threads)), single=_timed(lambda: jpeg.decode_images([datas[r % len(datas)]], DEV)),
                           pillow_1=_timed(lambda: pillow(1)), load_gpu=_timed(lambda: IM.load_images(files, 512, verbose=False, decode="gpu")),
                           load_pil=_timed(lambda: IM.load_images(files, 512, verbose=False, decode="pil")))
                if r >= args.warmup:
                    for k, v in row.items():
                        t[k].append(v)
        kernels = None
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                native()
                torch.cuda.synchronize()
            kernels = {}
            for e in prof.key_averages():
                us = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                if "jpeg_" in e.key and us:
                    kernels[e.key.split("(")[0].split("::")[-1]] = dict(us=float(us), calls=int(e.count))
            kernels = kernels or None
        except Exception as e:      # noqa: BLE001
            kernels = dict(error=repr(e))
        paths = jpeg.path_record()
        n = len(datas)
        rec = dict(figure="jpeg_decode", frames=n, width=args.width, height=args.height, sampling=sampling, restart=restart or "none", quality=90,
                   file_bytes_mean=float(np.mean([len(d) for d in datas])), host_threads=args.threads, paths=paths,
                   conditions="clocks not pinned, shared machine; medians with min and max; forms alternated inside every round; host clock around a synchronise; "
                              "upload included on both sides; Pillow with libjpeg-turbo on this machine's CPU",
                   native_batch=_stats(t["native"], unit="s"), pillow_1_thread=_stats(t["pillow_1"], unit="s"), pillow_n_threads=_stats(t["pillow_n"], unit="s"),
                   single_frame=_stats(t["single"], unit="s"), load_images_gpu=_stats(t["load_gpu"], unit="s"), load_images_pil=_stats(t["load_pil"], unit="s"),
                   kernels_one_round=kernels)
        rec["frames_per_s"] = {k: n / rec[k]["median"] for k in ("native_batch", "pillow_1_thread", "pillow_n_threads")}
        rec["batch_beats_pillow_n_threads_beyond_the_spreads"] = rec["native_batch"]["max"] < rec["pillow_n_threads"]["min"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
