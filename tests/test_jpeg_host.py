"""No GPU: the JPEG decoder's yardstick, parser and per-thread routine (tests/jpeg_ref.py; must3r_amd/csrc/jpeg_parse.hpp, jpeg_entropy.hpp; must3r_amd.jpeg).

1. tests/jpeg_ref.py, the numpy restatement of the whole decode, is bit-equal to Pillow over the corpus (every size of {1, 7, 8, 9, 16, 17, 33}^2 and 48 x 64 with
   the three samplings and grey; qualities 30 / 75 / 95 / 100, optimize on / off, restart_marker_blocks=1 / restart_marker_rows=1 rotating over them).
2. A planted defect in each stage breaks that equality.
3. The parser against Pillow's own size, mode, layers and sampling, and its refusals -- each with a reason, none with an exception from C.
4. tests/c/jpeg_check.cpp, a stand-alone program built with -fsanitize=address,undefined and run as a child process with nothing preloaded: the parser and the
   routine the kernels run, sequentially and by the subsequence scheme emulated on the host, over the corpus and over damaged variants of it.
"""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_ref as R
from conftest import ROOT
from must3r_amd import _lib, jpeg


def _noise(seed=5, size=(480, 640)):
    return np.random.default_rng(seed).integers(0, 256, (*size, 3), dtype=np.uint8)


def tile_image():
    """an 8 x 8 random tile repeated over 640 x 480: a periodic stream"""
    t = np.random.default_rng(1).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    return np.tile(t, (60, 80, 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 / 2: the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def test_corpus_covers_the_stated_cases():
    cases = R.corpus_cases()
    assert len(cases) == 200 and len({n for n, _, _ in cases}) == 200
    for sampling in R.SAMPLINGS:
        mine = [kw for _, kw, _ in cases if kw["sampling"] == sampling]
        assert len(mine) == 50
        assert {kw["quality"] for kw in mine} == set(R.QUALITIES) and {kw["optimize"] for kw in mine} == {False, True}
        assert {kw["restart"] for kw in mine} == set(R.RESTARTS)
    assert {s for _, _, s in cases} == set(R.SIZES) and (48, 64) in R.SIZES and len(R.SIZES) == 50


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_reference_is_bit_equal_to_pillow(sampling):
    n = 0
    for (name, kw, (w, h)), (_, data) in zip(R.corpus_cases(), R.corpus()):
        if kw["sampling"] != sampling:
            continue
        want = R.pillow_rgb(data)
        got = R.decode(data)
        assert want.shape == (h, w, 3) and got.shape == want.shape and np.array_equal(got, want), name
        n += 1
    assert n == 50


@pytest.mark.parametrize("defect", ["idct_truncate", "nearest_chroma", "color_round"])
def test_planted_defect_breaks_the_equality(defect):
    broken = total = 0
    for (name, kw, _), (_, data) in zip(R.corpus_cases(), R.corpus()):
        if defect == "nearest_chroma" and kw["sampling"] in ("grey", "444"):   # no chroma to interpolate
            continue
        if defect == "color_round" and kw["sampling"] == "grey":
            continue
        total += 1
        broken += not np.array_equal(R.decode(data, defect), R.pillow_rgb(data))
    print(f"{defect}: {broken} of {total} files differ from Pillow")
    assert total >= 100 and broken > total // 2, (defect, broken, total)


def test_reference_on_a_large_noise_image():
    for sampling in ("420", "444"):
        data = R.encode(_noise(size=(64, 96)), sampling=sampling, quality=95)
        assert np.array_equal(R.decode(data), R.pillow_rgb(data)), sampling


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: the parser
# ---------------------------------------------------------------------------------------------------------------------------------
def test_parser_agrees_with_pillow():
    import PIL.Image
    for (name, kw, (w, h)), (_, data) in zip(R.corpus_cases(), R.corpus()):
        im = PIL.Image.open(io.BytesIO(data))
        info = jpeg.probe(data)
        assert info is not None, (name, jpeg.refusal(data))
        assert (info["width"], info["height"]) == im.size == (w, h) and info["mode"] == im.mode, name
        assert info["components"] == im.layers == len(im.layer), name
        hs, vs = (im.layer[0][1], im.layer[0][2]) if im.layers == 3 else (1, 1)
        assert info["sampling"] == (hs, vs) == {"444": (1, 1), "422": (2, 1), "420": (2, 2), "grey": (1, 1)}[kw["sampling"]], name
        if kw["restart"] is None:
            assert info["restart_interval"] == 0 and info["n_segments"] == 1, name
        else:
            mcus = info["n_blocks"] // (1 if im.layers == 1 else hs * vs + 2)
            assert info["restart_interval"] > 0 and info["n_segments"] == -(-mcus // info["restart_interval"]), name
            assert kw["restart"] != "blocks" or info["n_segments"] == mcus, name
        assert jpeg.refusal(data) is None


def _markers(data):
    """offsets of the marker segments in front of the scan, and the scan's first byte"""
    pos, out = 2, []
    while True:
        assert data[pos] == 0xFF
        m, L = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        out.append((pos, m, L))
        pos += 2 + L
        if m == 0xDA:
            return out, pos


def _refused(data, *words):
    assert jpeg.probe(data) is None
    reason = jpeg.refusal(data)
    assert isinstance(reason, str) and reason, "a refusal without a reason"
    assert not words or any(w in reason for w in words), reason
    return reason


def test_parser_refusals():
    import PIL.Image
    img = R.synthetic(48, 64, 7)
    good = R.encode(img, sampling="422", quality=85)
    assert jpeg.probe(good)["sampling"] == (2, 1)
    _refused(R.encode(img, progressive=True), "progressive")
    buf = io.BytesIO()
    PIL.Image.fromarray(img).convert("CMYK").save(buf, "JPEG")
    _refused(buf.getvalue(), "4 components")
    # a 1x2-sampled file: the frame header of the 2x1 file with luma's factors swapped (the parser refuses on the header alone)
    segs, scan = _markers(good)
    sof = next(p for p, m, _ in segs if m == 0xC0)
    assert good[sof + 11] == 0x21
    _refused(good[:sof + 11] + b"\x12" + good[sof + 12:], "sampling")
    # cut at every marker boundary, in mid-scan, in front of EOI
    for p, _, _ in segs:
        _refused(good[:p])
        _refused(good[:p + 2])
        _refused(good[:p + 3])
    _refused(good[:scan], "EOI")
    _refused(good[:(scan + len(good)) // 2], "EOI")
    assert good[-2:] == b"\xff\xd9"
    _refused(good[:-2], "EOI")
    _refused(good[:-1], "EOI")
    # a length field pointing past the end, in every segment
    for p, m, L in segs:
        _refused(good[:p + 2] + b"\xff\xf0" + good[p + 4:], "past the end")
    # not a JPEG at all
    png = io.BytesIO()
    PIL.Image.fromarray(img).save(png, "PNG")
    _refused(png.getvalue(), "SOI")
    _refused(b"", "SOI")
    _refused(b"\xff\xd8", "SOI")
    _refused(b"\xff\xd8\xff", )
    # a restart marker the header does not announce; a scan too short for its MCUs
    _refused(good[:scan + 40] + b"\xff\xd0" + good[scan + 40:], "restart")
    _refused(good[:scan + 30] + b"\xff\xd9", "shorter")
    # the second component's Huffman table selector pointing at a table the file does not have
    sos = next(p for p, m, _ in segs if m == 0xDA)
    _refused(good[:sos + 8] + b"\x33" + good[sos + 9:], "Huffman")


def test_parser_handles_arbitrary_bytes_without_exceptions():
    rng = np.random.default_rng(3)
    good = R.encode(R.synthetic(33, 17, 2), sampling="420", quality=75, restart="blocks")
    for k in range(300):
        b = bytearray(good)
        for _ in range(1 + k % 5):
            b[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        info = jpeg.probe(bytes(b))
        assert info is not None or jpeg.refusal(bytes(b))


def test_load_images_decode_argument_is_checked_before_the_device():
    from must3r_amd import image
    import inspect
    assert inspect.signature(image.load_images).parameters["decode"].default == "pil"
    with pytest.raises(ValueError):
        image.load_images([], 512, decode="cpu")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: the stand-alone program under the host sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpeg_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("jpeg_check") / "jpeg_check"
    # the sanitizer runtimes linked into the program itself (clang's default; gcc needs the flags): it runs as it is, with nothing to preload
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    os.path.join(ROOT, "tests", "c", "jpeg_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_ctypes_layout_is_the_headers(jpeg_check):
    out = _run(jpeg_check, ["--sizes"])
    want = f"sizes: huff {C.sizeof(_lib.JpegHuff)} info {C.sizeof(_lib.JpegInfo)} image {C.sizeof(_lib.JpegImage)} batch {C.sizeof(_lib.JpegBatch)}"
    assert want in out, (want, out)


def test_sanitized_program_over_the_corpus(jpeg_check, tmp_path):
    paths = []
    for name, data in R.corpus():
        paths.append(str(tmp_path / f"{name}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    extra = {"noise_420": R.encode(_noise(), sampling="420", quality=95), "noise_444_rows": R.encode(_noise(), sampling="444", quality=95, restart="rows"),
             "grey128": R.encode(np.full((480, 640, 3), 128, np.uint8)), "black": R.encode(np.zeros((64, 64, 3), np.uint8)),
             "tile_420": R.encode(tile_image(), sampling="420", quality=90), "wide": R.encode(R.synthetic(4000, 3, 9))}
    for name, data in extra.items():
        paths.append(str(tmp_path / f"{name}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    dump = tmp_path / "coef"
    dump.mkdir()
    out = _run(jpeg_check, ["--dump", str(dump), *paths])
    last = out.strip().splitlines()[-1]
    print(last)
    assert last.startswith(f"jpeg_check: OK {len(paths)} files (0 refused), {6 * len(paths)} damaged variants"), last
    assert "tile_420.jpg: 640 x 480, 7200 blocks, 1 segments, sequential" in out      # a periodic stream defeats the synchronisation: the exact path
    assert "noise_420.jpg: 640 x 480, 7200 blocks, 1 segments, fast" in out
    # the coefficients the routine wrote are the reference's
    for name, data in list(R.corpus())[::7] + [("black", extra["black"])]:
        got = np.fromfile(dump / f"{name}.jpg.coef", dtype=np.int16).reshape(-1, 64)
        want = R.entropy(data)[1]
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_gpu_decode_switch_reaches_load_images(monkeypatch):
    """get_reconstruction.py --gpu_decode (its own switch: get_args_parser() stays the reference's) and get_reconstructed_scene(gpu_decode=True) pass
    decode="gpu" on to load_images; without them it is "pil" """
    from must3r_amd import demo, get_reconstruction as G
    assert G.get_cli_parser().parse_args(["--image_dir", "a", "--output", "b"]).gpu_decode is False
    assert G.get_cli_parser().parse_args(["--image_dir", "a", "--output", "b", "--gpu_decode"]).gpu_decode is True
    assert not any("--gpu_decode" in a.option_strings for a in G.get_args_parser()._actions)
    seen = []

    class Stop(Exception):
        pass

    def load_images(filelist, size, **kw):
        seen.append(kw.get("decode"))
        raise Stop

    monkeypatch.setattr(demo, "load_images", load_images)
    monkeypatch.setattr(demo, "get_pointmaps_activation", lambda *a, **k: None)

    class Model:
        def __iter__(self):
            enc = type("E", (), {"patch_size": 16})()
            return iter((enc, object()))

    for flag in (False, True):
        for fn, kw in ((demo.must3r_inference, dict(retrieval=None, num_mem_images=2, render_once=False, is_sequence=True)), (demo.must3r_inference_video, {})):
            with pytest.raises(Stop):
                fn(model=Model(), device="cuda", image_size=512, amp=False, filelist=["x.jpg"], max_bs=1, init_num_images=2, batch_num_views=1, verbose=False,
                   gpu_decode=flag, **kw)
    assert seen == ["pil", "pil", "gpu", "gpu"]
    # get_reconstructed_scene: the switch travels only when it is set (the default call hands the drivers the reference's arguments alone)
    got = []
    monkeypatch.setattr(demo, "must3r_inference", lambda *a, **k: got.append(k.get("gpu_decode", "absent")) or "scene")
    args = dict(outdir="o", viser_server=None, should_save_glb=False, model=("e", "d"), retrieval=None, device="cuda", verbose=False, image_size=512, amp=False,
                filelist=["a.jpg", "b.jpg"], max_bs=1, num_refinements_iterations=0, execution_mode="linseq", num_mem_images=2, render_once=False,
                vidseq_local_context_size=0, keyframe_interval=3, slam_local_context_size=0, subsample=2, min_conf_keyframe=1.5, keyframe_overlap_thr=0.05,
                overlap_percentile=85, min_conf_thr=3.0, as_pointcloud=True, transparent_cams=False, local_pointmaps=False, cam_size=0.05)
    demo.get_reconstructed_scene(**args)
    demo.get_reconstructed_scene(**args, gpu_decode=True)
    assert got == ["absent", True]
