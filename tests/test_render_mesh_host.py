"""Host side of the mesh rasteriser (must3r_amd.render with ``mesh=True``, csrc/render_mesh.hip's descriptor checks, csrc/render_tri.hpp, the numpy
restatement tests/render_mesh_ref.py), no GPU needed:

1. the cases of tests/render_mesh_cases.py are not vacuous, and each planted defect of the restatement is told from the true rule by one of them;
2. tests/c/render_tri_check.cpp -- render_tri.hpp on the host, built with the host sanitizers and -ffp-contract=off, run as a child process with nothing
   preloaded -- gives the restatement's candidate boxes, covered samples, Zp bits and t bits on every case;
3. the ABI surface: header text, ctypes layouts against the header and against sizeof, the scratch arithmetic and every refusal (the plan makes no HIP
   call: the pointers are host addresses);
4. the keyword and command-line switches with their errors.
"""
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import render_mesh_cases as K
import render_mesh_ref as MR
import render_ref as RR
from conftest import ROOT
from must3r_amd import _lib, render as Rn
from test_render_host import _header, _struct_layout

EMPTY = 0xFFFFFFFF
CASES = [("main", K.main_case), ("lattice", K.lattice_case), ("plane", K.plane_case), ("sizes", lambda: K.sizes_case(_lib.RENDER_MESH_WAVE_AREA)),
         ("degenerate", K.degenerate_case), ("twin", K.twin_case)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the cases and the planted defects
# ---------------------------------------------------------------------------------------------------------------------------------
def test_main_case_is_not_vacuous():
    views, M, cams, thr = K.case("main", K.main_case)
    assert [v[0].shape for v in views] == [(9, 13), (16, 16), (2, 2), (1, 7)] and not any(np.array_equal(m, np.eye(4)[:3]) for m in M[:3])
    total = dict.fromkeys(MR.DROPS + ("clipped",), 0)
    for ci, cam in enumerate(cams):
        _, _, index, c = K.want("main", K.main_case, ci)
        cnt = np.bincount(c["pix"], minlength=cam.W * cam.H)
        print(f"camera {ci}: covered {(cnt > 0).mean():.3f}, two or more contenders {(cnt >= 2).mean():.3f}, {c['stats']}")
        assert (cnt > 0).mean() >= 1 / 3 and (cnt >= 2).sum() >= 1 and np.array_equal(cnt > 0, index.reshape(-1) != EMPTY)
        assert c["stats"]["triangles"] == 2 * (8 * 12 + 15 * 15 + 1)          # the 1 x 7 view has none
        for k in total:
            total[k] += c["stats"][k]
    # every drop reason removes a triangle, some triangles are cut by the border, some lie off the image
    assert all(total[k] >= 1 for k in ("conf", "nonfinite", "near", "far", "off_image", "clipped")), total


def test_each_planted_defect_is_told_from_the_rule():
    # exclusive edges: the lattice case puts pixel centres on vertices, outline edges and diagonals
    true, excl = K.want("lattice", K.lattice_case, 0), K.want("lattice", K.lattice_case, 0, exclusive=True)
    assert (true[2] != EMPTY).sum() == 49 and (excl[2] != EMPTY).sum() < 49
    # affine weights: depth and colour of the main case change
    for ci in range(3):
        true, aff = K.want("main", K.main_case, ci), K.want("main", K.main_case, ci, affine=True)
        assert (_bits(true[1]) != _bits(aff[1])).sum() > 100 and (true[0] != aff[0]).sum() > 10
    # E_20 from corner 2: the same real number as -E_02, other bits -- in the weights t that the host program and the resolve reproduce bit for bit
    true, e20 = K.want("main", K.main_case, 0)[3], K.want("main", K.main_case, 0, e20=True)[3]
    assert np.array_equal(true["pix"], e20["pix"]) and (_bits(true["t"]) != _bits(e20["t"])).any(axis=1).sum() > 100
    assert np.allclose(true["t"], e20["t"], rtol=1e-9, atol=1e-12)


def test_lattice_plane_sizes_degenerate_and_twin_cases():
    # lattice: every pixel whose centre lies in or on the outline is covered
    index = K.want("lattice", K.lattice_case, 0)[2]
    want = np.zeros((8, 8), dtype=bool)
    want[:7, :7] = True
    assert np.array_equal(index != EMPTY, want)
    # plane: watertight inside the outline (a margin of one pixel), where points leave holes
    views, M, cams, thr = K.case("plane", K.plane_case)
    index, c = K.want("plane", K.plane_case, 0)[2:]
    inside = K.inside_outline(K.plane_outline(views, M, cams[0]), 64, 48, 1.0)
    points = RR.render(views, M, cams[0], thr, 1)[2]
    assert inside.sum() > 1000 and (index != EMPTY)[inside].all() and ((points != EMPTY) & inside).sum() < inside.sum() // 4
    assert max((b[1] - b[0] + 1) * (b[3] - b[2] + 1) for b in c["boxes"].values()) > _lib.RENDER_MESH_WAVE_AREA
    # sizes: the boxes straddle the split between the lane path and the wave path; the last camera's triangle 0 covers the whole target
    wa = _lib.RENDER_MESH_WAVE_AREA
    areas = []
    for ci in range(4):
        index, c = K.want("sizes", CASES[3][1], ci)[2:]
        areas.append([(b[1] - b[0] + 1) * (b[3] - b[2] + 1) for b in (c["boxes"][0], c["boxes"][1])])
        assert (index != EMPTY).sum() == areas[-1][0]
    assert areas == [[wa - 1] * 2, [wa] * 2, [wa + 1] * 2, [256] * 2] and (K.want("sizes", CASES[3][1], 3)[2] == 0).all()
    # degenerate: candidates, and nothing drawn
    rgb, depth, index, c = K.want("degenerate", K.degenerate_case, 0)
    assert c["stats"]["drawn"] >= 3 and len(c["pix"]) == 0 and (index == EMPTY).all() and np.isposinf(depth).all() and (rgb == 255).all()
    # twin: the lower id wins every pixel
    index = K.want("twin", K.twin_case, 0)[2]
    assert (index != EMPTY).mean() > 0.1 and index[index != EMPTY].max() < 2 * 6 * 7


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: render_tri.hpp on the host
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tri_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("render_tri_check") / "render_tri_check"
    # the sanitizer runtimes linked into the program itself (clang's default; gcc needs the flags): it runs as it is, with nothing to preload
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    os.path.join(ROOT, "tests", "c", "render_tri_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_ctypes_layout_is_the_headers(tri_check):
    out = _run(tri_check, ["--sizes"])
    want = (f"sizes: mesh_desc {C.sizeof(_lib.RenderMeshDesc)} camera {C.sizeof(_lib.RenderCamera)} view {C.sizeof(_lib.ExportView)} "
            f"wave_area {_lib.RENDER_MESH_WAVE_AREA} scratch_offset {_lib.RenderMeshDesc.scratch.offset}")
    assert want in out, (want, out)


def _write_case(path, views, matrices, cam, thr):
    with open(path, "wb") as f:
        f.write(struct.pack("<3i6df", len(views), cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy, float(np.float32(cam.z_near)), float(np.float32(cam.z_far)),
                            thr))
        for (conf, pts, _), M in zip(views, matrices):
            f.write(struct.pack("<2i", *conf.shape))
            f.write(RR.compose(cam.w2c, M).astype("<f8").tobytes())
            f.write(np.ascontiguousarray(conf, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(pts, dtype="<f4").tobytes())


@pytest.mark.parametrize("name,builder", CASES, ids=[c[0] for c in CASES])
def test_header_text_on_the_host_equals_the_restatement(tri_check, tmp_path, name, builder):
    views, matrices, cams, thr = K.case(name, builder)
    samples = 0
    for ci, cam in enumerate(cams):
        c = K.want(name, builder, ci)[3]
        path = str(tmp_path / f"{name}{ci}.bin")
        _write_case(path, views, matrices, cam, thr)
        lines = _run(tri_check, [path]).strip().splitlines()
        boxes = {int(t[1]): tuple(int(x) for x in t[2:]) for t in (ln.split() for ln in lines if ln.startswith("box "))}
        hits = [ln.split()[1:] for ln in lines if ln.startswith("hit ")]
        assert boxes == c["boxes"], (name, ci)
        assert lines[-1] == f"render_tri_check: OK {len(boxes)} triangles, {len(hits)} samples"
        # the same covered set in the same order (triangles ascending, a box row-major), the same Zp bits and t bits
        ids = (c["key"] & np.uint64(EMPTY)).astype(np.int64)
        assert len(hits) == len(ids) and [int(h[0]) for h in hits] == ids.tolist() and [int(h[1]) for h in hits] == c["pix"].tolist()
        got = np.array([[int(x, 16) for x in h[2:]] for h in hits], dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(got[:, 0], _bits(c["Zp"])) and np.array_equal(got[:, 1:], _bits(c["t"]))
        samples += len(hits)
    assert samples > 0 or name == "degenerate"


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: ABI surface, layout, scratch and refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _align(x):
    return (x + 255) // 256 * 256


def _scratch(nv, nc, W, H):
    return _align(40 * nv) + _align(40 * nc) + _align(96 * nc * nv) + _align(8 * nc * W * H)


def _desc(n_views=2, n_cams=2, W=64, H=48, vh=12, vw=16):
    """a valid descriptor over host addresses that are never read; returns it with the objects it points to"""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    views = (_lib.ExportView * max(n_views, 1))()
    for e in views:
        e.conf = e.pts = e.rgb = p
        e.H, e.W = vh, vw
    cams = (_lib.RenderCamera * max(n_cams, 1))()
    for e in cams:
        e.fx = e.fy = 10.0
        e.z_near, e.z_far, e.W, e.H = 0.01, 100.0, W, H
    d = _lib.RenderMeshDesc()
    d.views, d.cams, d.n_views, d.n_cams, d.thr = views, cams, n_views, n_cams, 1.5
    d.scratch, d.scratch_bytes = p // 256 * 256 + 256, 1 << 40
    d.rgb = d.depth = d.index = p
    return d, (buf, views, cams)


def test_abi_surface_layout_and_scratch_bytes():
    h = _header()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.must3r_hip_abi_version() == 21 and "ABI 21, additive: scene rendering, triangles" in h
    for name, proto in (("must3r_hip_render_mesh_scratch_bytes", (C.c_size_t, [C.POINTER(_lib.RenderMeshDesc)])),
                        ("must3r_hip_render_mesh", (C.c_int, [C.POINTER(_lib.RenderMeshDesc)]))):
        assert name in _lib.EXPORTS and _lib.PROTOTYPES[name] == proto and hasattr(lib, name)
    assert re.search(r"\bsize_t\s+must3r_hip_render_mesh_scratch_bytes\s*\(\s*const\s+must3r_hip_render_mesh_desc\s*\*\s*d\s*\)\s*;", h)
    assert re.search(r"\bint\s+must3r_hip_render_mesh\s*\(\s*const\s+must3r_hip_render_mesh_desc\s*\*\s*d\s*\)\s*;", h)
    assert int(re.search(r"#define\s+MUST3R_RENDER_MESH_WAVE_AREA\s+(\d+)", h).group(1)) == _lib.RENDER_MESH_WAVE_AREA
    # the descriptor repeats the point path's fields without point_size; the point path's descriptor keeps its layout
    layout, size = _struct_layout("must3r_hip_render_mesh_desc")
    assert [(n, getattr(_lib.RenderMeshDesc, n).offset) for n, _ in _lib.RenderMeshDesc._fields_] == layout and C.sizeof(_lib.RenderMeshDesc) == size
    assert [n for n, _ in _lib.RenderMeshDesc._fields_ if n != "reserved"] == [n for n, _ in _lib.RenderDesc._fields_ if n not in ("point_size", "reserved")]
    assert C.sizeof(_lib.RenderDesc) == 88 and _lib.RenderDesc.scratch.offset == 40
    with open(os.path.join(ROOT, "must3r_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRCS\s*=.*\brender_mesh\.hip\b", mk, flags=re.M) and re.search(r"^build/render_mesh\.o: FLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    # the same four sections as the point path
    for nv, nc, W, H, vh, vw in ((5, 2, 64, 48, 12, 16), (200, 120, 512, 384, 384, 512)):
        d, keep = _desc(nv, nc, W, H, vh, vw)
        assert lib.must3r_hip_render_mesh_scratch_bytes(C.byref(d)) == _scratch(nv, nc, W, H)
    assert lib.must3r_hip_render_mesh_scratch_bytes(None) == 0 and "null" in lib.must3r_hip_last_error().decode()


def _refused(d, word):
    lib = _lib.load()
    assert lib.must3r_hip_render_mesh(C.byref(d)) != 0
    msg = lib.must3r_hip_last_error().decode()
    assert word in msg and msg.startswith("render_mesh:"), (word, msg)


def test_refusals_before_any_launch():
    """every refusal the header lists; the pointers are host addresses, so a call that got as far as an upload or a launch would not return cleanly"""
    lib = _lib.load()
    assert lib.must3r_hip_render_mesh(None) != 0 and "null descriptor" in lib.must3r_hip_last_error().decode()
    for field in ("W", "H"):
        d, keep = _desc()
        for e in keep[2]:
            setattr(e, field, 0)
        _refused(d, "non-positive image size")
        assert lib.must3r_hip_render_mesh_scratch_bytes(C.byref(d)) == 0
    d, keep = _desc(); d.n_cams = 0; _refused(d, "camera table is empty")
    d, keep = _desc(); d.n_views = 0; _refused(d, "view table is empty")
    d, keep = _desc(); keep[2][1].W = 65; _refused(d, "share one image size")
    d, keep = _desc(); keep[2][1].H = 47; _refused(d, "share one image size")
    d, keep = _desc(); d.views = None; _refused(d, "null view table")
    d, keep = _desc(); d.cams = None; _refused(d, "null camera table")
    d, keep = _desc(); keep[1][1].H = 0; _refused(d, "a view has a non-positive size")
    for zn, zf in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.1, float("inf")), (0.1, float("nan"))):
        d, keep = _desc()
        keep[2][0].z_near, keep[2][0].z_far = zn, zf
        _refused(d, "z_near")
    # 2^31 source pixels in the scene (the point path takes up to 2^32), 2^31 in one view, 2^31 target pixels: arithmetic on the sizes alone
    d, keep = _desc(n_views=2, vh=32768, vw=32768)
    assert 2 * 32768 * 32768 == 2 ** 31
    _refused(d, "the scene has 2^31")
    d.n_views = 1
    assert lib.must3r_hip_render_mesh_scratch_bytes(C.byref(d)) > 0
    d, keep = _desc(n_views=1, vh=65536, vw=32768); _refused(d, "a view has 2^31")
    d, keep = _desc(n_cams=2, W=32768, H=32768); _refused(d, "target pixels")
    # views without a triangle are no error
    for vh, vw in ((1, 7), (7, 1), (1, 1)):
        d, keep = _desc(vh=vh, vw=vw)
        assert lib.must3r_hip_render_mesh_scratch_bytes(C.byref(d)) == _scratch(2, 2, 64, 48)
    # the scratch
    d, keep = _desc(); d.scratch = None; _refused(d, "null scratch")
    d, keep = _desc(); d.scratch_bytes = _scratch(2, 2, 64, 48) - 1; _refused(d, "scratch too small")
    d, keep = _desc(); d.scratch += 8; _refused(d, "aligned")
    for plane in ("conf", "pts", "rgb"):
        d, keep = _desc()
        setattr(keep[1][1], plane, None)
        _refused(d, "null plane")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: switches
# ---------------------------------------------------------------------------------------------------------------------------------
def test_keyword_and_command_line_switches():
    from must3r_amd import demo, get_reconstruction as G, slam
    for fn in (Rn.SceneRenderer.render, Rn.render_views, Rn.render_scene, demo.render_previews):
        assert inspect.signature(fn).parameters["mesh"].default is False, fn
    assert inspect.signature(demo.get_reconstructed_scene).parameters["render_mesh"].default is False
    renderer = Rn.SceneRenderer([], device="cuda:0")          # no view, no device call: the arguments are checked first
    for ps in (2, 0, 8):
        with pytest.raises(ValueError, match="mesh=True"):
            renderer.render([], 1.5, point_size=ps, mesh=True)
    with pytest.raises(ValueError, match="want"):
        renderer.render([], 1.5, mesh=True, want=("normals",))
    a = G.get_cli_parser().parse_args(["--image_dir", "i", "--output", "o"])
    assert a.render_mesh is False
    a = G.get_cli_parser().parse_args(["--image_dir", "i", "--output", "o", "--render_dir", "r", "--render_mesh"])
    assert a.render_mesh is True and a.render_dir == "r"
    with pytest.raises(SystemExit, match="--render_mesh needs --render_dir"):
        G.main(["--image_dir", "i", "--output", "o", "--weights", "w", "--render_mesh"])
    # the SLAM fly-through stays on points: its map is a compacted point list
    assert not any("mesh" in s for a in slam.get_parser()._actions for s in a.option_strings)
