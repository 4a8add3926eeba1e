"""No GPU: the rule that picks the GEMM kernel family of a launch (must3r_amd/csrc/gemm_route.hpp), evaluated by tests/c/gemm_route_check.cpp -- a stand-alone program
over that header alone, built with -fsanitize=address,undefined and run as a child process with nothing preloaded.

1. At the default options the program against the Python restatements of the rule, point for point: gemm_forms.dispatch over the grid below (M: the tile boundaries, each
   with its neighbours; N: every multiple of 64 up to 4608; the six epilogues, EPI_HEAD where N % 112 == 0; plain, split and split-with-sparse-copy weights; rope_tab
   exactly with the RoPE epilogue), and lnfold_forms.consumer_kernel / producer_kernel over their own domain.
2. Properties of the rule over the full product of the allowed values of its eight options (ranges: misc.hip kOpts), on the same grid thinned in N."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_forms as G
import lnfold_forms as L
from conftest import ROOT

MS = (1, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 196, 255, 256, 257, 700, 767, 768, 769, 1024, 1536, 3072, 3840, 12288, 15360, 15361, 43008)
NS = tuple(range(64, 4608 + 1, 64))
KS = (64, 128, 192, 256, 768, 1024, 3072)
BS = (1, 2, 12, 84)
NS_THIN = (768, 1024)          # section 2: 48-, 96-, 128-, 192- and 256-column tiles / 128 and 256 but none of the others
OPT_NAMES = ("GEMM256", "G256K", "G256P", "G256P_SPLIT", "SPARSE_256", "SPARSE_LO", "BK128", "PERSIST")
OPT_RANGE = dict(GEMM256=(0, 1, 2), G256K=(0, 1, 2), G256P=(0, 1), G256P_SPLIT=(0, 1, 2), SPARSE_256=(0, 1), SPARSE_LO=(0, 1), BK128=(0, 1), PERSIST=(0, 1))
OPT_DEFAULT = dict(GEMM256=1, G256K=1, G256P=1, G256P_SPLIT=1, SPARSE_256=1, SPARSE_LO=1, BK128=1, PERSIST=0)
CUS = 256
FAMILIES = ("", "g64", "g64p", "g128", "g48", "g48k128", "g96", "g256", "g256o2", "g256k", "g256p", "g256ps", "g256s", "g256pf", "g256sf")   # enum GemmFamily
FAM = {n: i for i, n in enumerate(FAMILIES)}
ROWS256_NAMES = ("g256", "g256o2", "g256k", "g256p", "g256ps", "g256s", "g256pf", "g256sf")
SPLIT_REFUSAL = "gemm: split weights are only built for fp16"


@pytest.fixture(scope="module")
def route_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("gemm_route_check") / "gemm_route_check"
    # the sanitizer runtimes linked into the program itself (clang's default; gcc needs the flags): it runs as it is, with nothing to preload
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    os.path.join(ROOT, "tests", "c", "gemm_route_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, args, text):
    r = subprocess.run([exe, *args], input=text.encode(), capture_output=True, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-4000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
    return r.stdout


def ask(exe, lines):
    """the program's answer lines to the input lines (the `o` lines have none)"""
    return _run(exe, [], "\n".join(lines) + "\n").decode().splitlines()


def shape_line(epi, M, N, K, wsplit, batch=1, fp16=1, sparse=0, ln_consumer=0, ln_producer=0, fold256=0):
    return f"s {fp16} {epi} {M} {N} {K} {wsplit} {batch} {int(epi == G.EPI_QKV_ROPE)} {sparse} {ln_consumer} {ln_producer} {fold256}"


def opt_line(**kw):
    v = dict(OPT_DEFAULT, **kw)
    return "o " + " ".join(str(v[n]) for n in OPT_NAMES) + f" {CUS}"


def grid(exe, opts, D=(1,), P=(0,), ms=MS, ns=NS, ks=KS, bs=BS):
    """records [options..., D, P, M, N, K, B, epilogue, weights, 4] = (family, ws, bn / 16, flags) of the product; opts: name -> values"""
    axes = [tuple(opts[n]) for n in OPT_NAMES] + [(CUS,), D, P, ms, ns, ks, bs]
    text = "".join(f"{n} {' '.join(map(str, v))}\n" for n, v in zip(OPT_NAMES + ("CUS", "D", "P", "M", "N", "K", "B"), axes))
    rec = np.frombuffer(_run(exe, ["--grid"], text), dtype=np.uint8)
    shape = [len(a) for a in axes] + [6, 3, 4]
    assert rec.size == int(np.prod(shape)), (rec.size, shape)
    return rec.reshape(shape)


def record(name):
    fam, _, ws, bn = name.split("/")
    return FAM[fam], int(ws[1:]), int(bn[1:]) // 16


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the default options against the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
def test_default_route_is_gemm_forms_dispatch(route_check):
    rec = grid(route_check, {n: (OPT_DEFAULT[n],) for n in OPT_NAMES})
    rec = rec.reshape(len(MS), len(NS), len(KS), len(BS), 6, 3, 4)
    assert not (rec[..., 3] & 0x0F).any(), "persistent, fold or refused at the default options"
    want = np.zeros(rec.shape[:-1] + (3,), dtype=np.uint8)
    cache = {}
    for (i, M), (j, N), (k, K), (b, B) in itertools.product(enumerate(MS), enumerate(NS), enumerate(KS), enumerate(BS)):
        for epi in range(6):
            for w in range(3):
                name = G.dispatch(epi, M, N, K, 2 if w else 0, B, w == 2)
                if name not in cache:
                    cache[name] = record(name)
                want[i, j, k, b, epi, w] = cache[name]
    head_ok = np.array([N % 112 == 0 for N in NS])
    same = (rec[..., :3] == want).all(-1)
    same[:, ~head_ok, :, :, G.EPI_HEAD] = True      # launch_gemm refuses EPI_HEAD at another N before any route is asked
    bad = np.argwhere(~same)
    assert bad.size == 0, [(MS[i], NS[j], KS[k], BS[b], epi, w, rec[i, j, k, b, epi, w, :3].tolist(), want[i, j, k, b, epi, w].tolist()) for i, j, k, b, epi, w in bad[:10]]
    assert head_ok.sum() >= 5 and {c[0] for c in cache.values()} >= {FAM[n] for n in ("g64", "g64p", "g128", "g48", "g48k128", "g96", "g256", "g256o2", "g256k", "g256p",
                                                                                         "g256ps", "g256s")}
    print(f"{same.size} points, {len(cache)} distinct kernels")


def test_default_route_of_the_lnfold_launches(route_check):
    lines, want = [], []
    for bk128 in (0, 1):
        lines.append(opt_line(BK128=bk128))
        for M, K in itertools.product(L.MS, (768, 3072)):
            for epi, N in ((L.EPI_QKV_ROPE, 3 * L.D), (L.EPI_STORE16, L.D), (L.EPI_STORE16_GELU, 4 * L.D)):     # at the width of the form's call site, and at 768
                for weights, n in itertools.product(("split", "plain"), (N, L.D)):
                    lines.append(shape_line(epi, M, n, K, 2 if weights == "split" else 0, ln_consumer=1))
                    want.append(L.consumer_kernel(epi, weights, bk128))
    lines.append(opt_line())
    for M in L.MS:
        for K in (768, 3072):
            for epi in (L.EPI_RESID_F32, L.EPI_F32):
                for weights in ("split", "plain"):
                    for fold_outputs in (True, False):
                        lines.append(shape_line(epi, M, L.D, K, 2 if weights == "split" else 0, ln_producer=int(fold_outputs)))
                        want.append(L.producer_kernel(epi, M, K, weights, fold_outputs))
    got = ask(route_check, lines)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:10]
    assert len(got) == 2 * len(L.MS) * 2 * 12 + len(L.MS) * 16


def test_refusals_and_the_names_they_leave(route_check):
    got = ask(route_check, [
        shape_line(G.EPI_STORE16, 768, 768, 768, 2, fp16=0),                       # split bf16
        shape_line(G.EPI_STORE16, 768, 768, 768, 2, fp16=0, fold256=1),            # fold256 bf16: the fold's own text
        shape_line(G.EPI_STORE16_GELU, 1024, 1024, 768, 2, sparse=1, fold256=1),   # fold256, split: not built for the GELU epilogue
        shape_line(G.EPI_STORE16, 1024, 1024, 768, 0, fold256=1),                  # fold256, plain: not built for STORE16
        shape_line(G.EPI_STORE16_GELU, 768, 64, 768, 2, ln_consumer=1),            # consumer on 96-column tiles, N % 96 != 0
        shape_line(G.EPI_STORE16, 768, 64, 768, 2, ln_consumer=1),                 # consumer on 48-column tiles, N % 48 != 0
        shape_line(G.EPI_RESID_F32, 768, 768, 768, 2, ln_consumer=1),              # consumers are built for the 16-bit-store epilogues
        shape_line(G.EPI_F32, 768, 768, 768, 0, ln_consumer=1),
        shape_line(G.EPI_RESID_F32, 15360, 1024, 768, 2, sparse=1, fold256=1),
        shape_line(G.EPI_STORE16_GELU, 15360, 3072, 768, 0, fold256=1),
    ])
    fold = "gemm: fold256 is built for fp16: split STORE16 / QKV_ROPE / RESID_F32 and plain STORE16_GELU / RESID_F32"
    failed = "gemm: kernel launch failed"
    assert got == [f"refused: {SPLIT_REFUSAL} | -", f"refused: {fold} | -", f"refused: {fold} | -", f"refused: {fold} | -", f"refused: {failed} | g96/e1/w2/n96",
                   f"refused: {failed} | g48k128/e0/w2/n48", f"refused: {failed} | -", f"refused: {failed} | -", "g256sf/e3/w3/n256", "g256pf/e1/w1/n256"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: properties over every option value.  Records [GEMM256, G256K, G256P, G256P_SPLIT, SPARSE_256, SPARSE_LO, BK128, PERSIST, M, N, K, B, epilogue, weights, 4]
# ---------------------------------------------------------------------------------------------------------------------------------
def _product(exe, ns, fp16=1, producer=0):
    rec = grid(exe, OPT_RANGE, D=(fp16,), P=(producer,), ns=ns)
    return rec.reshape([len(OPT_RANGE[n]) for n in OPT_NAMES] + [len(MS), len(ns), len(KS), len(BS), 6, 3, 4])


class _Records:
    """holds the array, so that the report of a failing test does not print it"""
    def __init__(self, rec):
        self.rec = rec


@pytest.fixture(scope="module")
def product(route_check):
    """fp16 launches without fold outputs"""
    return _Records(_product(route_check, NS_THIN))


def _fam(rec, *names):
    lut = np.zeros(256, dtype=bool)
    lut[[FAM[n] for n in names]] = True
    return lut[rec[..., 0]]


def _refusal(rec):
    return rec[..., 3] >> 2 & 3


def test_gemm256_0_never_yields_a_256_row_family(product):
    """This includes the two sparse kernels (g256ps, g256s), which the rule this one was taken from still picked with GEMM256 = 0 whenever the caller had the packed
    low part: at 693504 of the 8418816 points of this grid.  With the switch at 0 the sparse copy now changes nothing: the launch goes where the dense split one goes."""
    off = product.rec[0]
    n = int(_fam(off, *ROWS256_NAMES).sum())
    print(f"GEMM256 = 0: {n} of {off[..., 0].size} points on a 256-row family")
    assert n == 0
    assert np.array_equal(off[..., 2, :], off[..., 1, :]), "GEMM256 = 0: the packed sparse low part moves a launch"
    on = product.rec[1]
    assert _fam(on, *ROWS256_NAMES).any() and _fam(on[..., 2, :], "g256ps", "g256s").any()


def test_switches_turn_their_families_off(product, route_check):
    r = product.rec
    off = r[:, :, :, 0]
    assert not _fam(off, "g256ps", "g256s").any() and not (_fam(off, "g256p") & (off[..., 1] == 2)).any(), "G256P_SPLIT = 0 and g256ps, g256s or split g256p"
    assert not _fam(r[:, :, :, :, 0], "g256s").any(), "SPARSE_256 = 0 and g256s"
    assert not _fam(r[:, :, :, :, :, :, 0], "g48k128").any(), "BK128 = 0 and g48k128"
    assert (_refusal(r) == 0).all() and (r[..., 0] != 0).all(), "an fp16 launch of the grid refused"
    # and each of them is reached with the switch on, so the assertions above are not vacuous
    on = r[:, :, :, 1]
    assert _fam(on, "g256ps").any() and (_fam(on, "g256p") & (on[..., 1] == 2)).any() and _fam(r[:, :, :, :, 1], "g256s").any() and _fam(r[:, :, :, :, :, :, 1], "g48k128").any()
    prod = _product(route_check, (768,), producer=1)
    assert not _fam(prod, *ROWS256_NAMES, "g128").any() and not (prod[..., 1] == 3).any(), "an LN-fold producer on a 256-row, g128 or sparse family"
    assert _fam(prod, "g48", "g48k128").any() and _fam(prod, "g96").any() and _fam(prod, "g64").any() and _fam(prod, "g64p").any() and (_refusal(prod) == 0).all()


def test_split_weights_on_bf16_are_refused(route_check):
    bf16 = _product(route_check, (768,), fp16=0)
    split, plain = bf16[..., 1:, :], bf16[..., 0, :]
    assert (split[..., 0] == 0).all() and (_refusal(split) == 1).all(), "a bf16 launch with split weights that is not the split-weights refusal"
    assert (plain[..., 0] != 0).all() and (_refusal(plain) == 0).all() and (plain[..., 1] == 1).all()


def test_persist_moves_nothing_but_its_flag(product):
    p0, p1 = product.rec[:, :, :, :, :, :, :, 0], product.rec[:, :, :, :, :, :, :, 1]
    assert np.array_equal(p0[..., :3], p1[..., :3]) and np.array_equal(p0[..., 3] & 0xFE, p1[..., 3] & 0xFE)
    assert not (p0[..., 3] & 1).any(), "persistent with PERSIST = 0"
    # with PERSIST = 1: exactly the launches of g256p / g256ps / g256s with more work items than CUs (nothing in the grid folds)
    M = np.array(MS).reshape(-1, 1, 1, 1, 1, 1)
    N = np.array(NS_THIN).reshape(-1, 1, 1, 1, 1)
    B = np.array(BS).reshape(-1, 1, 1)
    nwork = (M + 255) // 256 * B * (N // np.maximum(p1[..., 2].astype(np.int64) * 16, 1))
    fams = _fam(p1, "g256p", "g256ps", "g256s")
    want = fams & (nwork > CUS)
    assert not (p1[..., 3] & 2).any() and np.array_equal((p1[..., 3] & 1) != 0, want) and want.any() and (fams & ~want).any()


def test_fold256_shape_ok_implies_the_fold_carrying_kernel(product):
    """wherever gemm_fold256_shape_ok says yes, the non-fold route of that shape with one problem is the 256 x 256 kernel that carries the fold"""
    r = product.rec[..., BS.index(1), :, :, :]      # one problem: [options..., M, N, K, epilogue, weights, 4]
    ok = (r[..., 3] & 16) != 0
    for weights, epis, kernel in ((2, (G.EPI_STORE16, G.EPI_QKV_ROPE, G.EPI_RESID_F32), (FAM["g256s"], 3, 16)),
                                  (0, (G.EPI_STORE16_GELU, G.EPI_RESID_F32), (FAM["g256p"], 1, 16))):
        for epi in epis:
            yes = ok[..., epi, weights]
            assert yes.any() and not yes.all() and (r[..., epi, weights, :3][yes] == kernel).all(), (weights, epi)
    # the predicate reads the shape and the weight form only: one answer for every epilogue, and for split weights with and without the sparse copy
    assert (ok == ok[..., :1, :]).all() and np.array_equal(ok[..., 1], ok[..., 2])
