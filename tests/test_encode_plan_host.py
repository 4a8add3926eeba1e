"""No GPU: the rule that cuts the encoder's views into chunks (must3r_amd/csrc/encode_plan.hpp), evaluated by tests/c/encode_plan_check.cpp -- a stand-alone program
over that header and gemm_route.hpp alone, built with -fsanitize=address,undefined and run as a child process with nothing preloaded.  The program asserts the
properties itself (sizes sum to the view count, no chunk over the cap, never dearer and never more chunks than the equal split, 560 views at 375.5 weighted rounds or
less against 392, 100 views filled to 90 % but for one remainder, 224 x 224 inputs, shapes off the 256-row kernels); this file builds it, runs it and reads a few
plans back."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("encode_plan_check") / "encode_plan_check"
    # the sanitizer runtimes linked into the program itself (clang's default; gcc needs the flags): it runs as it is, with nothing to preload
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    os.path.join(ROOT, "tests", "c", "encode_plan_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, timeout=600)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, (out[-4000:], err[-4000:])
    assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
    return out


def _plan(exe, n, tokens=768, C=1024, F=4096, cap=32768):
    """([chunk sizes], weighted rounds) of one call at the default options"""
    line = _run(exe, n, tokens, C, F, cap).strip()
    assert line.startswith("plan:"), line
    sizes, units = line[len("plan:"):].split("|")
    plan = []
    for run in sizes.split():
        count, size = run.split("x")
        plan += [int(size)] * int(count)
    return plan, float(units)


def test_the_program_own_checks_hold(plan_check):
    out = _run(plan_check)
    print(out)
    assert out.rstrip().endswith("OK") and "FAIL" not in out


def test_plans_of_the_benched_step_and_its_neighbours(plan_check):
    plan, units = _plan(plan_check, 560)
    # 13 chunks' worth of full rounds and a remainder's: every chunk on the rounds of a 42-view one or cheaper, 14 chunks as before
    assert sum(plan) == 560 and len(plan) == 14 and max(plan) == 42 and plan.count(42) >= 12 and units <= 375.5
    assert _plan(plan_check, 80) == ([40, 40], 56.0)          # 42 + 38 costs the same rounds: the tie goes to the even split
    assert _plan(plan_check, 40) == ([40], 28.0) and _plan(plan_check, 42) == ([42], 28.0)
    plan, units = _plan(plan_check, 100)
    assert sorted(plan) == [16, 42, 42] and units < 76.75     # the equal split, 34 + 34 + 32, counts 76.75
    assert _plan(plan_check, 7, tokens=48, cap=256)[0] == [4, 3]      # the ragged case tests/test_encode_plan_gpu.py runs
    assert _plan(plan_check, 20, tokens=196)[0] == [20]
