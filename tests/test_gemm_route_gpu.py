"""GPU (-m gpu): what the library launches under non-default options is what tests/c/gemm_route_check.cpp answers for the same input -- the glue between the rule
(must3r_amd/csrc/gemm_route.hpp) and the launch, the filling of GemmOpts from the option table and of GemmShape from the arguments, which the host checks of
tests/test_gemm_route_host.py cannot see.  Two small fp16 launches (K = 64, EPI_STORE16: 256 x 256 plain, 256 x 128 split) under five settings of the 256-row switches:
`picked` of must3r_hip_op_gemm_ex equals the program's line, and the output equals the default-option output of the same operands bit for bit (options.hpp)."""
import pytest
import torch

import gemm_forms as F
from test_gemm_forms_gpu import DEFAULTS, launch
from test_gemm_route_host import ask, opt_line, route_check, shape_line   # noqa: F401 (route_check: the fixture that builds the program)

pytestmark = pytest.mark.gpu
SHAPES = (("plain", 256, 256), ("split", 256, 128))
SETTINGS = (dict(GEMM256=2), dict(GEMM256=2, G256P=0), dict(GEMM256=2, G256P=0, G256K=0), dict(GEMM256=2, G256P_SPLIT=0), dict(GEMM256=0))


def test_library_launches_what_the_rule_answers(route_check):
    from must3r_amd import _lib
    lines = []
    for setting in ({},) + SETTINGS:
        lines.append(opt_line(**setting))
        lines += [shape_line(F.EPI_STORE16, M, N, 64, 0 if weights == "plain" else 2) for weights, M, N in SHAPES]
    want = ask(route_check, lines)
    assert len(want) == 2 * (1 + len(SETTINGS)) and len(set(want)) >= 6, want      # the settings do move these launches
    try:
        for n, v in DEFAULTS:
            _lib.set_option(n, v)
        base = []
        for i, (weights, M, N) in enumerate(SHAPES):
            ops = F.make_operands(F._case("route", f"route-{weights}", F.EPI_STORE16, N, 64, M), "fp16", weights, "cuda")
            outs = F.alloc_outputs(ops, "cuda")
            assert launch(_lib, ops, outs) == want[i] == ops["kernel"]
            F.check_canaries(ops, outs)
            base.append((ops, outs))
        for j, setting in enumerate(SETTINGS):
            for n, v in setting.items():
                _lib.set_option(n, v)
            for i, (ops, outs0) in enumerate(base):
                outs = F.alloc_outputs(ops, "cuda")
                picked = launch(_lib, ops, outs)
                print(setting, SHAPES[i], picked)
                assert picked == want[2 * (j + 1) + i], (setting, SHAPES[i])
                assert torch.equal(outs["buf"], outs0["buf"]), (setting, SHAPES[i], "bits differ from the default-option output")
            for n, v in DEFAULTS:
                _lib.set_option(n, v)
    finally:
        for n, v in DEFAULTS:
            _lib.set_option(n, v)
