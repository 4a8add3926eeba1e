"""Records tests/golden/select_batch_cases.json: what the reference's ``select_batch`` and ``get_args_parser`` (must3r/engine/train.py) return over a grid
that takes every branch of ``select_batch``.

    python scripts/make_train_fixture.py [--reference ROOT] [--out tests/golden/select_batch_cases.json]

The two functions are read out of the reference's file when this runs (its other imports -- croco, dust3r, tensorboard -- are not needed for them and are
not touched) and executed; the file stores arguments and results only, and the torch version beside them, since ``torch.randperm``'s stream belongs to torch.
tests/test_train_loop_host.py replays the file against must3r_amd.train, and the grid live against the reference where its tree exists.
"""
import argparse
import ast
import itertools
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIMGS = 6
SEEDS = (0, 1, 2, 3)


def reference_functions(reference_root):
    """``(select_batch, get_args_parser)`` of ``reference_root/must3r/engine/train.py``, compiled from the file's own text"""
    path = os.path.join(reference_root, "must3r", "engine", "train.py")
    with open(path) as f:
        text = f.read()
    wanted = ("get_args_parser", "select_batch")
    nodes = [n for n in ast.parse(text).body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(n.name for n in nodes) == sorted(wanted), path
    ns = {"argparse": argparse, "math": math, "torch": torch}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns["select_batch"], ns["get_args_parser"]


def grid():
    """every branch: memory_num_views below (2: a curriculum that starts with no unseen view; 3), equal to and above the number of views; render_once, causal,
    memory_batch_views, progress, seeds"""
    for mnv, render_once, causal, mbv, progress, seed in itertools.product((2, 3, NIMGS, 10), (False, True), (False, True), (None, 3), (0.0, 0.5, 1.0), SEEDS):
        yield dict(memory_num_views=mnv, render_once=render_once, causal=causal, memory_batch_views=mbv, progress=progress, seed=seed,
                   loader_memory_num_views=min(mnv, NIMGS - 1), nimgs=NIMGS)


def case_args(parser, case):
    argv = ["--dataset", "none", "--memory_num_views", str(case["memory_num_views"])]
    argv += ["--render_once"] if case["render_once"] else []
    argv += ["--causal"] if case["causal"] else []
    argv += ["--memory_batch_views", str(case["memory_batch_views"])] if case["memory_batch_views"] is not None else []
    return parser.parse_args(argv)


def run_case(select_batch, parser, case):
    """the JSON-able result of one case: the seeds of the loop (numpy Generator and torch's global generator), inputs that show which views were kept"""
    args = case_args(parser, case)
    rng = np.random.default_rng(seed=case["seed"])
    torch.manual_seed(case["seed"])
    n = case["nimgs"]
    imgs = torch.arange(n, dtype=torch.float32).view(1, n, 1, 1, 1).expand(1, n, 3, 2, 2)
    true_shape = torch.stack([torch.arange(n), torch.arange(n) + 100], dim=-1).view(1, n, 2)
    imgs, true_shape, mnv, to_skip, to_render, to_skip_batches, mem_batches = select_batch(
        "cpu", args, rng, case["loader_memory_num_views"], case["progress"], imgs, true_shape, n)
    assert imgs.is_contiguous() or imgs.shape[1] == n
    if isinstance(to_render, torch.Tensor):
        to_render = to_render.tolist()
    return dict(kept=imgs[0, :, 0, 0, 0].to(torch.int64).tolist(), kept_shapes=true_shape[0, :, 0].tolist(), memory_num_views=int(mnv), to_skip=int(to_skip),
                to_render=None if to_render is None else [int(i) for i in to_render], to_skip_batches=[int(i) for i in to_skip_batches],
                mem_batches=[int(i) for i in mem_batches], next_choice=int(rng.choice(1 << 30)), next_randperm=torch.randperm(8).tolist())


def parser_table(parser):
    """per option: its strings, default, type name, choices, required flag and whether it is a switch"""
    rows = []
    for a in parser._actions:
        rows.append(dict(dest=a.dest, options=list(a.option_strings), default=a.default, type=getattr(a.type, "__name__", None), choices=a.choices and list(a.choices),
                         required=bool(a.required), switch=a.nargs == 0))
    groups = [sorted(a.dest for a in g._group_actions) for g in parser._mutually_exclusive_groups]
    return dict(prog=parser.prog, add_help=parser.add_help, options=rows, exclusive=sorted(groups))


def build(reference_root):
    select_batch, get_args_parser = reference_functions(reference_root)
    parser = get_args_parser()
    cases = [dict(case=c, result=run_case(select_batch, parser, c)) for c in grid()]
    return dict(torch_version=torch.__version__, numpy_version=np.__version__, parser=parser_table(parser), cases=cases)


def main():
    sys.path.insert(0, ROOT)
    from oracle.ref_shims import REFERENCE_ROOT
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", default=REFERENCE_ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "select_batch_cases.json"))
    a = ap.parse_args()
    data = build(a.reference)
    with open(a.out, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    branches = {(c["result"]["to_skip"] > 0, c["result"]["to_render"] is None, len(c["result"]["mem_batches"])) for c in data["cases"]}
    print(f"{a.out}: {len(data['cases'])} cases, {len(branches)} distinct (skipped, renders all, updates) outcomes, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
