"""No GPU: the case table of the stream-order tests (tests/stream_forms.py) covers every entry point of include/must3r_hip.h that takes a stream, its two
input sets are different, valid data, and the entry points marked as synchronising are the documented ones."""
import os
import re

import pytest
import torch

import stream_forms as SF
from conftest import ROOT


def stream_entry_points():
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return re.findall(r"\bint\s+(must3r_hip_\w+)\s*\([^;{}]*?void\*\s*stream\s*\)\s*;", h)


def test_every_stream_entry_point_has_a_case():
    names = stream_entry_points()
    assert len(names) >= 55 and len(set(names)) == len(names)
    covered = {e for c in SF.CASES for e in c.entries}
    assert len(SF.EXCLUDED) <= 4 and all(isinstance(r, str) and r for r in SF.EXCLUDED.values())
    missing = [n for n in names if n not in covered and n not in SF.EXCLUDED]
    assert not missing, f"entry points with a stream argument and no case in tests/stream_forms.py: {missing}"
    unknown = sorted((covered | set(SF.EXCLUDED)) - set(names))
    assert not unknown, f"the table names entry points the header does not declare with a stream: {unknown}"
    assert not covered & set(SF.EXCLUDED)


def test_every_source_file_with_entry_points_has_a_control():
    """one control case per file of csrc/ that defines a stream entry point"""
    csrc = os.path.join(ROOT, "must3r_amd", "csrc")
    owners = {}
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith(".hip"):
            with open(os.path.join(csrc, fn)) as f:
                for n in re.findall(r'extern "C" int (must3r_hip_\w+)\(', f.read()):
                    owners[n] = fn
    names = stream_entry_points()
    assert all(n in owners for n in names)
    for c in SF.CASES:
        assert {owners[e] for e in c.entries} == {c.src}, (c.name, c.src)
    with_control = {c.src for c in SF.CASES if c.control}
    assert with_control == {owners[n] for n in names}, sorted({owners[n] for n in names} - with_control)


def test_syncs_set_is_the_documented_one():
    """must3r_hip_export_count is the one entry point whose declaration says that it synchronises the stream"""
    assert SF.SYNCS == {"export"}
    c = SF.CASE["export"]
    assert "must3r_hip_export_count" in c.entries and "synchronises" in c.reason
    with open(os.path.join(ROOT, "include", "must3r_hip.h")) as f:
        assert "the call synchronises `stream`" in f.read()
    assert all(c.reason for c in SF.CASES if c.syncs) and all(not c.syncs or c.reason for c in SF.CASES)


@pytest.mark.parametrize("name", [c.name for c in SF.CASES])
def test_input_sets_are_valid_and_different(name):
    spec = SF.CASE[name].spec()
    A, B = spec.A, spec.B
    assert set(A) == set(B)
    if spec.no_inputs:
        assert not A and spec.bufs and spec.outs
        return
    assert A, "a case without inputs must say so"
    for k in A:
        a, b = A[k], B[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.is_floating_point():
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{k}: the decoy is finite data too"
        if k in spec.shared:
            assert torch.equal(a, b), k
        else:
            assert not torch.equal(a, b), f"{k}: the two sets hold the same values"
            if a.is_floating_point() and a.numel() >= 16:
                assert float((a != b).float().mean()) > 0.5, k
    assert any(k not in spec.shared for k in A)
    for k, (lo, hi) in spec.ranges.items():
        for t in (A[k], B[k]):
            assert not t.is_floating_point() and int(t.min()) >= lo and int(t.max()) < hi, (k, lo, hi, int(t.min()), int(t.max()))
    # every integer input is either ranged or a mask / flag of 0 and 1
    for k, t in A.items():
        if not t.is_floating_point() and k not in spec.ranges:
            assert t.dtype == torch.uint8 and int(t.max()) <= 1, f"{k}: an index-like input without a range"
    for k in spec.outs:
        assert k in A or k in spec.bufs, k


def test_view_tables_stay_inside_their_rows():
    SF.check_views(SF.ATT_VIEWS, SF.ATT_RQ, SF.ATT_RK)
    SF.check_views(SF.NO_VIEW_TABLE, SF.NO_VIEW_ROWS, SF.NO_VIEW_ROWS)
    SF.check_views(SF.attn_train_table(), 210, 210)
    for tab in SF.ATTN_TABLES:
        SF.check_views(tab, 210, 210)
    with pytest.raises(AssertionError):
        SF.check_views([[0, 70, 0, 211, 0, 0]], 210, 210)
