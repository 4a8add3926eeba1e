"""GPU (-m gpu): every entry point with a stream argument runs wholly on the caller's stream (include/must3r_hip.h, "stream order").

Per case of tests/stream_forms.py: the reference bits of the two input sets A and B on the default stream (A twice: repeatable), then on a non-blocking side
stream, with the inputs holding the decoy B: a delay, copies of A into the inputs, the call, clones of the outputs, B and the byte pattern back -- all queued
without a host synchronisation.  The clones must be A's reference bits, and the delay must still be running when the call returns on the host (the premise:
the whole call was queued while its inputs held the decoy).  A launch, memset or copy of the call that goes to another stream than the caller's reads the
decoy or the pattern, or has its result overwritten, and the bits differ.  The control shows that the check can see that: the same call sent to the null
stream (legal: every read is of valid data) reproduces B's reference bits, one case per source file.

The side stream is one that the null stream is seen to overtake (Delay.overtakes): streams share a few hardware queues, and a mis-streamed launch that lands in
the queue of the delayed stream would wait behind the delay and read the right inputs.

Then the staging rings: many calls behind one delay (more calls than a ring has slots) and two host threads on two streams.

Every row (delay, host time of the call, GPU time of the call, whether the premise held) goes through record() to the suite's metrics file and, as a table, to the file
M3R_STREAM_ORDER_TABLE names (kept as profiles/stream_order.txt).
"""
import contextlib
import os
import threading
import time

import pytest
import torch

import stream_forms as SF
from must3r_amd import _lib
from test_ops_gpu import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELAY_CAP_MS = 250.0
_rows = {}      # case -> dict of the table's columns


# ---------------------------------------------------------------------------------------------------------------------------------
# the delay: one thread spinning on the side stream (torch.cuda._sleep), a chain of dependent skinny matmuls where that returns at once
# ---------------------------------------------------------------------------------------------------------------------------------
class Delay:
    def __init__(self):
        self.stream = torch.cuda.Stream()
        self.kind, self.per_ms = "sleep", None
        self.side, self.picked, self.probe = None, 0, torch.zeros((64,), device=DEV)
        cycles = 20_000_000
        ms = self._measure(lambda: torch.cuda._sleep(cycles))
        ms = self._measure(lambda: torch.cuda._sleep(cycles))
        if ms > 1.0:
            self.per_ms = cycles / ms
        else:
            self.kind = "matmul"
            self.w = torch.randn((8192, 8192), device=DEV) / 90.0
            self.x = torch.randn((16, 8192), device=DEV)
            self._chain(20)
            ms = self._measure(lambda: self._chain(200))
            self.per_ms = 200 / ms
        self.measured = {ms_: self.measure_ms(ms_) for ms_ in (40.0,)}

    def _chain(self, n):
        x = self.x
        for _ in range(int(n)):
            x = x @ self.w
        self.x = x.clamp_(-1.0, 1.0)

    def _measure(self, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            e0.record()
            fn()
            e1.record()
        self.stream.synchronize()
        return e0.elapsed_time(e1)

    def enqueue(self, ms):
        """on the current stream"""
        n = max(1, int(ms * self.per_ms))
        if self.kind == "sleep":
            torch.cuda._sleep(n)
        else:
            self._chain(n)

    def measure_ms(self, ms):
        return self._measure(lambda: self.enqueue(ms))

    def overtakes(self, s):
        """Does work on the null stream overtake a delay on ``s``?  Streams share the process's few hardware queues, and inside one queue work runs in the
        order of submission: a side stream that shares its queue with the null stream would hold a mis-streamed launch back behind the delay, where it reads
        the right inputs -- the check would see nothing."""
        ev = torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            self.enqueue(5.0)
            ev.record()
        self.probe.add_(1.0)                                # one kernel on the null stream
        torch.cuda.default_stream().synchronize()
        free = not ev.query()
        s.synchronize()
        return free

    def side_stream(self):
        """a non-blocking stream that the null stream overtakes, checked again at every use"""
        if self.side is None or not self.overtakes(self.side):
            tried = []
            for _ in range(33):                             # torch hands its pool of 32 streams out in turn
                tried.append(torch.cuda.Stream())
                if self.overtakes(tried[-1]):
                    break
            else:
                raise AssertionError("no side stream whose delay the null stream overtakes")
            self.side = tried[-1]
            self.picked += 1
        return self.side


@pytest.fixture(scope="module")
def delay():
    d = Delay()
    record("stream_order_delay", kind=d.kind, units_per_ms=d.per_ms, asked_ms=40.0, measured_ms=d.measured[40.0])
    # the delay is what it is asked to be, within a factor of two: the premise below does not rest on this, only the choice of its length
    assert 20.0 < d.measured[40.0] < 80.0, d.measured
    yield d
    path = os.environ.get("M3R_STREAM_ORDER_TABLE")
    if _rows and path:
        with open(path, "w") as f:
            f.write("# tests/test_stream_order_gpu.py: per case of tests/stream_forms.py, the delay queued in front of the call on the side stream (ms, measured alone for\n"
                    "# the asked length), the host time of the call behind it and of the same call on the default stream, and its GPU time there (events).  premise: the\n"
                    "# delay had not finished when the call returned on the host (asserted for every case that does not synchronise by contract).  bits: the side-stream\n"
                    "# outputs equal the default-stream reference of the same inputs.  control: the same call on the null stream gives the DECOY's reference bits.\n"
                    f"# delay: {d.kind}, {d.per_ms:.4g} units per ms; 40 ms asked = {d.measured[40.0]:.1f} ms measured\n")
            f.write(f"{'case':<24}{'file':<20}{'entries':>8}{'delay ms':>10}{'host ms':>9}{'host0 ms':>10}{'op ms':>9}{'syncs':>7}{'premise':>9}{'bits':>6}{'control':>9}\n")
            for name, r in _rows.items():
                f.write(f"{name:<24}{r['file']:<20}{r['entries']:>8}{r['delay_ms']:>10.1f}{r['host_ms']:>9.3f}{r['host0_ms']:>10.3f}{r['op_ms']:>9.3f}{str(r['syncs']):>7}"
                        f"{str(r['premise']):>9}{str(r['bits']):>6}{r.get('control', '-'):>9}\n")
            f.write("# syncs = True: " + "; ".join(f"{c.name}: {c.reason}" for c in SF.CASES if c.syncs) + "\n")


# ---------------------------------------------------------------------------------------------------------------------------------
# a case on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    """names whose bits differ"""
    assert set(a) == set(b)
    return [k for k in a if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not torch.equal(_bytes(a[k]), _bytes(b[k]))]


def differing_fraction(a, b):
    n = d = 0
    for k in a:
        x, y = _bytes(a[k]).view(-1, a[k].element_size()), _bytes(b[k]).view(-1, b[k].element_size())
        n += x.shape[0]
        d += int((x != y).any(dim=1).sum())
    return d / max(n, 1)


class Bound:
    def __init__(self, case):
        self.case, self.spec = case, case.spec()
        sp = self.spec
        self.src = {"A": {k: v.to(DEV) for k, v in sp.A.items()}, "B": {k: v.to(DEV) for k, v in sp.B.items()}}
        self.d = {k: torch.empty_like(v) for k, v in self.src["A"].items()}
        self.bufs = []
        for name, b in sp.bufs.items():
            self.d[name] = torch.empty((b(),), dtype=torch.uint8, device=DEV) if callable(b) else torch.empty(b[0], dtype=b[1], device=DEV)
            self.bufs.append(name)
        self.fill()
        if sp.prepare:
            sp.prepare(self.d)
        torch.cuda.synchronize()

    def load(self, which):
        """device-to-device copies on the current stream"""
        for k, v in self.src[which].items():
            self.d[k].copy_(v)

    def fill(self):
        for name in self.bufs:
            _bytes(self.d[name]).fill_(SF.PATTERN)

    def call(self):
        extra = self.spec.run(self.d) or {}
        outs = {k: self.d[k] for k in self.spec.outs}
        outs.update({k: v for k, v in extra.items() if v is not None})
        assert outs, "a case without outputs"
        return outs

    def reference(self, which, timed=False):
        self.load(which)
        self.fill()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        outs = self.call()
        host_ms = (time.perf_counter() - t0) * 1e3
        e1.record()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in outs.items()}
        torch.cuda.synchronize()
        return (got, host_ms, e0.elapsed_time(e1)) if timed else got


@contextlib.contextmanager
def null_stream():
    """every stream argument the wrappers and the table pass becomes the null stream (handle 0)"""
    keep = _lib.stream_ptr
    _lib.stream_ptr = lambda device: 0
    try:
        yield
    finally:
        _lib.stream_ptr = keep


_bound = {}


def bound(name):
    """the case on the device with its references: (Bound, ref_A, ref_B, host ms, op ms), once per case"""
    if name not in _bound:
        b = Bound(SF.CASE[name])
        ref_a = b.reference("A")              # (also grows the context workspace and the caches of the wrappers)
        ref_a2, host_ms, op_ms = b.reference("A", timed=True)
        bad = same_bits(ref_a, ref_a2)
        assert not bad, f"{name}: not repeatable on the default stream: {bad}"
        ref_b = b.reference("B")
        if b.spec.no_inputs:
            pat = {k: torch.full_like(_bytes(v), SF.PATTERN) for k, v in ref_a.items()}
            assert all(not torch.equal(_bytes(v), pat[k]) for k, v in ref_a.items())
        else:
            frac = differing_fraction(ref_a, ref_b)
            assert frac > 0.5, f"{name}: the outputs of the two input sets differ in {frac:.3f} of their elements only"
        _bound[name] = (b, ref_a, ref_b, host_ms, op_ms)
    return _bound[name]


def delay_for(host_ms):
    """long enough for the copies of A and the whole call to be queued behind it with margin: 10 x the host time of the call plus 30 ms, at most the cap"""
    return min(DELAY_CAP_MS, 30.0 + 10.0 * host_ms)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2 / 3: every case on a delayed side stream
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in SF.CASES])
def test_call_runs_on_the_callers_stream(delay, name):
    case = SF.CASE[name]
    b, ref_a, ref_b, host0_ms, op_ms = bound(name)
    ms = delay_for(host0_ms)
    b.load("B")
    b.fill()
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        b.load("A")
        if b.spec.no_inputs:
            b.fill()
        t0 = time.perf_counter()
        outs = b.call()
        host_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = {k: v.clone() for k, v in outs.items()}
        b.load("B")
        b.fill()
    s.synchronize()
    bad = same_bits(got, ref_a)
    row = dict(file=case.src, entries=len(case.entries), delay_ms=ms, host_ms=host_ms, host0_ms=host0_ms, op_ms=op_ms, syncs=case.syncs, premise=premise, bits=not bad)
    _rows.setdefault(name, {}).update(row)
    record("stream_order", case=name, **row)
    print(f"{name}: delay {ms:.1f} ms, host {host_ms:.3f} ms (default stream {host0_ms:.3f} ms), op {op_ms:.3f} ms, syncs {case.syncs}, premise {premise}, differing {bad}")
    if not case.syncs:
        assert premise, f"{name}: delay too short or undocumented host synchronisation (delay {ms:.1f} ms, the call took {host_ms:.3f} ms on the host)"
    frac = differing_fraction(got, ref_a) if bad else 0.0
    assert not bad, f"{name}: on a side stream {bad} differ from the default-stream bits ({frac:.3f} of all elements; equal to the decoy's: {not same_bits(got, ref_b)})"


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: the control -- a call on the null stream gives the decoy's bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in SF.CASES if c.control])
def test_control_call_on_the_null_stream_reads_the_decoy(delay, name):
    b, ref_a, ref_b, host0_ms, _ = bound(name)
    ms = delay_for(host0_ms)
    b.load("B")
    b.fill()
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(ms)
        done.record()
        b.load("A")                       # queued behind the delay: the inputs still hold the decoy
        with null_stream():
            outs = b.call()
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.cuda.default_stream().synchronize()
            got = {k: v.clone() for k, v in outs.items()}      # before the side stream moves on (in/out buffers are inputs too)
            torch.cuda.default_stream().synchronize()
        premise = not done.query()
    s.synchronize()
    bad = same_bits(got, ref_b)
    _rows.setdefault(name, {})["control"] = "ref_B" if premise and not bad else "FAILED"
    record("stream_order_control", case=name, delay_ms=ms, premise=premise, decoy_bits=not bad)
    assert premise, f"{name}: the delay ({ms:.1f} ms) ended before the null stream was idle"
    assert not bad, f"{name}: a call on the null stream did not give the decoy's bits in {bad} (A's: {not same_bits(got, ref_a)})"


# ---------------------------------------------------------------------------------------------------------------------------------
# many calls in a row behind one delay: the staging rings wrap
# ---------------------------------------------------------------------------------------------------------------------------------
def _resample_call(srcs_pairs, out):
    from must3r_amd import image
    srcs, pairs = srcs_pairs
    descs, _ = SF.resample_descs(srcs, pairs)
    image._resample(_lib.RESAMPLE_AA_BILINEAR, descs, out, srcs)
    return out


def _resample_jobs():
    """6 calls of one image each with 6 different size pairs (the ring has 4 pinned slots)"""
    jobs = []
    for i, pair in enumerate(SF.RESAMPLE_PAIRS):
        src = SF.resample_inputs([pair], 200 + i)(0)["src0"].to(DEV)
        jobs.append((([src], [pair]), 3 * pair[1][0] * pair[1][1]))
    return jobs


def test_six_resample_calls_behind_one_delay(delay):
    jobs = _resample_jobs()
    ref = [_resample_call(j, torch.empty((n,), device=DEV)).clone() for j, n in jobs]
    outs = [torch.full((n,), float("nan"), device=DEV) for _, n in jobs]
    torch.cuda.synchronize()
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(60.0)
        done.record()
        _resample_call(jobs[0][0], outs[0])
        premise = not done.query()
        for (j, _), o in zip(jobs[1:], outs[1:]):     # (the host may wait for a slot of the ring here: by design)
            _resample_call(j, o)
    s.synchronize()
    assert premise, "delay too short or undocumented host synchronisation"
    for i, (o, r) in enumerate(zip(outs, ref)):
        assert torch.equal(_bytes(o), _bytes(r)), f"call {i} of 6"


def _attn_jobs():
    """3 calls each of the forward and the backward with 3 different view tables: 6 uploads through the calling thread's ring of 4 pinned buffers"""
    d = {k: v.to(DEV) for k, v in SF.attn_train_inputs(0).items()}
    return d, [torch.tensor(t, dtype=torch.int32) for t in SF.ATTN_TABLES]


def _attn_calls(d, tabs):
    from must3r_amd import train_attention as TA
    q, k, v = SF._qkv(d)
    out = []
    for t in tabs:
        o, lse = TA.attention_forward(q, k, v, t, 2, want_lse=True)
        out += [o, lse, *TA.attention_grad(q, k, v, d["dO"], t, 2)]
    return out


def test_three_attention_tables_behind_one_delay(delay):
    d, tabs = _attn_jobs()
    ref = [t.clone() for t in _attn_calls(d, tabs)]
    torch.cuda.synchronize()
    assert any(not torch.equal(ref[0], ref[5 * i]) for i in (1, 2)), "the tables give different outputs"
    s = delay.side_stream()
    with torch.cuda.stream(s):
        delay.enqueue(60.0)
        got = _attn_calls(d, tabs)
        got = [t.clone() for t in got]
    s.synchronize()
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(_bytes(g), _bytes(r)), f"output {i % 5} of table {i // 5}"


def test_attention_sublayer_backward_alone_does_not_wait_for_the_stream(delay):
    """must3r_hip_attn_sublayer_grad uploads its table twice (forward recompute, backward).  Through ONE pinned buffer the second upload waited for the first,
    which is queued behind everything the stream still has to do: the call returned when the stream had drained (measured: 31.8 ms on the host behind a 31.6 ms
    delay, 0.16 ms on an idle stream).  The buffers are a ring now (csrc/train_attention.hip)."""
    from must3r_amd import train_block
    import block_ref
    b, ref_a, _, _, _ = bound("attn_sublayer")
    tab = torch.tensor(SF.NO_VIEW_TABLE, dtype=torch.int32)
    b.load("A")
    torch.cuda.synchronize()
    d = b.d
    p = [d[k] for k in block_ref.ATTN_PARAMS]
    s = delay.side_stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        delay.enqueue(40.0)
        done.record()
        t0 = time.perf_counter()
        got = train_block.attn_grad(d["x"], d["pos"], tab, d["tab"], *p, d["dy"])
        host_ms = (time.perf_counter() - t0) * 1e3
        premise = not done.query()
        got = [t.clone() for t in got]
    s.synchronize()
    record("stream_order_attn_sublayer_grad_alone", host_ms=host_ms, premise=premise)
    assert premise, f"the call took {host_ms:.3f} ms on the host behind a 40 ms delay"
    for n, g in zip(train_block.ATTN_OUTPUTS, got):
        assert torch.equal(_bytes(g), _bytes(ref_a[n])), n


def _scene(enc, dec, imgs, ts):
    from must3r_amd.engine import run_scene
    out = run_scene(enc, dec, imgs, ts)
    return {"update": out["update"], "render": out["render"], "conf": out["conf"], "pts3d": out["pts3d"], **{f"mem{i}": m for i, m in enumerate(out["mem"][0])}}


def test_six_frame_schedule_on_a_delayed_stream(delay):
    """the streaming schedule [2, 1, 1, 1, 1] and the render of the tiny configuration through engine.run_scene, every call of it on the side stream"""
    from must3r_amd import synthetic as S
    enc, dec = SF.tiny_modules()
    imgs, ts = S.make_images(6, SF.TINY_H, SF.TINY_W, 5)
    imgs = imgs.to(DEV)
    ref = {k: v.clone() for k, v in _scene(enc, dec, imgs, ts).items()}
    torch.cuda.synchronize()
    s = delay.side_stream()
    with torch.cuda.stream(s):
        delay.enqueue(60.0)
        got = {k: v.clone() for k, v in _scene(enc, dec, imgs, ts).items()}
    s.synchronize()
    bad = same_bits(got, ref)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# two host threads, two streams: the staging is per thread
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_threads_on_two_streams():
    from must3r_amd import train_attention as TA
    jobs = _resample_jobs()
    d, tabs = _attn_jobs()
    q, k, v = SF._qkv(d)

    def work(tid, outs):
        """20 alternating calls: resample of pair (2 i + tid) % 6, attention with table (i + tid) % 2"""
        for i in range(10):
            j, n = jobs[(2 * i + tid) % len(jobs)]
            outs.append(_resample_call(j, torch.empty((n,), device=DEV)))
            outs.append(TA.attention_forward(q, k, v, tabs[(i + tid) % 2], 2))

    ref = [[], []]
    for tid in (0, 1):
        work(tid, ref[tid])
    ref = [[t.clone() for t in r] for r in ref]
    torch.cuda.synchronize()
    got, errors = [[], []], []

    def thread(tid):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                work(tid, got[tid])
            s.synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append((tid, repr(e)))
    ts = [threading.Thread(target=thread, args=(tid,)) for tid in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for tid in (0, 1):
        assert len(got[tid]) == 20
        for i, (g, r) in enumerate(zip(got[tid], ref[tid])):
            assert torch.equal(_bytes(g), _bytes(r)), f"thread {tid}, call {i}"
