"""The stream contract of a context (gs_set_stream, gs_stream_wait, gs_stream_signal,
gs_set_async), tested through ``Context.call`` with work that is really still pending.

Everywhere else in the suite a device input is complete on the host's clock before the
library is called, so a ``gs_stream_wait`` that did nothing would pass.  Here the producer
is held back by a delay kernel on torch's stream: the input (or the output block's last use
by torch) is written only after the delay, and an event recorded behind it is still
unfinished when the library call is issued.  Each test has a control that takes the ordering
away and must then *not* give the reference -- reading the NaN / zero poison is harmless.

Entry points: gs_feature_cosine_f32 (device x), gs_degree (no device input: its device
output block is what torch's stream uses last), gs_adamic_adar (device c) and gs_topk_mask
(device scores, device mask).  Tests 3 and 4 need calls that make no host round trip; read
in csrc/gs_scores.hip: gs_feature_cosine_*, gs_degree and gs_adamic_adar with device
inputs and a device output launch their kernels and end in finish_out, which for a device
output only synchronises outside async mode; they copy nothing to the host and allocate
nothing once scratch[0] has its size (a warm-up call at the same shapes comes first, since
growing a buffer frees the old one, which waits for the device).  gs_topk_mask returns its
cut through the host and is left out of 3 and 4.

The delay is 50 times the measured duration of the test's own library call, at least 20 ms,
from torch.cuda._sleep calibrated once per module with two events (a chain of matmuls if
_sleep does not behave).

Streams: torch's default, s1, s2 and the one context's own -- four, and no test makes
another context.  Every control assumes that two of them really run side by side: work on
the library's stream must finish while the delay holds torch's stream, or the "missing"
wait happens anyway and the control reads the true input.  That is not a given: the runtime
maps streams onto a few hardware queues (four by default), two streams on one queue run in
order, and in a process that has already made other contexts and streams (the whole suite)
a new stream can land on a queue that is taken.  So the fixture checks the precondition
rather than assuming it: it picks the context, s1 and s2 so that each pair a test relies on
overlaps (``_overlap``: work on the one completes while a delay holds the other), trying a
further candidate only when a pair shares a queue, and fails -- never skips -- when none
does; ``test_the_streams_overlap`` asserts the chosen pairs again."""

import time

import numpy as np
import pytest
import torch

import gsparse_oracle as O
import reuse_cases as C
from conftest import bits_equal

pytestmark = pytest.mark.gpu

CASES = ("feature_cosine", "degree", "adamic_adar", "topk_mask")
NO_ROUND_TRIP = ("feature_cosine", "degree", "adamic_adar")
MIN_DELAY_MS, DELAY_FACTOR = 20.0, 50.0


class Delay:
    """A kernel that keeps a stream busy for a given time; calibrated once."""

    def __init__(self):
        torch.cuda.synchronize()
        self.kind, self.per_ms = "sleep", self._calibrate(lambda k: torch.cuda._sleep(k), 20_000_000)
        if self.per_ms is None:
            self.a = torch.randn(4096, 4096, device="cuda")
            self.kind, self.per_ms = "matmul", self._calibrate(self._matmuls, 20)
        assert self.per_ms is not None, "no way to delay a stream on this device"

    def _matmuls(self, k):
        for _ in range(int(k)):
            self.a @ self.a

    @staticmethod
    def _calibrate(fn, units):
        fn(max(units // 20, 1))  # warm up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn(units)
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        return units / ms if ms >= 1.0 else None

    def enqueue(self, ms):
        """On torch's current stream."""
        units = max(int(ms * self.per_ms), 1)
        (torch.cuda._sleep if self.kind == "sleep" else self._matmuls)(units)


class Case:
    """One entry point with device-resident input and output on the shared graph."""

    def __init__(self, eng, name):
        ip, ix, _ = C.csr("G1")
        n, nnz = len(ip) - 1, len(ix)
        self.name, self.eng = name, eng
        f64 = dict(dtype=torch.float64, device="cuda")
        self.out = torch.empty(nnz, **f64)
        self.poison_out = float("nan")
        self.inp = self.true = None
        if name == "feature_cosine":
            self.true = torch.from_numpy(np.array(C.features("G1"))).cuda()
            self.ref = C.ref("G1", "feature_cosine")
            self.run = lambda: eng.feature_cosine(self.inp, out=self.out)
        elif name == "degree":
            self.ref = C.ref("G1", "degree")
            self.run = lambda: eng.degree(out=self.out)
        elif name == "adamic_adar":
            self.true = torch.from_numpy(np.array(O.aa_weights(ip))).cuda()
            self.ref = C.ref("G1", "adamic_adar")
            self.run = lambda: eng.adamic_adar(out=self.out, c=self.inp)
        elif name == "topk_mask":
            s = np.random.default_rng(3).integers(1, 40, nnz) / 8.0
            self.true = torch.from_numpy(s).cuda()
            self.ref = O.topk_mask(s, nnz, 0.3, False, kind="stable")
            self.out = torch.empty(nnz, dtype=torch.uint8, device="cuda")
            self.poison_out = 7
            self.run = lambda: eng.topk_mask(self.inp, nnz, int(nnz * 0.3), False, out=self.out)
        if self.true is not None:
            self.inp = torch.empty_like(self.true)
        self.spare = torch.empty_like(self.out)  # what a clone of the output will reuse
        torch.cuda.synchronize()

    def fill(self, true_input):
        """Input = the true values or NaN poison, output = poison; complete on return."""
        if self.inp is not None:
            self.inp.copy_(self.true) if true_input else self.inp.fill_(float("nan"))
        self.out.fill_(self.poison_out)
        torch.cuda.synchronize()

    def late(self):
        """What torch's stream does behind the delay: produce the input; for the call without
        one, use the output block last."""
        if self.inp is not None:
            self.inp.copy_(self.true)
        else:
            self.out.fill_(self.poison_out)

    def call_ms(self):
        """Wall time of one complete call in the default mode, buffers at their sizes."""
        self.fill(True)
        self.run()
        t = time.perf_counter()
        self.run()
        ms = (time.perf_counter() - t) * 1e3
        assert self.matches(self.result())
        return ms

    def result(self, t=None):
        return (self.out if t is None else t).cpu().numpy()

    def matches(self, got):
        if self.name == "topk_mask":  # mask bytes, 0 / 1
            return np.array_equal(got, self.ref.astype(np.uint8))
        return bits_equal(got, self.ref)


@pytest.fixture(scope="module")
def env():
    from gsparse._lib import Context
    from gsparse.engine import Engine

    delay = Delay()
    default = torch.cuda.default_stream()
    n, ei = C.graph("G1")
    ctx, rejected = None, []  # a rejected candidate stays alive so that the next gets another queue
    for _ in range(4):
        c = Context(0)
        c.set_graph_edge_index(n, np.array(ei[0]), np.array(ei[1]))
        if _overlap(delay, default, _library_probe(c)):
            ctx = c
            break
        rejected.append(c)
    assert ctx is not None, "no context whose stream runs beside torch's default stream"
    lib = _library_probe(ctx)
    s1 = s2 = None
    for _ in range(8):
        s = torch.cuda.Stream()
        if s1 is None and _overlap(delay, s, lib):
            s1 = s
        elif s2 is None and _overlap(delay, s, lib) and _overlap(delay, s, _torch_probe(default)):
            s2 = s
        if s1 is not None and s2 is not None:
            break
    for c in rejected:
        c.close()
    assert s1 is not None and s2 is not None, "no two torch streams that run beside the library's"
    eng = Engine(ctx)
    e = {"ctx": ctx, "eng": eng, "delay": delay, "s1": s1, "s2": s2,
         "cases": {k: Case(eng, k) for k in CASES}}
    yield e
    torch.cuda.synchronize()
    ctx.close()


def _library_probe(ctx):
    """A small library call on the context's stream with no ordering against torch (the ABI
    directly, not Context.call), complete at return."""
    from gsparse._lib import GS_HOST, check, ptr

    nnz = ctx.shape()[1]
    buf = np.empty(max(nnz, 1), dtype=np.float64)

    def run():
        check(ctx._L.gs_degree(ctx.handle, 0, nnz, ptr(buf), GS_HOST), "gs_degree")

    run()  # buffers at their sizes
    return run


def _torch_probe(stream):
    t = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()

    def run():
        with torch.cuda.stream(stream):
            t.add_(1.0)
        stream.synchronize()

    return run


def _overlap(delay, held, other):
    """Whether the work ``other()`` issues and waits for completes while a delay keeps the
    stream ``held`` busy: the two do not share a hardware queue."""
    torch.cuda.synchronize()
    with torch.cuda.stream(held):
        delay.enqueue(MIN_DELAY_MS)
        ev = torch.cuda.Event()
        ev.record()
    other()
    beside = not ev.query()
    torch.cuda.synchronize()
    return beside


def test_the_streams_overlap(env):
    """The precondition of every control below, for the pairs the tests use."""
    ctx, delay, s1, s2 = env["ctx"], env["delay"], env["s1"], env["s2"]
    lib, default = _library_probe(ctx), torch.cuda.default_stream()
    assert _overlap(delay, default, lib), "library stream behind torch's default stream"
    assert _overlap(delay, s1, lib), "library stream behind s1"
    assert _overlap(delay, s2, lib), "library stream behind s2"
    assert _overlap(delay, s2, _torch_probe(default)), "torch's default stream behind s2"
    assert len({default.cuda_stream, s1.cuda_stream, s2.cuda_stream}) == 3


@pytest.fixture
def clean(env):
    """Every test leaves the context in the default mode on its own stream."""
    try:
        yield env
    finally:
        torch.cuda.synchronize()
        env["ctx"].set_async(False)
        env["ctx"].set_stream(None)


def _delay_ms(case):
    call = case.call_ms()
    ms = max(MIN_DELAY_MS, DELAY_FACTOR * call)
    print(f"{case.name}: call {call:.3f} ms, delay {ms:.1f} ms")
    return ms


def _late_producer(env, case):
    """Poison, then on torch's current stream the delay and the producer, then the call.
    -> (result, whether the producer was still pending when the call was issued, delay)."""
    ms = _delay_ms(case)
    case.fill(False)
    env["delay"].enqueue(ms)
    case.late()
    ev = torch.cuda.Event()
    ev.record()
    pending = not ev.query()
    case.run()
    torch.cuda.synchronize()
    return case.result(), pending, ms


def _without_the_wait(monkeypatch):
    from gsparse._lib import Context

    monkeypatch.setattr(Context, "_torch_stream", lambda self: None)


@pytest.mark.parametrize("name", CASES)
def test_late_producer(clean, name, monkeypatch):
    env, case = clean, clean["cases"][name]
    got, pending, ms = _late_producer(env, case)
    assert pending, f"{name}: the producer had finished before the call (delay {ms:.1f} ms)"
    assert case.matches(got), f"{name}: the call did not wait for its producer (delay {ms:.1f} ms)"
    with monkeypatch.context() as m:  # control: no gs_stream_wait -> the poison is read
        _without_the_wait(m)
        got, pending, ms = _late_producer(env, case)
    assert pending, f"{name}: control, the producer had finished (delay {ms:.1f} ms)"
    assert not case.matches(got), f"{name}: the control cannot see a missing wait (delay {ms:.1f} ms)"


def _late_graph(env, ctx):
    """src / dst tensors that hold zeros until the delay has passed -> (the CSR the context
    built from them, whether they were still pending at the call, the delay)."""
    n, ei = C.graph("G2")
    true = [torch.from_numpy(np.array(r)).cuda() for r in ei]
    late = [torch.zeros_like(t) for t in true]
    torch.cuda.synchronize()
    ctx.set_graph_edge_index(n, true[0], true[1])  # buffers at their sizes, then the timed call
    t = time.perf_counter()
    ctx.set_graph_edge_index(n, true[0], true[1])
    call = (time.perf_counter() - t) * 1e3
    ms = max(MIN_DELAY_MS, DELAY_FACTOR * call)
    print(f"set_graph_edge_index: call {call:.3f} ms, delay {ms:.1f} ms")
    env["delay"].enqueue(ms)
    for a, b in zip(late, true):
        a.copy_(b)
    ev = torch.cuda.Event()
    ev.record()
    pending = not ev.query()
    ctx.set_graph_edge_index(n, late[0], late[1])
    got = ctx.csr()
    torch.cuda.synchronize()
    return got, pending, ms


def test_graph_from_late_tensors_on_a_side_stream(clean, monkeypatch):
    """On the shared context (no further stream), G1 put back afterwards."""
    env, ctx = clean, clean["ctx"]
    want = O.canonical_csr(C.graph("G2")[1], C.graph("G2")[0])
    try:
        with torch.cuda.stream(env["s1"]):
            got, pending, ms = _late_graph(env, ctx)
            assert pending, f"the ids were complete before the call (delay {ms:.1f} ms)"
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), f"delay {ms:.1f} ms"
            with monkeypatch.context() as m:  # control: the zeros are read, one entry (0, 0)
                _without_the_wait(m)
                got, pending, ms = _late_graph(env, ctx)
            assert pending, f"control: the ids were complete before the call (delay {ms:.1f} ms)"
            assert not np.array_equal(got[1], want[1]), \
                f"the control cannot see a missing wait (delay {ms:.1f} ms)"
    finally:
        torch.cuda.synchronize()
        n, ei = C.graph("G1")
        ctx.set_graph_edge_index(n, np.array(ei[0]), np.array(ei[1]))
    assert ctx.shape()[:2] == (env["eng"].n, env["eng"].nnz)
    assert bits_equal(env["eng"].degree(), C.ref("G1", "degree"))


@pytest.mark.parametrize("name", CASES)
def test_late_producer_on_a_side_stream(clean, name, monkeypatch):
    env, case = clean, clean["cases"][name]
    with torch.cuda.stream(env["s1"]):
        assert torch.cuda.current_stream() == env["s1"]
        got, pending, ms = _late_producer(env, case)
        assert pending, f"{name}: the producer had finished before the call (delay {ms:.1f} ms)"
        assert case.matches(got), f"{name}: no wait for the side stream's producer (delay {ms:.1f} ms)"
        with monkeypatch.context() as m:
            _without_the_wait(m)
            got, pending, ms = _late_producer(env, case)
        assert pending, f"{name}: control, the producer had finished (delay {ms:.1f} ms)"
        assert not case.matches(got), f"{name}: the control cannot see a missing wait (delay {ms:.1f} ms)"


def _async_call(env, case, signal=True):
    """The library on s2 behind the delay, async mode -> (clone of the output taken on torch's
    current stream right after the call, whether s2 was still busy at return, delay)."""
    ctx, s2 = env["ctx"], env["s2"]
    ctx.set_async(False)
    ctx.set_stream(s2.cuda_stream)
    ms = _delay_ms(case)
    case.fill(True)
    ctx.set_async(True)
    if not signal:
        ctx._async = False  # the library stays in async mode, the shim no longer signals
    with torch.cuda.stream(s2):
        env["delay"].enqueue(ms)
    case.run()
    busy = not s2.query()
    case.spare.copy_(case.out)  # on torch's current stream, no other ordering
    torch.cuda.synchronize()
    return case.result(case.spare), busy, ms


@pytest.mark.parametrize("name", NO_ROUND_TRIP)
def test_async_device_outputs(clean, name):
    env, case = clean, clean["cases"][name]
    got, busy, ms = _async_call(env, case)
    assert busy, f"{name}: the async call waited on the host (delay {ms:.1f} ms)"
    assert case.matches(got), f"{name}: torch's stream read the output too early (delay {ms:.1f} ms)"
    got, busy, ms = _async_call(env, case, signal=False)  # control: no gs_stream_signal
    assert busy, f"{name}: control, the call waited on the host (delay {ms:.1f} ms)"
    assert not case.matches(got), f"{name}: the control cannot see a missing signal (delay {ms:.1f} ms)"
    assert np.isnan(got).all()


def test_async_host_outputs_are_complete_at_return(clean):
    env, ctx, s2 = clean, clean["ctx"], clean["s2"]
    ctx.set_stream(s2.cuda_stream)
    ctx.set_async(True)
    with torch.cuda.stream(s2):
        env["delay"].enqueue(MIN_DELAY_MS)
    busy = not s2.query()
    got = env["eng"].degree()
    assert busy and bits_equal(got, C.ref("G1", "degree"))
    x = torch.from_numpy(np.array(C.features("G1"))).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        env["delay"].enqueue(MIN_DELAY_MS)
    assert bits_equal(env["eng"].feature_cosine(x), C.ref("G1", "feature_cosine"))


@pytest.mark.parametrize("name", NO_ROUND_TRIP)
def test_set_stream(clean, name):
    env, case, ctx, s2 = clean, clean["cases"][name], clean["ctx"], clean["s2"]
    ctx.set_stream(s2.cuda_stream)
    ms = _delay_ms(case)
    case.fill(True)
    with torch.cuda.stream(s2):
        env["delay"].enqueue(ms)
    ctx.set_stream(None)  # the context's own stream: not behind the delay
    case.run()
    busy = not s2.query()
    got = case.result()
    assert busy, f"{name}: after set_stream(None) the call still ran behind s2 (delay {ms:.1f} ms)"
    assert case.matches(got)
    # back on s2 with the delay still pending there (no synchronisation since it was enqueued;
    # the poison fill is on torch's stream, which the call orders itself after): still right
    case.out.fill_(case.poison_out)
    ctx.set_stream(s2.cuda_stream)
    still = not s2.query()
    case.run()
    assert still, f"{name}: the delay on s2 had run out before the second call (delay {ms:.1f} ms)"
    assert case.matches(case.result())


@pytest.mark.parametrize("name", CASES)
def test_sync_mode_output_is_complete_for_any_stream(clean, name):
    """Default mode, the library's stream held back by the delay: at return the device output
    is final for a stream that was never ordered with anything."""
    env, case, ctx = clean, clean["cases"][name], clean["ctx"]
    ctx.set_stream(env["s2"].cuda_stream)
    ms = _delay_ms(case)
    case.fill(True)
    with torch.cuda.stream(env["s2"]):
        env["delay"].enqueue(ms)
    case.run()
    with torch.cuda.stream(env["s1"]):
        case.spare.copy_(case.out)
    env["s1"].synchronize()
    assert case.matches(case.result(case.spare)), f"{name} (delay {ms:.1f} ms)"
