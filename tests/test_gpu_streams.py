"""The stream contract of include/freepose_hip.h on the MI355X: every call enqueues ALL of its device work on the stream it is given, state
made by one call is safe to use from another stream once the caller has ordered the two, and no steady-state call drains the device.

The rest of the suite runs on torch's default stream, where a kernel, memset or copy enqueued on the wrong stream is ordered correctly by
accident.  Here every case of tests/_stream_cases.py runs on a side stream behind a delay kernel, with its inputs copied in behind that
delay: whatever the entry enqueues anywhere else runs at once, on the other input set, and shows in the bits.

  0. harness control   a side stream and a busy stream that provably run independently of the default stream on this machine
  1. late inputs       per case: the call on `side` returns while the delay is still running and gives the bits of the single-stream call
  2. hand-over         per stateful object, ffa and the mesh: state built on the default stream, used on `side` with a larger batch (the
                       workspaces regrow), used on the default stream again — the caller orders the streams, the bits are the single-stream ones
  3. steady state      per case: a warm call on the default stream neither waits for an unrelated busy stream (no device-wide wait, no
                       hipFree) nor changes the context's workspace total
  mutant control       the five value-only entries with the launch stream swapped for the default one: part 1 must report a mismatch"""
import ctypes as C
import gc

import pytest
import torch

from tests import _stream_cases as sc

pytestmark = pytest.mark.gpu

DELAY_MS = 300.0          # long against any enqueue of a case (milliseconds of Python and launches), short enough for ~170 delays per module run
MAX_STREAMS = 8


def _ops():
    from freepose_amd import ops
    return ops


# ---- 0. harness control -------------------------------------------------------------------------------------------------------------------
class Harness:
    def __init__(self, side, busy, cycles, delay_ms, tried, picked):
        self.side, self.busy, self.cycles, self.delay_ms, self.tried, self.picked = side, busy, cycles, delay_ms, tried, picked

    def delay(self):
        """torch's own spin kernel on the current stream: about DELAY_MS"""
        torch.cuda._sleep(self.cycles)


def _time_sleep(cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _calibrate():
    """cycles of torch.cuda._sleep for DELAY_MS, in three steps (a short spin is mostly launch overhead), and the delay they measure"""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    cycles = 1_000_000
    for target in (10.0, 100.0, DELAY_MS):
        ms = max(_time_sleep(cycles), 1e-3)
        cycles = max(1000, int(cycles * target / ms))
    return cycles, _time_sleep(cycles)


def _independent_of_default(stream, cycles):
    """a torch add on the default stream completes, and the default stream synchronises, while `stream` is still inside its delay"""
    x = torch.ones(1024, device="cuda")
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
    y = x + 1
    done.record()
    done.synchronize()
    torch.cuda.current_stream().synchronize()
    still_busy = not stream.query()
    stream.synchronize()
    return still_busy and bool((y == 2).all())


@pytest.fixture(scope="module")
def harness():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    cycles, delay_ms = _calibrate()
    assert 0.5 * DELAY_MS <= delay_ms <= 2.0 * DELAY_MS, f"torch.cuda._sleep({cycles}) measures {delay_ms:.1f} ms, not about {DELAY_MS:.0f}"
    found, picked, tried = [], [], 0
    keep = []                                       # streams that failed stay alive, so that torch hands out the next one of its pool
    while len(found) < 2 and tried < 2 * MAX_STREAMS:          # up to 8 for `side`, up to 8 more for `busy`
        s = torch.cuda.Stream()
        tried += 1
        keep.append(s)
        if _independent_of_default(s, cycles):
            found.append(s)
            picked.append(tried)
    if len(found) < 2:
        pytest.fail(f"the harness cannot discriminate on this machine: of {tried} fresh streams {len(found)} ran independently of the default stream "
                    f"(a delay of {delay_ms:.0f} ms on the stream held back work on the default stream), so a launch on the wrong stream could not be seen")
    h = Harness(found[0], found[1], cycles, delay_ms, tried, tuple(picked))
    print(f"\n[streams] delay {delay_ms:.1f} ms = torch.cuda._sleep({cycles}); side / busy = fresh streams no. {picked[0]} / {picked[1]} of {tried} tried; "
          f"cases: part 1 {len(sc.CASES)}, part 2 {len(sc.HANDOVER)}, part 3 {len(sc.CASES)}, mutants {len(sc.MUTANTS)}")
    return h


def test_harness_control(harness):
    """the fixture has proved both streams; here again, in the order the parts use them, and that they are three different streams"""
    default = torch.cuda.default_stream()
    assert len({default.cuda_stream, harness.side.cuda_stream, harness.busy.cuda_stream}) == 3
    assert _independent_of_default(harness.side, harness.cycles), "side stream"
    assert _independent_of_default(harness.busy, harness.cycles), "busy stream"
    assert harness.tried <= 2 * MAX_STREAMS


def test_split_shapes_split_on_this_device():
    """the planner of the library on this device gives every GEMM case the tier the table recorded on the host (the split ones: two launches)"""
    ops = _ops()
    for c in sc.CASES:
        if c.plan:
            M, N, K, epi, ln_part, label = c.plan
            p = ops.gemm_plan(M, N, K, epi, ln_part=ln_part)
            assert p["label"].startswith(label), (c.name, p["text"])
            assert (p["row0"] > 0) == (label == "split_"), (c.name, p["text"])


# ---- the runs -----------------------------------------------------------------------------------------------------------------------------
def _dev(host):
    return {k: v.cuda() for k, v in host.items()}


def _late_names(case, x):
    return case.late if case.late is not None else tuple(x)


def _run_late(case, h, A, B):
    """the call on the side stream behind the delay, the late inputs copied in behind the delay too -> (outputs, the delay was still
    running when the call returned)"""
    late = _late_names(case, A)
    X = {k: (B[k].clone() if k in late else A[k]) for k in A}
    torch.cuda.synchronize()
    with torch.cuda.stream(h.side):
        h.delay()
        for k in late:
            X[k].copy_(A[k], non_blocking=True)
        got = case.call(X)
        still_delayed = not h.side.query()
    h.side.synchronize()
    torch.cuda.synchronize()
    return got, still_delayed


_GROUND = {}


def _ground(case):
    """(A, B, want = call(A), other = call(B)) on the default stream, once per case"""
    if case.name not in _GROUND:
        A, B = _dev(case.build("A")), _dev(case.build("B"))
        want = case.call(A)
        other = case.call(B)
        torch.cuda.synchronize()
        assert not sc.same_bits(want, other), f"{case.name}: input sets A and B give the same bits — the case could not fail"
        _GROUND[case.name] = (A, B, want, other)
    return _GROUND[case.name]


# ---- 1. late inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_late_inputs(case, harness):
    A, B, want, _ = _ground(case)
    got, still_delayed = _run_late(case, harness, A, B)
    if not case.waits:
        assert still_delayed, f"{case.name}: the call blocked the host (it is not documented to wait), or its enqueue outlasted the delay"
    assert sc.same_bits(got, want), (f"{case.name}: the call on a side stream does not give the single-stream bits — a launch, memset or copy of "
                                     f"{', '.join(case.entries)} did not go to the stream it was given")


# ---- mutant control ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.MUTANTS)
def test_mutant_on_the_default_stream_is_caught(name, harness, monkeypatch):
    """the bug the method is for, made on purpose: the wrapper hands the entry the default stream while torch's current stream is `side`.
    Value-only entries: the kernel reads caller buffers that hold the valid set B."""
    from freepose_amd import _lib
    ops = _ops()
    case = sc.by_name(name)
    A, B, want, _ = _ground(case)
    handle = torch.cuda.default_stream().cuda_stream
    wrong = lambda: C.c_void_p(handle)          # noqa: E731
    monkeypatch.setattr(_lib, "current_stream", wrong)
    monkeypatch.setattr(ops, "current_stream", wrong)
    got, _ = _run_late(case, harness, A, B)
    assert not sc.same_bits(got, want), f"{name}: launched on the default stream and still the single-stream bits — part 1 would not see it"


# ---- 2. hand-over between streams --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fresh_context(monkeypatch):
    """a context of its own in place of the process's: no workspace, no FFA counters, and (through it) no object built yet"""
    from freepose_amd import _lib
    ops = _ops()
    lib = _lib.load()
    dev = torch.cuda.current_device()
    ops.context(dev)
    ctx = C.c_void_p()
    _lib.check(lib.fp_ctx_create(dev, C.byref(ctx)), "fp_ctx_create")
    own = ops._ctx[dev]
    monkeypatch.setitem(ops._ctx, dev, ctx)
    ctx.own = own                                   # the process's context: the single-stream results come from it and its objects
    yield ctx
    ops._ctx[dev] = own
    sc.drop_objects(ctx.value)
    gc.collect()
    torch.cuda.synchronize()
    lib.fp_ctx_destroy(ctx)


@pytest.mark.parametrize("name", sc.HANDOVER)
def test_hand_over(name, harness, fresh_context):
    from freepose_amd import _lib
    ops = _ops()
    case = sc.by_name(name)
    n0, n1, n2 = case.batches
    default = torch.cuda.default_stream()
    A0, A1, B1, A2 = (_dev(case.build(w, n)) for w, n in (("A", n0), ("A", n1), ("B", n1), ("A", n2)))
    # the single-stream results, under the process's own context and its own objects
    dev = torch.cuda.current_device()
    ops._ctx[dev] = fresh_context.own
    want0, want1, other1, want2 = case.call(A0), case.call(A1), case.call(B1), case.call(A2)
    torch.cuda.synchronize()
    ops._ctx[dev] = fresh_context
    assert not sc.same_bits(want1, other1)
    assert ops.context().value == fresh_context.value and _lib.load().fp_ctx_workspace_bytes(fresh_context) == 0
    got0 = case.call(A0)                            # builds the state on the default stream
    got1, _ = _run_late_ordered(case, harness, A1, B1)
    default.wait_stream(harness.side)
    got2 = case.call(A2)
    torch.cuda.synchronize()
    assert sc.same_bits(got0, want0), f"{name}: first call"
    assert sc.same_bits(got1, want1), f"{name}: the call on the side stream behind the hand-over (batch {n1})"
    assert sc.same_bits(got2, want2), f"{name}: back on the default stream"


def _run_late_ordered(case, h, A, B):
    """_run_late without its device-wide synchronisations in front: the hand-over is ordered by wait_stream alone"""
    late = _late_names(case, A)
    X = {k: (B[k].clone() if k in late else A[k]) for k in A}
    h.side.wait_stream(torch.cuda.default_stream())
    with torch.cuda.stream(h.side):
        h.delay()
        for k in late:
            X[k].copy_(A[k], non_blocking=True)
        got = case.call(X)
    return got, None


# ---- 3. no device-wide wait in steady state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_steady_state_call_does_not_drain_the_device(case, harness):
    from freepose_amd import _lib
    ops = _ops()
    lib = _lib.load()
    A = _ground(case)[0]
    case.call(A)
    case.call(A)
    torch.cuda.synchronize()
    before = lib.fp_ctx_workspace_bytes(ops.context())
    with torch.cuda.stream(harness.busy):
        harness.delay()
    out = case.call(A)
    torch.cuda.current_stream().synchronize()
    still_busy = not harness.busy.query()
    after = lib.fp_ctx_workspace_bytes(ops.context())
    harness.busy.synchronize()
    torch.cuda.synchronize()
    assert out is not None
    if case.name not in sc.DRAINS_DEVICE:
        assert still_busy, f"{case.name}: the call (or the wait on its own stream) waited for an unrelated stream — a device-wide wait or a hipFree"
    assert after == before, f"{case.name}: the workspaces changed in steady state ({before} -> {after} bytes)"


# ---- the event timer ---------------------------------------------------------------------------------------------------------------------------
def test_timer_events_are_recorded_on_the_given_stream(harness):
    """delay, start, delay, stop on the side stream: one delay between the events.  A start on another stream would measure two, a stop on
    another stream none."""
    from freepose_amd import _lib
    lib, t = _lib.load(), sc.timer()
    torch.cuda.synchronize()
    with torch.cuda.stream(harness.side):
        harness.delay()
        _lib.check(lib.fp_timer_start(t, _lib.current_stream()), "fp_timer_start")
        harness.delay()
        _lib.check(lib.fp_timer_stop(t, _lib.current_stream()), "fp_timer_stop")
        assert not harness.side.query()
    ms = C.c_float()
    _lib.check(lib.fp_timer_elapsed_ms(t, C.byref(ms)), "fp_timer_elapsed_ms")
    harness.side.synchronize()
    assert 0.8 * harness.delay_ms <= ms.value <= 1.5 * harness.delay_ms, (ms.value, harness.delay_ms)
