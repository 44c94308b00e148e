"""When a call reads and writes, observed from outside: the harness of
tests/test_gpu_stream_order.py.  Not a test module; the suite imports torch
before it imports this one.

include/rsgpu.h promises of every device entry point that its work is enqueued
on the context's stream and that nothing synchronises unless the function says
so, and of rsgpu_set_stream that work on the old stream is ordered before what
the context enqueues afterwards.  On the legacy null stream, where every other
GPU suite runs, neither sentence can be observed: everything in the process is
serialised there.  Here a call is made behind a GATE.

The gate is a bounded device-side delay (torch.cuda._sleep, its cycle count
calibrated once per module against HIP events, never a kernel that waits for
the host) on a side stream s, with an event g recorded behind it.  One gated
call (gated() below):

  1. every buffer of the call lies in ONE arena (tests/footprint.py) and the
     whole arena holds the DECOY state: well-formed inputs of another seed,
     valid lists that name other rows, noise in outputs, reports and statuses.
     Pointer tables of the decoy state name rows of a second, separate arena
     that holds the decoy state as well, so a kernel that runs too early
     computes a wrong answer and never follows a wild pointer;
  2. on s: the gate, the event g, one device-to-device copy that puts the TRUE
     state over the whole arena;
  3. the context moves to s, the call under test is made, and `closed = not
     g.query()` is read the moment it returns;
  4. while the gate is still closed, on s: the arena is copied into a result
     tensor and then overwritten with the decoy state again (a superset of
     "every input the call only reads"); on the host every array that was
     passed in (coef, gftbls, encode_matrix) is overwritten in place;
  5. s is waited for and the result is compared with the expectation: the
     arena after the same call on the same true state made the ordinary way,
     synchronised, on the same context with the same kernel choices.

Whatever escapes the stream -- a kernel or a status fill on stream 0, an
auxiliary stream that does not wait for the caller's or is not joined back, a
host argument read after the return -- meets decoys and shows as a difference.
Nothing is repeated to catch a race.  The region named `workspace` is scratch
whose contents no contract fixes; it is left out of the comparison.

A case's inputs come in variants: 0 the true state of the warm run, 1 the
decoy, 2 and above the true states of cold runs (another matrix of the same
size, other lists, other data).

Measured on an MI355X, one run of tests/test_gpu_stream_order.py:
torch.cuda._sleep delays (no copy-based gate was needed) at 2.36e6 cycles per
ms (4e6 cycles took 1.69 ms), so the 50 ms gate is 118e6 cycles and lasted
49.5 ms by events; the longest host time of a warm call was 0.05 ms, three
orders of magnitude inside the gate, and no gate was lengthened."""
import time

import numpy as np
import torch

import footprint as fp
import gpu_family as gf

GATE_MS = 50.0   # where a gate starts
GATE_CAP_MS = 200.0  # and what no gate may exceed
PROBE_CYCLES = 4_000_000


def host_rows(a, r):
    """[blocks, per, len] view of row buffer r in a host copy of the arena."""
    return np.lib.stride_tricks.as_strided(a[r.start:], (r.blocks, r.per, r.length), (r.per * r.pitch, r.pitch, 1))


class Gate:
    """The calibrated delay.  cycles_per_ms comes from timing one short sleep
    with events; no clock rate is assumed."""

    def __init__(self):
        torch.cuda._sleep(PROBE_CYCLES)  # the first launch pays for loading the kernel
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(PROBE_CYCLES)
        b.record()
        torch.cuda.synchronize()
        self.probe_ms = a.elapsed_time(b)
        assert self.probe_ms > 0.05, f"torch.cuda._sleep({PROBE_CYCLES}) took {self.probe_ms} ms: it does not delay"
        self.cycles_per_ms = PROBE_CYCLES / self.probe_ms
        self.longest_warm_ms = 0.0
        self.opened_cold = []  # ids of the cold calls that returned with the gate open

    def cycles(self, ms):
        assert 0 < ms <= GATE_CAP_MS
        return int(self.cycles_per_ms * ms)

    def close(self, s, ms=GATE_MS):
        """Enqueues the gate on s; the event behind it."""
        g = torch.cuda.Event()
        with torch.cuda.stream(s):
            torch.cuda._sleep(self.cycles(ms))
            g.record(s)
        return g

    def measure(self, s, ms=GATE_MS):
        """The length in ms of one gate on s, by events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            a.record(s)
            torch.cuda._sleep(self.cycles(ms))
            b.record(s)
        s.synchronize()
        return a.elapsed_time(b)


def independent(gate, sa, sb, ms=20.0):
    """Whether a fill on sb completes while a gate on sa is pending: the two
    streams do not share a hardware queue."""
    t = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = gate.close(sa, ms)
    with torch.cuda.stream(sb):
        t.fill_(1)
    sb.synchronize()
    pending = not g.query()
    sa.synchronize()
    return pending


class HostArg:
    """A host array a call is handed (coef, gftbls, encode_matrix): `live` is
    the memory that goes down, contiguous bytes, so the wrapper passes it and
    no copy; true and decoy are what it holds before and after the call."""

    def __init__(self, true, decoy):
        self.true = np.ascontiguousarray(true, np.uint8).copy()
        self.decoy = np.ascontiguousarray(decoy, np.uint8).copy()
        assert self.true.shape == self.decoy.shape and (self.true != self.decoy).any()
        self.live = self.true.copy()

    def restore(self):
        self.live[...] = self.true

    def clobber(self):
        self.live[...] = self.decoy


class Case:
    """What gated() and ordinary() need of a case: an fp.Arena `ar` that is
    allocated (ar.t, the working arena all pointers of call() go into), the
    device tensors `true` and `decoy` of the arena's size, the host arguments
    `host` ({name: HostArg}), call(ctx), verify(before, after) on host copies
    of the arena (the model's or the oracle's check of an ordinary run), and
    `scratch`, the regions left out of the comparison."""

    scratch = ("workspace",)
    host = {}

    def mask(self):
        m = np.ones(self.ar.size, bool)
        for name in self.scratch:
            if name in self.ar.by_name:
                r = self.ar[name]
                m[r.start: r.end] = False
        return m

    def differs(self, got, want):
        """The number of compared arena bytes in which two host copies differ,
        and the name of the first."""
        d = (got != want) & self.mask()
        return int(d.sum()), (self.ar.describe(int(np.argmax(d))) if d.any() else None)

    def same(self, got, want, what):
        n, where = self.differs(got, want)
        assert n == 0, f"{what}: {n} arena bytes differ from the ordinary run's, the first in {where}"


def ordinary(ctx, case):
    """The call on the true state the ordinary way, synchronised; the model's
    check of it.  Returns (arena after, record names): the expectation."""
    case.ar.t.copy_(case.true)
    for h in case.host.values():
        h.restore()
    torch.cuda.synchronize()
    before = case.ar.snapshot()
    names = gf.recorded(ctx, lambda: case.call(ctx))
    torch.cuda.synchronize()
    after = case.ar.snapshot()
    case.verify(before, after)
    return after, names


class Gated:
    """What one gated call left: the arena behind the call (host), whether the
    gate was closed when the call was entered, when it returned and when the
    trailing clobber was enqueued, and the host time of the call in ms."""

    def __init__(self, result, entry, closed, clobbered, ms):
        self.result, self.entry, self.closed, self.clobbered, self.ms = result, entry, closed, clobbered, ms


def gated(ctx, gate, case, s, move=True, ms=GATE_MS, before_clobber=None):
    """Steps 1 to 5 of the module docstring.  move=False leaves the context on
    the stream it is on (the negative controls: the call then meets decoys).
    before_clobber(): further calls behind the same gate, after the call under
    test and before the result is taken (the sequences)."""
    ar = case.ar
    result = torch.empty_like(ar.t)
    ar.t.copy_(case.decoy)
    for h in case.host.values():
        h.restore()
    torch.cuda.synchronize()
    prev = ctx.get_stream()
    try:
        g = gate.close(s, ms)
        with torch.cuda.stream(s):
            ar.t.copy_(case.true, non_blocking=True)
        if move:
            ctx.set_stream(s.cuda_stream)
        entry = not g.query()
        t0 = time.perf_counter()
        case.call(ctx)
        t1 = time.perf_counter()
        closed = not g.query()
        if before_clobber is not None:
            before_clobber()
        with torch.cuda.stream(s):
            result.copy_(ar.t, non_blocking=True)
            ar.t.copy_(case.decoy, non_blocking=True)
        for h in case.host.values():
            h.clobber()
        clobbered = not g.query()
        s.synchronize()
    finally:
        ctx.set_stream(prev)
        torch.cuda.synchronize()
        for h in case.host.values():
            h.restore()
    return Gated(result.cpu().numpy(), entry, closed, clobbered, (t1 - t0) * 1e3)


def warm(ctx, gate, case, s, names=None):
    """A warm case: the ordinary run (which also caches the program and grows
    the buffers), then the same call gated.  The result must be the ordinary
    run's, and the call must return with the gate still closed: the header's
    "nothing synchronises"."""
    want, got_names = ordinary(ctx, case)
    if names is not None:
        assert got_names == names, got_names
    r = gated(ctx, gate, case, s)
    assert r.entry, "the gate was open before the call was made"
    case.same(r.result, want, "behind the gate")
    assert r.closed, f"the call synchronised: it took {r.ms:.1f} ms and returned with the gate open"
    assert r.clobbered, "the gate opened before the trailing clobber was enqueued"
    gate.longest_warm_ms = max(gate.longest_warm_ms, r.ms)
    return r, got_names


def cold(ctx, gate, warm_case, case, s, ident, names=None):
    """A cold case: `case` has a matrix or lists the context has not seen, of
    warm_case's sizes, and warm_case has run, so that no buffer grows.  The
    gated call comes FIRST here and its expectation, the ordinary run of the
    same state, after it: made before, the ordinary run would be the first
    use.  The gate must be closed on entry and the result right; whether the
    call returned with the gate closed is recorded, not asserted (the header
    lets a first use synchronise)."""
    ordinary(ctx, warm_case)
    r = gated(ctx, gate, case, s)
    assert r.entry, "the gate was open before the call was made"
    want, got_names = ordinary(ctx, case)
    if names is not None:
        assert got_names == names, got_names
    case.same(r.result, want, "behind the gate, first use")
    if not r.closed:
        gate.opened_cold.append(ident)
    return r, got_names


def sequence(gate, steps, s, ms=GATE_MS):
    """Several calls behind ONE gate on s.  steps: [(ctx, case, stream)], in
    order; every case has its own arena.  All arenas hold decoys, the gate is
    enqueued on s and behind it the copies that put every case's true state
    in place; then each step moves its context to its stream (rsgpu_set_stream
    is what orders a step on another stream behind the gate) and makes its
    call, at once.  After the last call every arena is copied out and
    clobbered on the stream its call was made on.  Returns the arenas behind
    the calls (host), in step order, and for each call whether the gate was
    still closed when it returned."""
    results = [torch.empty_like(case.ar.t) for _, case, _ in steps]
    for _, case, _ in steps:
        case.ar.t.copy_(case.decoy)
        for h in case.host.values():
            h.restore()
    torch.cuda.synchronize()
    prev = [(ctx, ctx.get_stream()) for ctx, _, _ in steps]
    try:
        g = gate.close(s, ms)
        with torch.cuda.stream(s):
            for _, case, _ in steps:
                case.ar.t.copy_(case.true, non_blocking=True)
        closed = []
        for ctx, case, st in steps:
            ctx.set_stream(st.cuda_stream)
            case.call(ctx)
            closed.append(not g.query())
        for (_, case, st), result in zip(steps, results):
            with torch.cuda.stream(st):
                result.copy_(case.ar.t, non_blocking=True)
                case.ar.t.copy_(case.decoy, non_blocking=True)
            for h in case.host.values():
                h.clobber()
        for _, _, st in steps:
            st.synchronize()
    finally:
        for ctx, stream in prev:
            ctx.set_stream(stream)
        torch.cuda.synchronize()
        for _, case, _ in steps:
            for h in case.host.values():
                h.restore()
    return [r.cpu().numpy() for r in results], closed


# ---- arenas ------------------------------------------------------------------

def arena(layout, device):
    """layout(ar) declares the buffers; the arena allocated, its noise from a
    fixed seed (the states overwrite all of it)."""
    ar = fp.Arena()
    layout(ar)
    ar.allocate(device, seed=ar.size % 9973 + 1)
    return ar


def noise_state(ar, seed):
    """A device tensor of the arena's size, seeded noise."""
    return torch.from_numpy(ar.noise(seed)).to(ar.t.device)
