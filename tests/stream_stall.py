"""Hold one stream back and look at what the others do: the helper of tests/test_stream_order_gpu.py.

A stall is one wave of the library's k_spin on a raw hipStream_t (orbx_debug_stall_stream, developer build only) with a torch event
recorded behind it.  While the event is pending, everything queued on that stream behind the stall has not run: a consumer on
another stream that lacks its wait reads what the buffers held before.  Three things make such a test mean something, and all three
are checked here rather than assumed:

  calibrate()        the stall really lasts (a nominal 30 ms and 50 ms stall measured with events, each at least half its nominal
                     length) - a stall that is too short lets every case pass while proving nothing;
  independent(x, y)  work on y does not queue behind work on x.  A process has a handful of hardware queues and the runtime deals
                     streams to them round-robin; two streams on one queue run in order, which hides a missing wait;
  Stall.pending()    the stall was still in front of the work when the host had finished issuing the call (Stall.since(): for a call
                     that returns results to the host, the time from the stall's launch to the call's return).

Streams are raw hipStream_t values (ints; 0 = the default stream), as the library's entry points take them."""
import time

import torch

STALL_MS = 30           # internal joins, the caller's stream
POLL_STALL_MS = 50      # the polls' windows (200000 pause instructions: a few ms) run out on any CPU
ATTEMPTS = 4            # arrangements a case may try to find an effective pair of streams

_pkg = None
_measured = {}          # nominal ms -> measured ms (calibrate, once per session)


def _torch_stream(raw):
    return torch.cuda.ExternalStream(raw) if raw else torch.cuda.default_stream()


class Stall:
    """A spin of `ms` on `stream` and the event behind it."""

    def __init__(self, stream, ms):
        assert _pkg is not None, "stream_stall.use(pkg) first"
        self.stream, self.ms = int(stream or 0), ms
        self.t0 = time.perf_counter()
        _pkg.debug_stall_stream(self.stream, int(ms * 1000))
        self.event = torch.cuda.Event()
        self.event.record(_torch_stream(self.stream))

    def pending(self):
        return not self.event.query()

    def wait(self):
        self.event.synchronize()

    def since(self):
        """Milliseconds on the host since the stall was about to be issued: at least its length once work queued behind it has been
        waited for."""
        return (time.perf_counter() - self.t0) * 1e3


def use(pkg):
    global _pkg
    _pkg = pkg


def stall(stream, ms):
    return Stall(stream, ms)


def calibrate():
    """Measured length of a nominal 30 ms and 50 ms stall -> {30: ms, 50: ms}; asserted to be at least half the nominal length."""
    if not _measured:
        s = torch.cuda.Stream()
        _pkg.debug_stall_stream(s.cuda_stream, 1)          # the kernel's first launch loads its code: not part of a stall's length
        s.synchronize()
        for ms in (STALL_MS, POLL_STALL_MS):
            got = []
            for _ in range(3):                             # the spin's length is the shortest bracket; the rest is what the events add
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                _pkg.debug_stall_stream(s.cuda_stream, ms * 1000)
                b.record(s)
                b.synchronize()
                got.append(a.elapsed_time(b))
            _measured[ms] = min(got)
            print("stream_stall.calibrate: nominal %d ms stall measured %s ms" % (ms, ", ".join("%.3f" % g for g in got)))
        for ms, got in _measured.items():
            assert got >= 0.5 * ms, "a nominal %d ms stall lasted %.2f ms: too short to show a missing wait" % (ms, got)
    return dict(_measured)


def independent(x, y):
    """True iff a kernel on y runs while x is held back, i.e. the two streams do not share a hardware queue."""
    x, y = int(x or 0), int(y or 0)
    if x == y:
        return False
    _torch_stream(x).synchronize()
    _torch_stream(y).synchronize()
    busy = Stall(x, 2)
    _pkg.debug_stall_stream(y, 1)             # as good as empty: one wave, one microsecond
    ev = torch.cuda.Event()
    ev.record(_torch_stream(y))
    ev.synchronize()
    ok = busy.pending()
    busy.wait()
    return ok


def effective(arrange, what):
    """arrange(attempt) -> (context, [(stalled stream, waiting stream, names), ...]).  The first of up to ATTEMPTS arrangements whose
    pairs are all independent; fails - never skips, never passes - when there is none, naming the streams."""
    tried = []
    for attempt in range(ATTEMPTS):
        ctx, pairs = arrange(attempt)
        bad = [names for x, y, names in pairs if not independent(x, y)]
        if not bad:
            print("%s: effective at arrangement %d" % (what, attempt))
            return ctx
        tried.append((ctx, bad))               # (kept alive: the next arrangement's streams are dealt other queues)
    raise AssertionError("%s: no arrangement of %d separates %s - the case cannot show a missing wait" %
                         (what, ATTEMPTS, sorted({"%s / %s" % n for _, bad in tried for n in bad})))


def fresh_caller_stream(keep=[]):
    """A new non-default torch stream for the caller's side (all of them stay alive: queues are dealt round-robin)."""
    s = torch.cuda.Stream()
    keep.append(s)
    return s
