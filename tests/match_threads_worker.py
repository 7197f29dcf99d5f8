"""Worker of tests/test_match_threads_gpu.py (run as ONE child process: at most three worker threads beside the main thread).

The matchers as the reference's three threads call them, concurrently, each result compared byte for byte with the CPU oracle:

  tracking       (src/Tracking.cc:1336)                a tracking_chain.Chain on the latency path at 752x480 / 1000 features /
                                                       12 frames: orbx_stereo_frame_view, orbm_search_by_projection_frame_device,
                                                       orbm_search_local_points_device.  One iteration = 4 frames; a new Chain
                                                       every 3 iterations; the log must equal the OracleBackend's.
  local_mapping  (src/LocalMapping.cc:223,276,497)     orbm_search_for_triangulation at the crowded nodes, orbm_best_in_windows and
                                                       orbm_match_windows (the device part of Fuse) on 640x480 / 1000 features /
                                                       1500 queries.
  loop_closing   (src/LoopClosing.cc:249,333,608)      orbm_search_by_bow (both variants), orbv_transform on the shared vocabulary,
                                                       SearchByProjection(F, MPs) with 1500 map points, SearchForInitialization on
                                                       the fast path and with 513 candidates in one window (exact kernel).

Wave 1: three threads behind a Barrier, `--iters1` iterations each; a thread that is through goes on iterating (checked like
the others) until all three are, so every counted iteration runs beside two busy threads.  On iteration 10 (wave 2: 5) each thread runs
one larger call that outgrows ITS scratch (tests/match_cases.py names the sizes) and asserts through orbm_debug_thread_scratch
that the capacity grew.  At the end each thread releases its scratch (orbx_thread_release_scratch, twice), sees it gone, runs one
more iteration - the scratch is re-created with the arena's call counter already above zero - and releases again.  Wave 2: three
NEW threads, `--iters2` iterations, the roles rotated by one thread.  Every case's expected results are computed by the oracle,
single-threaded, before the first GPU call.  Prints one JSON line.

--alloc-fill WORD switches the developer build's scratch fill on (orbx_debug_set_alloc_fill) before the first GPU call: every arena,
mirror, staging pair, plan buffer and frame record of both waves starts out holding WORD instead of whatever the allocator returned.

--options role=fast_wave,role=exact sets orbm_set_thread_option(3, 1) / (2, 1) in the threads of that role; every thread records
what orbm_debug_match_path reports after each guided search it made."""
import argparse
import bisect
import importlib
import json
import os
import sys
import threading
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402

PKG = "orb_slam2v2-1_amd"
ROLES = ("tracking", "local_mapping", "loop_closing")
USES = {"tracking": ("arena",), "local_mapping": ("arena", "bow"), "loop_closing": ("arena", "bow", "stage")}   # scratch a role's iteration touches
REGROWS = {"tracking": "arena_cap", "local_mapping": "bow_cap", "loop_closing": "stage_cap"}                  # ... and the one its larger call outgrows
W, H, NF, FRAMES, FRAMES_PER_ITER = 752, 480, 1000, 12, 4


def uses(role, option):
    """The scratch a role's iteration touches: with the exact kernels asked for, a guided search never enters the fast path, so
    loop_closing - all of whose arena users are guided searches - leaves the arena alone."""
    return tuple(u for u in USES[role] if not (u == "arena" and option == "exact" and role == "loop_closing"))
OPTIONS = {"fast_wave": (3, 1), "exact": (2, 1)}


# ---- comparison and report code (importable without a GPU: tests/test_thread_scratch_cpu.py feeds it wrong results) ----------
def first_index(got, want):
    """Index of the first differing element of two results (flattened), -1 when they differ in shape or type."""
    a, b = np.asarray(got), np.asarray(want)
    if a.ndim == 0 and b.ndim == 0:                  # a count: an int on one side, a numpy integer on the other
        return None if a == b else 0
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1
    if a.dtype.kind == "f":
        ne = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    else:
        ne = a != b
    idx = np.flatnonzero(ne)
    return int(idx[0]) if len(idx) else None


def check_results(thread, iteration, call, got, want, bad):
    """Every field of `want` against `got`, exactly; appends {thread, iteration, call, field, first_index} per difference."""
    for field in sorted(set(want) | set(got)):
        if field not in got or field not in want:
            bad.append({"thread": thread, "iteration": iteration, "call": call, "field": field, "first_index": -1})
            continue
        i = first_index(got[field], want[field])
        if i is not None:
            bad.append({"thread": thread, "iteration": iteration, "call": call, "field": field, "first_index": i})


def chain_detail(want_snap, got_snap, field):
    """What differed in one field of a chain snapshot.  A number: the values got and wanted.  An array (the log keeps its bytes): both lengths
    in bytes and the first eight differing indices, counted in 32-bit words - every array of the log is made of 4-byte fields but the
    descriptors, whose index / 8 is the row - with the words got and wanted there (hex)."""
    got, want = (got_snap or {}).get(field), (want_snap or {}).get(field)
    if not isinstance(got, (bytes, bytearray)) or not isinstance(want, (bytes, bytearray)):
        plain = lambda v: v if isinstance(v, (int, float, str, type(None))) else repr(v)[:80]
        return {"got": plain(got), "want": plain(want)}
    n = min(len(got), len(want)) // 4
    a, b = np.frombuffer(got, np.uint32, n), np.frombuffer(want, np.uint32, n)
    idx = np.flatnonzero(a != b)[:8]
    return {"got_bytes": len(got), "want_bytes": len(want), "indices": [int(i) for i in idx], "got": ["%08x" % a[i] for i in idx],
            "want": ["%08x" % b[i] for i in idx]}


def check_chain(thread, iteration, diff, bad, want_log=None, got_log=None):
    """diff: tracking_chain.first_difference(oracle log, this log); with both logs, the entry also says what differed (chain_detail)."""
    if diff is not None:
        entry = {"thread": thread, "iteration": iteration, "call": "chain", "field": diff[1], "first_index": int(diff[0])}
        if want_log is not None and got_log is not None:
            t = int(diff[0])
            if diff[1] == "length":
                entry.update(got=len(got_log), want=len(want_log))
            elif t < len(want_log) and t < len(got_log):
                entry.update(chain_detail(want_log[t], got_log[t], diff[1]))
        bad.append(entry)


def scratch_is_released(s):
    return (s["arena_cap"], s["stage_cap"], s["bow_cap"]) == (0, 0, 0) and (s["arena_device"], s["stage_device"], s["bow_device"]) == (-1, -1, -1) \
        and s["arena_stream"] == 0 and s["arena_word"] == 0


def check_scratch(thread, iteration, what, ok, bad):
    if not ok:
        bad.append({"thread": thread, "iteration": iteration, "call": what, "field": "scratch", "first_index": -1})


def in_flight_during(first, second):
    """first, second: the (start, end) of each thread's library calls, in order.  True when some call of `first` was in flight at
    the moment a call of `second` started."""
    starts = [a for a, _ in first]
    for b0, _ in second:
        i = bisect.bisect_right(starts, b0) - 1
        if i >= 0 and first[i][1] > b0:
            return True
    return False


def overlap_matrix(intervals):
    """{thread: [(start, end), ...]} -> {"i>j": bool} for each ordered pair of threads."""
    names = sorted(intervals)
    return {"%s>%s" % (i, j): in_flight_during(intervals[i], intervals[j]) for i in names for j in names if i != j}


# ---- the threads --------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Times a thread's library calls and keeps the path record of its guided searches."""

    def __init__(self, pkg):
        self.pkg, self.intervals, self.paths, self.calls = pkg, [], {}, 0

    def call(self, name, guided, fn, *args):
        t0 = time.perf_counter()
        out = fn(*args)
        self.intervals.append((t0, time.perf_counter()))
        if name != "frame":
            self.calls += 1
        if guided:
            self.paths.setdefault(name, set()).add(self.pkg.debug_match_path()[:2])
        return out


def timed_view_backend(tc, rec):
    class TimedView(tc.GpuViewBackend):
        def frame(self, *a):
            return rec.call("frame", False, super().frame, *a)

        def search_frame(self, *a):
            return rec.call("search_by_projection_frame_device", True, super().search_frame, *a)

        def search_local(self, *a):
            return rec.call("search_local_points_device", True, super().search_local, *a)
    return TimedView(W, H, NF)


class Wave:
    def __init__(self, nthreads):
        self.barrier, self.lock, self.through, self.abort, self.n = threading.Barrier(nthreads), threading.Lock(), 0, threading.Event(), nthreads

    def finished_counted_iterations(self):
        with self.lock:
            self.through += 1

    def all_through(self):
        with self.lock:
            return self.through >= self.n


def role_thread(ctx, wave, name, role, iters, regrow_at, option, out):
    pkg, tc, L = ctx["pkg"], ctx["tc"], ctx["pkg"].matcher_lib()
    bad, scratch, rec = [], {}, Recorder(ctx["pkg"])
    out.update(role=role, option=option, bad=bad, scratch=scratch, error=None)
    counted = False
    try:
        scratch["start"] = pkg.debug_thread_scratch()                       # a thread that never called a matcher
        check_scratch(name, -1, "start", scratch_is_released(scratch["start"]) and scratch["start"]["arena_seq"] == 0, bad)
        if option:
            assert L.orbm_set_thread_option(*OPTIONS[option]) == 0
        state = {"chain": None, "backend": timed_view_backend(tc, rec) if role == "tracking" else None}

        def iteration(it):
            if role == "tracking":
                c = state["chain"]
                if c is None or c.t >= FRAMES:
                    c = state["chain"] = tc.Chain(state["backend"], W, H, NF)
                for _ in range(FRAMES_PER_ITER):
                    c.step(ctx["frames"][c.t][0], ctx["frames"][c.t][1], ctx["poses"][c.t])
                want = ctx["oracle_log"][:len(c.log)]
                check_chain(name, it, tc.first_difference(want, c.log), bad, want, c.log)
            else:
                for case in ctx["cases"][role]:
                    check_results(name, it, case.name, rec.call(case.name, case.guided, case.run, pkg, ctx["shared"]), case.want, bad)

        def regrow(it):
            big, field = ctx["big"][role], REGROWS[role]
            before = pkg.debug_thread_scratch()
            check_results(name, it, big.name, rec.call(big.name, big.guided, big.run, pkg, ctx["shared"]), big.want, bad)
            after = pkg.debug_thread_scratch()
            scratch["before_regrow"], scratch["after_regrow"] = before, after
            out["regrow"] = {"call": big.name, "field": field, "need": int(big.need), "expected_before": int(big.before), "before": before[field], "after": after[field]}
            check_scratch(name, it, big.name, before[field] < big.need <= after[field], bad)

        wave.barrier.wait(timeout=120)
        t_start = time.perf_counter()
        it = 0
        while not wave.abort.is_set() and (it < iters or (not wave.all_through() and it < 30 * iters)):
            if it == iters:
                out["calls"], counted = rec.calls, True
                wave.finished_counted_iterations()
                if wave.all_through():
                    break
            iteration(it)
            if it == regrow_at:
                regrow(it)
            it += 1
        if not counted:
            out["calls"], counted = rec.calls, True
            wave.finished_counted_iterations()
        out["iterations"] = it
        # the release: everything gone, a second release is a no-op, the next use re-creates the scratch, released again
        scratch["before_release"] = pkg.debug_thread_scratch()
        for key in ("after_release", "after_release_again"):
            check_scratch(name, it, key, L.orbx_thread_release_scratch() == 0, bad)
            scratch[key] = pkg.debug_thread_scratch()
            check_scratch(name, it, key, scratch_is_released(scratch[key]), bad)
        if not wave.abort.is_set():
            iteration(it)
        s = scratch["after_reuse"] = pkg.debug_thread_scratch()
        arena = int("arena" in uses(role, option))
        ok = all(s[u + "_cap"] > 0 and s[u + "_device"] == 0 for u in uses(role, option)) and s["arena_stream"] == arena and s["arena_word"] == arena \
            and s["arena_seq"] >= scratch["before_release"]["arena_seq"]
        check_scratch(name, it, "after_reuse", ok, bad)
        check_scratch(name, it, "final", L.orbx_thread_release_scratch() == 0, bad)
        scratch["final"] = pkg.debug_thread_scratch()
        check_scratch(name, it, "final", scratch_is_released(scratch["final"]), bad)
        out["wall_s"], out["all_calls"] = time.perf_counter() - t_start, rec.calls
    except BaseException:   # (reported, and the other threads stop starting GPU work)
        out["error"] = traceback.format_exc()
        wave.abort.set()
        try:
            wave.barrier.abort()
        except Exception:
            pass
    finally:
        if not counted:
            out.setdefault("calls", rec.calls)
            wave.finished_counted_iterations()
        if option:
            L.orbm_set_thread_option(OPTIONS[option][0], 0)
        out["paths"] = {k: sorted(list(p) for p in v) for k, v in rec.paths.items()}
        out["_intervals"] = rec.intervals


def run_wave(ctx, roles, iters, regrow_at, options):
    wave = Wave(len(roles))
    outs = {str(i): {} for i in range(len(roles))}
    threads = [threading.Thread(target=role_thread, args=(ctx, wave, str(i), role, iters, regrow_at, options.get(role), outs[str(i)]))
               for i, role in enumerate(roles)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    wall = time.perf_counter() - t0
    overlap = overlap_matrix({k: v.pop("_intervals", []) for k, v in outs.items()})
    for v in outs.values():
        v["bad"] = v.get("bad", [])[:20]
    return {"threads": outs, "overlap": overlap, "wall_s": wall, "iters": iters, "regrow_at": regrow_at}


def _kept(cache, name, make):
    """make(), or what an earlier run of this worker left under `cache` (a directory of the test session; None: no cache): the two
    slow oracle stages - the 1920x1080 extraction and the 12-frame chain - are the same for every run."""
    import pickle
    path = os.path.join(cache, name + ".pickle") if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    value = make()
    if path:
        with open(path + ".tmp", "wb") as f:
            pickle.dump(value, f)
        os.replace(path + ".tmp", path)
    return value


def build_context(pkg, oracle, synth, cache=None):
    """a. the cases and their expected results: the oracle, single-threaded, no GPU call."""
    import match_cases as mc
    import tracking_chain as tc
    frame = _kept(cache, "limits_frame", lambda: mc.limits_frame(oracle, synth))
    lm_cases, lm_big = mc.local_mapping_cases(pkg, oracle, synth)
    lc_cases, lc_big = mc.loop_closing_cases(pkg, oracle, synth, frame)
    step = 0.04
    frames, _ = synth.stereo_sequence(W, H, FRAMES, k=11, step=step)
    poses = tc.poses(FRAMES, step)

    def oracle_log():
        ref = tc.Chain(tc.OracleBackend(W, H, NF), W, H, NF)
        for t in range(FRAMES):
            ref.step(frames[t][0], frames[t][1], poses[t])
        return ref.log
    log = _kept(cache, "oracle_chain_log", oracle_log)
    assert len(log) == FRAMES and min(s["proj_n"] for s in log[1:]) >= 20 and sum(s["local_n"] for s in log[1:]) > 50
    ctx = {"pkg": pkg, "tc": tc, "frames": frames, "poses": poses, "oracle_log": log, "shared": {},
           "cases": {"local_mapping": lm_cases, "loop_closing": lc_cases},
           "big": {"tracking": mc.big_local_points_case(pkg, oracle, synth), "local_mapping": lm_big, "loop_closing": lc_big}}
    return ctx, mc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters1", type=int, default=30)
    ap.add_argument("--iters2", type=int, default=10)
    ap.add_argument("--options", default="")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--alloc-fill", type=int, default=None, metavar="WORD")
    a = ap.parse_args()
    options = dict(x.split("=") for x in a.options.split(",") if x)
    # every call of this process - the bag-of-words entry points too - goes to the developer build, where the hook lives
    os.environ["ORBX_LIB"] = os.path.join(ROOT, PKG, "lib", "liborbx_hip_dev.so")
    t0 = time.perf_counter()
    import oracle
    oracle.build()
    pkg = importlib.import_module(PKG)
    pkg.default_developer = True
    synth = importlib.import_module(PKG + ".synth")
    ctx, mc = build_context(pkg, oracle, synth, a.cache)
    t_cases = time.perf_counter() - t0
    # b. both libraries and the shared read-only handles, in the main thread
    L, ML = pkg.lib(), pkg.matcher_lib()
    assert L._orbx_developer and ML._orbx_developer
    if a.alloc_fill is not None:   # before the first GPU call: every scratch block of this process is born filled with the word
        pkg.debug_set_alloc_fill(1, a.alloc_fill)
    voc = mc.vocabulary()
    ctx["shared"]["voc"] = pkg.Vocabulary(10, 3, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    report = {"options": options, "cases_s": t_cases, "waves": []}
    # c, d. wave 1; e. wave 2: new threads, the roles rotated by one
    report["waves"].append(run_wave(ctx, ROLES, a.iters1, min(10, a.iters1 // 2), options))
    if not any(t.get("error") for t in report["waves"][0]["threads"].values()):
        report["waves"].append(run_wave(ctx, ROLES[-1:] + ROLES[:-1], a.iters2, min(10, a.iters2 // 2), options))
    report["main_thread_scratch"] = pkg.debug_thread_scratch()
    report["alloc_fill"] = None if a.alloc_fill is None else {"word": a.alloc_fill, "stats": list(pkg.debug_alloc_fill_stats())}
    report["total_s"] = time.perf_counter() - t0
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
