"""CPU: the parts of the per-thread scratch contract that need no GPU.

orbx_thread_release_scratch() on a thread that holds nothing is ORBX_OK and a no-op (the three release functions guard on "nothing
allocated"), the developer build's orbm_debug_thread_scratch reports that record, and the comparison code of the threaded GPU test
(tests/match_threads_worker.py) names thread, iteration, call and field of a wrong result - so tests/test_match_threads_gpu.py cannot
pass vacuously."""
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc                 # noqa: E402
import match_threads_worker as worker    # noqa: E402
import tracking_chain as tc              # noqa: E402

NOTHING = {"arena_cap": 0, "arena_device": -1, "arena_stream": 0, "arena_word": 0, "stage_cap": 0, "stage_device": -1, "bow_cap": 0,
           "bow_device": -1}


def _without_counter(s):
    return {k: v for k, v in s.items() if k != "arena_seq"}


def test_release_scratch_with_nothing_allocated(pkg):
    """Main thread (released first: an earlier test of this process may have called a matcher from it) and a fresh thread that never
    called one: ORBX_OK, twice in a row, the hook reports "nothing allocated" before and after; the product library too."""
    D, P = pkg.lib(True), pkg.lib()
    seen = {}

    def body(name, fresh):
        if fresh:
            seen[name + ":before"] = pkg.debug_thread_scratch()
        rcs = []
        for _ in range(2):
            rcs.append(D.orbx_thread_release_scratch())
            seen["%s:after%d" % (name, len(rcs))] = pkg.debug_thread_scratch()
        rcs += [P.orbx_thread_release_scratch(), P.orbx_thread_release_scratch()]
        seen[name + ":rc"] = rcs

    body("main", False)
    t = threading.Thread(target=body, args=("fresh", True))
    t.start()
    t.join()
    assert seen["main:rc"] == [pkg.ORBX_OK] * 4 and seen["fresh:rc"] == [pkg.ORBX_OK] * 4
    for key in ("main:after1", "main:after2", "fresh:before", "fresh:after1", "fresh:after2"):
        assert _without_counter(seen[key]) == NOTHING, (key, seen[key])
        assert worker.scratch_is_released(seen[key])
    assert seen["fresh:before"]["arena_seq"] == 0
    assert list(seen["fresh:before"]) == pkg.THREAD_SCRATCH_FIELDS and len(pkg.THREAD_SCRATCH_FIELDS) == 9


def test_thread_scratch_hook_arguments(pkg):
    D = pkg.lib(True)
    out = np.full(10, 7, np.int64)
    assert D.orbm_debug_thread_scratch(None, 9) == pkg.ORBX_ERR_ARG
    assert D.orbm_debug_thread_scratch(out.ctypes.data, 8) == pkg.ORBX_ERR_ARG and D.orbm_debug_thread_scratch(out.ctypes.data, 10) == pkg.ORBX_ERR_ARG
    assert (out == 7).all() and b"orbm_debug_thread_scratch" in D.orbx_last_error()
    assert D.orbm_debug_thread_scratch(out.ctypes.data, 9) == pkg.ORBX_OK and out[9] == 7


def _results():
    rng = np.random.default_rng(3)
    a = {"nmatches": 412, "match_q": rng.integers(-1, 900, 789).astype(np.int32)}
    b = {"nmatches": 388, "match_q": rng.integers(-1, 900, 789).astype(np.int32)}
    c = {"nmatches": 5, "matches12": rng.integers(-1, 50, 400).astype(np.int32), "prev_matched": rng.random((400, 2)).astype(np.float32)}
    return a, b, c


def test_worker_comparison_names_thread_iteration_call_and_field():
    a, b, c = _results()
    bad = []
    for want in (a, b, c):
        worker.check_results("1", 4, "call", {k: (v.copy() if hasattr(v, "copy") else v) for k, v in want.items()}, want, bad)
    assert bad == []
    # one corrupted element of one result array
    got = dict(c, prev_matched=c["prev_matched"].copy())
    got["prev_matched"][123, 1] = np.nextafter(got["prev_matched"][123, 1], np.float32(2))
    worker.check_results("2", 17, "search_for_initialization", got, c, bad)
    assert bad == [{"thread": "2", "iteration": 17, "call": "search_for_initialization", "field": "prev_matched", "first_index": 247}]
    # a swapped pair: each call handed the other one's (well-formed) result
    bad = []
    worker.check_results("0", 9, "search_by_bow_kf_frame", b, a, bad)
    worker.check_results("0", 9, "search_by_bow_kf_kf", a, b, bad)
    assert [(x["thread"], x["iteration"], x["call"], x["field"]) for x in bad] == [
        ("0", 9, "search_by_bow_kf_frame", "match_q"), ("0", 9, "search_by_bow_kf_frame", "nmatches"),
        ("0", 9, "search_by_bow_kf_kf", "match_q"), ("0", 9, "search_by_bow_kf_kf", "nmatches")]
    assert bad[0]["first_index"] == int(np.flatnonzero(a["match_q"] != b["match_q"])[0]) and bad[1]["first_index"] == 0
    # the match count alone, a missing field, another length, another type
    bad = []
    worker.check_results("1", 0, "x", dict(a, nmatches=411), a, bad)
    worker.check_results("1", 1, "x", {"nmatches": 412}, a, bad)
    worker.check_results("1", 2, "x", dict(a, match_q=a["match_q"][:-1]), a, bad)
    worker.check_results("1", 3, "x", dict(a, match_q=a["match_q"].astype(np.int64)), a, bad)
    assert [(x["iteration"], x["field"], x["first_index"]) for x in bad] == [(0, "nmatches", 0), (1, "match_q", -1), (2, "match_q", -1), (3, "match_q", -1)]
    # the tracking chain's log: frame and field of the first difference
    bad = []
    worker.check_chain("2", 6, None, bad)
    worker.check_chain("2", 7, (5, "local"), bad)
    assert bad == [{"thread": "2", "iteration": 7, "call": "chain", "field": "local", "first_index": 5}]
    worker.check_scratch("2", 10, "search_local_points_big", False, bad)
    assert bad[-1] == {"thread": "2", "iteration": 10, "call": "search_local_points_big", "field": "scratch", "first_index": -1}


def test_worker_chain_report_says_what_differed():
    """A wrong tracking chain: besides frame and field, the report holds the values got and wanted of a count, and of an array the first
    eight differing 32-bit word indices with the words on both sides - one occurrence of a rare failure then says what differed."""
    rng = np.random.default_rng(5)
    proj = rng.integers(-1, 900, 40).astype(np.int32)
    want = [{"n": 300, "proj_n": 0, "proj": b""}, {"n": 301, "proj_n": 212, "proj": proj.tobytes()}]
    same = [dict(x) for x in want]
    bad = []
    worker.check_chain("0", 1, tc.first_difference(want, same), bad, want, same)
    assert bad == []
    # a count
    got = [dict(x) for x in want]
    got[1]["proj_n"] = 211
    worker.check_chain("0", 2, tc.first_difference(want, got), bad, want, got)
    assert bad == [{"thread": "0", "iteration": 2, "call": "chain", "field": "proj_n", "first_index": 1, "got": 211, "want": 212}]
    # an array: ten wrong elements, the first eight are named, in order, with both words
    wrong = proj.copy()
    where = [3, 5, 8, 13, 21, 22, 30, 31, 38, 39]
    wrong[where] += 1
    got = [dict(x) for x in want]
    got[1]["proj"] = wrong.tobytes()
    bad = []
    worker.check_chain("1", 3, tc.first_difference(want, got), bad, want, got)
    assert len(bad) == 1 and (bad[0]["field"], bad[0]["first_index"]) == ("proj", 1)
    assert bad[0]["indices"] == where[:8] and bad[0]["got_bytes"] == bad[0]["want_bytes"] == 160
    assert bad[0]["got"] == ["%08x" % (int(v) & 0xFFFFFFFF) for v in wrong[where[:8]]]
    assert bad[0]["want"] == ["%08x" % (int(v) & 0xFFFFFFFF) for v in proj[where[:8]]]
    # another length: both lengths, and the differing words of the common part
    got[1]["proj"] = wrong.tobytes()[:-8]
    bad = []
    worker.check_chain("1", 4, tc.first_difference(want, got), bad, want, got)
    assert (bad[0]["got_bytes"], bad[0]["want_bytes"], bad[0]["indices"]) == (152, 160, where[:8])
    # a shorter log
    bad = []
    worker.check_chain("2", 5, (1, "length"), bad, want, want[:1])
    assert bad == [{"thread": "2", "iteration": 5, "call": "chain", "field": "length", "first_index": 1, "got": 1, "want": 2}]
    import json
    json.dumps(bad)          # the report travels as JSON


def test_worker_overlap_matrix_is_ordered():
    """"i>j": a call of i was in flight when a call of j started."""
    iv = {"0": [(0.0, 1.0), (4.0, 5.0)], "1": [(0.5, 0.6), (2.0, 3.0)], "2": [(6.0, 7.0)]}
    assert worker.overlap_matrix(iv) == {"0>1": True, "1>0": False, "0>2": False, "2>0": False, "1>2": False, "2>1": False}
    iv["2"] = [(2.5, 4.5)]
    m = worker.overlap_matrix(iv)
    assert m["1>2"] and m["2>0"] and not m["2>1"] and not m["0>2"]
    assert not worker.scratch_is_released(dict(NOTHING, arena_seq=3, arena_word=1)) and worker.scratch_is_released(dict(NOTHING, arena_seq=3))


def test_regrow_sizes_are_the_smallest_past_each_first_capacity():
    """The sizes the worker's larger calls use, from the need formulas restated in tests/match_cases.py (csrc/orbx_match_fast.hip,
    orbx_match.hip, orbx_bow.hip): just past what the arena (4 MiB), the BoW scratch (twice the crowded case's need) and the
    staging pair (1 MiB) hold by then; the next smaller size is not."""
    sq, sc = mc.big_triangulation_sizes()
    need = lambda q, c: mc.bow_need_triangulation(sum(q), sum(c), len(q), sum(q), sum(c))
    s, g = mc.bs.tri_case()
    small = mc.bow_need_triangulation(len(s["qa"]), len(s["ca"]), 10, len(s["qit"]), len(s["cit"]))
    assert small == need(mc.bs.CROWD_Q, mc.bs.CROWD_C) and mc.triangulation_capacity() == 2 * small > mc.BOW_MIN
    assert need(sq, sc) > 2 * small >= need(sq, sc[:-1] + (sc[-1] - 8,)) and 8 <= sc[-1] <= 4096
    n1 = 7001
    while mc.stage_need_initialization(n1, 7001) <= mc.STAGE_MIN:
        n1 += 1
    assert 7001 < n1 < 7500 and mc.stage_need_initialization(7001, 7001) < mc.STAGE_MIN
    assert mc.arena_need_local_points(1000, 17634) <= mc.ARENA_MIN < mc.arena_need_local_points(1000, 17635)
