"""The matchers from three host threads at once, as the reference's Tracking, LocalMapping and LoopClosing threads call ORBmatcher
(src/Tracking.cc:1336, src/LocalMapping.cc:223,276,497, src/LoopClosing.cc:249,333,608), and the per-thread scratch contract of
INTEGRATION.md section 4: thread-local arena / staging pair / bag-of-words scratch, thread-local options and path records, the
mutex-guarded LDS budget cache, orbx_thread_release_scratch().

tests/match_threads_worker.py does the work in ONE fresh child process (three worker threads beside its main thread) and prints one
JSON report; this file asserts all of it.  Every result of every iteration of every thread equals the CPU oracle byte for byte
(tests/test_thread_scratch_cpu.py shows the comparison code reporting wrong results).  Which size triggers which regrow - the sizes
are the smallest past what each scratch holds by then, from the need formulas of csrc/ restated in tests/match_cases.py:

  tracking       arena, 4 MiB          orbm_search_local_points, ~1000 keypoints and 17 6xx world points:
                                       n * 108 + m * 228 + 64 KiB > 4 MiB
  local_mapping  BoW scratch, 1.4 MiB  orbm_search_for_triangulation, the crowded nodes + two 4096-candidate nodes + one of ~2600:
                                       69 B per query, 65 B per candidate, 4 B per list item > twice the crowded case's need
  loop_closing   staging pair, 1 MiB   SearchForInitialization 7329 x 7001 (n2 = 7001: the exact kernel): 76 * n1 + 70 * n2 > 1 MiB

Each regrow starts from a scratch the thread has been using (a scratch holds max(twice the largest need so far, its first capacity);
loop_closing's staging pair serves the 513-candidate initialization, which the fast path hands to the exact kernel), while the other
two threads keep calling; the new capacity is twice the larger call's need.

The child's time limit is a guard against a hang, not a performance bar.  After a time-out or a death by signal nothing more of this
file starts on the GPU."""
import json
import os
import subprocess
import sys

import pytest

import match_threads_worker as worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "match_threads_worker.py")
FATAL = (124, 134, 137, 139, -6, -11)
_gpu_gave_way = []       # set once by a run that timed out or died: every later test of this file skips
MIN = {"arena_cap": 4 << 20, "bow_cap": 1 << 20, "stage_cap": 1 << 20}
ROLES, REGROWS = worker.ROLES, worker.REGROWS


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("match_threads"))


def run_worker(cache, *args):
    if _gpu_gave_way:
        pytest.skip("an earlier worker run of this file timed out or died (%s): nothing more starts on the GPU" % _gpu_gave_way[0])
    cmd = [sys.executable, WORKER, "--cache", cache] + list(args)
    try:
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, text=True)
    except subprocess.TimeoutExpired as e:
        _gpu_gave_way.append("time-out")
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("the worker did not finish within 300 s\n" + err[-4000:])
    if p.returncode in FATAL:
        _gpu_gave_way.append("exit status %d" % p.returncode)
        pytest.fail("the worker died with status %d\n%s" % (p.returncode, p.stderr[-4000:]))
    assert p.returncode == 0, "worker failed (%d)\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def released(s):
    return (s["arena_cap"], s["stage_cap"], s["bow_cap"], s["arena_device"], s["stage_device"], s["bow_device"], s["arena_stream"],
            s["arena_word"]) == (0, 0, 0, -1, -1, -1, 0, 0)


def check_report(rep, iters):
    """What both runs must show: every thread of both waves without a difference, overlap, regrow, release, re-creation."""
    assert len(rep["waves"]) == 2, [t.get("error") for t in rep["waves"][0]["threads"].values()]
    assert released(rep["main_thread_scratch"]) and rep["main_thread_scratch"]["arena_seq"] == 0     # the main thread made no matcher call
    for w, (wave, n) in enumerate(zip(rep["waves"], iters)):
        print("wave %d: %.2f s, overlap %s" % (w + 1, wave["wall_s"], wave["overlap"]))
        roles = [wave["threads"][str(i)]["role"] for i in range(3)]
        assert roles == list(ROLES if w == 0 else ROLES[-1:] + ROLES[:-1])                          # wave 2: the roles rotated by one thread
        assert len(wave["overlap"]) == 6 and all(wave["overlap"].values()), wave["overlap"]
        for i in range(3):
            t = wave["threads"][str(i)]
            role, sc = t["role"], t["scratch"]
            what = "wave %d thread %d (%s)" % (w + 1, i, role)
            print("  %s: %d counted calls in %d iterations, %d calls in all, %.2f s; regrow %s" % (what, t.get("calls", -1), n, t.get("all_calls", -1),
                                                                                                 t.get("wall_s", -1), t.get("regrow")))
            assert t["error"] is None, "%s\n%s" % (what, t["error"])
            assert t["bad"] == [], "%s: %s" % (what, t["bad"])
            assert t["iterations"] >= n and t["calls"] >= n and t["all_calls"] > t["calls"]
            assert released(sc["start"]) and sc["start"]["arena_seq"] == 0, (what, sc["start"])
            g, field = t["regrow"], REGROWS[role]
            assert g["field"] == field and MIN[field] <= g["expected_before"] == g["before"] < g["need"] <= g["after"] == 2 * g["need"], (what, g)
            assert sc["before_regrow"][field] == g["before"] and sc["after_regrow"][field] == g["after"]
            used = worker.uses(role, t["option"])
            for u in ("arena", "stage", "bow"):
                for key in ("before_release", "after_reuse"):
                    if u in used:
                        assert sc[key][u + "_cap"] >= MIN[u + "_cap"] and sc[key][u + "_device"] == 0, (what, u, key, sc[key])
                    else:
                        assert sc[key][u + "_cap"] == 0 and sc[key][u + "_device"] == -1, (what, u, key, sc[key])
            assert sc["before_release"][field] == g["after"]                                        # grow-only until the release
            arena = int("arena" in used)
            assert sc["before_release"]["arena_stream"] == arena and sc["before_release"]["arena_word"] == arena
            for key in ("after_release", "after_release_again", "final"):
                assert released(sc[key]), (what, key, sc[key])
                assert sc[key]["arena_seq"] == sc["before_release" if key != "final" else "after_reuse"]["arena_seq"]   # the counter outlives the release
            assert sc["after_reuse"]["arena_stream"] == arena and sc["after_reuse"]["arena_word"] == arena
            assert sc["after_reuse"]["arena_seq"] >= sc["before_release"]["arena_seq"]
        by_role = {t["role"]: t for t in wave["threads"].values()}
        assert by_role["tracking"]["calls"] >= max(by_role["local_mapping"]["calls"], by_role["loop_closing"]["calls"])
    return {w: {t["role"]: t for t in wave["threads"].values()} for w, wave in enumerate(rep["waves"])}


def test_matchers_from_three_threads(pkg, cache):
    """Default options: 30 iterations per thread in wave 1, 10 in wave 2 (new threads, roles rotated).  On top of check_report: the
    threads whose fast path ends in k_resolve_par count their calls in the arena's completion word, so the iteration after the
    release runs with a fresh word and a counter far above it (the stale-word case), and goes on counting; loop_closing's
    513-candidate initialization really ran the exact kernel (the staging pair was in use before its regrow)."""
    rep = run_worker(cache, "--iters1", "30", "--iters2", "10")
    print("cases built in %.1f s, the run took %.1f s" % (rep["cases_s"], rep["total_s"]))
    waves = check_report(rep, (30, 10))
    for w, roles in waves.items():
        for role in ("tracking", "loop_closing"):
            sc = roles[role]["scratch"]
            assert sc["before_release"]["arena_seq"] >= (30, 10)[w], (w, role, sc["before_release"])
            assert sc["after_reuse"]["arena_seq"] > sc["before_release"]["arena_seq"], (w, role)
        paths = roles["loop_closing"]["paths"]
        assert paths["search_for_initialization_513"] == [[pkg.RES_EXACT, pkg.FB_CAND_CAP]], paths
        assert paths["search_for_initialization_big"] == [[pkg.RES_EXACT, pkg.FB_INIT_SIZE]], paths
        seen = [tuple(p) for r in ROLES for call, ps in roles[r]["paths"].items() for p in ps]
        assert all(_default_path(pkg, p) for p in seen), seen                     # nobody saw a neighbour's option
        tr = roles["tracking"]["paths"]
        assert any(p[0] in (pkg.RES_PAR_Q2, pkg.RES_PAR_Q4) for ps in tr.values() for p in ps), tr


def test_matchers_from_three_threads_on_filled_scratch(pkg, cache):
    """--alloc-fill 1: every scratch block of the child (arenas and their mirrors, staging pairs, BoW scratch, the extractors' plan buffers
    and frame records, the completion words before their initialisation) is born holding the word 1 - wave 1 then runs under wave 2's
    conditions (blocks that are no zero pages), on every run.  6 and 3 iterations; everything check_report asks, and the fill reached the
    threads' scratch: at least the three arenas + mirrors of each wave, more than 2 * 3 * 2 blocks of 4 MiB."""
    rep = run_worker(cache, "--alloc-fill", "1", "--iters1", "6", "--iters2", "3")
    print("cases built in %.1f s, the run took %.1f s; filled %s" % (rep["cases_s"], rep["total_s"], rep["alloc_fill"]))
    check_report(rep, (6, 3))
    assert rep["alloc_fill"]["word"] == 1
    blocks, nbytes = rep["alloc_fill"]["stats"]
    assert blocks >= 12 and nbytes >= 12 * MIN["arena_cap"], rep["alloc_fill"]


def _data_fallback(pkg, p):
    """The exact kernels for a reason of the call's data or size, not of an option."""
    return p[0] == pkg.RES_EXACT and p[1] in (pkg.FB_CAND_CAP, pkg.FB_QK, pkg.FB_INIT_SIZE, pkg.FB_N)


def _default_path(pkg, p):
    """What a thread without options may see: k_resolve_par, the single-wave resolvers where k_resolve_par does not apply
    (SearchForInitialization, more than 4096 queries), or a fall-back for a reason of the data."""
    return (p[0] in (pkg.RES_PAR_Q2, pkg.RES_PAR_Q4, pkg.RES_WAVE) and p[1] == pkg.FB_NONE) or _data_fallback(pkg, p)


def test_matchers_from_three_threads_each_with_its_resolver(pkg, cache):
    """The same with the tracking threads on the single-wave resolvers (orbm_set_thread_option(3, 1)), the loop-closing threads on the
    exact kernels ((2, 1)) and the local-mapping threads on the default: options and path records are per thread, and each thread saw,
    through orbm_debug_match_path after every guided search it made, the resolver it asked for and never a neighbour's."""
    rep = run_worker(cache, "--iters1", "30", "--iters2", "10", "--options", "tracking=fast_wave,loop_closing=exact")
    print("cases built in %.1f s, the run took %.1f s" % (rep["cases_s"], rep["total_s"]))
    waves = check_report(rep, (30, 10))
    for w, roles in waves.items():
        assert [roles[r]["option"] for r in ROLES] == ["fast_wave", None, "exact"]
        tr = roles["tracking"]["paths"]
        assert set(tr) == {"search_by_projection_frame_device", "search_local_points_device", "search_local_points_big"}, tr
        for call, seen in tr.items():                         # the single-wave resolver, or the exact kernels for a reason of the data: never k_resolve_par
            assert all((p[0] == pkg.RES_WAVE and p[1] == pkg.FB_NONE) or _data_fallback(pkg, p) for p in seen), (call, seen)
        assert any(p[0] == pkg.RES_WAVE for ps in tr.values() for p in ps), tr
        lc = roles["loop_closing"]["paths"]
        assert set(lc) == {"search_by_projection", "search_for_initialization", "search_for_initialization_513", "search_for_initialization_big"}, lc
        for call, seen in lc.items():
            assert seen == [[pkg.RES_EXACT, pkg.FB_OPTION]], (call, seen)
        lm = roles["local_mapping"]["paths"]
        assert set(lm) == {"match_windows"} and all(_default_path(pkg, p) and p[0] != pkg.RES_WAVE for p in lm["match_windows"]), lm
