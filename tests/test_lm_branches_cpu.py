"""CPU: which branches of g2o's Levenberg-Marquardt loop (optimization_algorithm_levenberg.cpp:100-161) the committed scenes of
the four device optimisers enter.  The GPU tests compare kernels and drivers with the numpy restatements on the scenes of
tests/pose_scene.py, sim3opt_scene.py, lba_scene.py and essential_scene.py: CASES; a branch of the loop that no scene enters is a
branch no test checks.  This census runs the restatements alone, names per optimiser the cases that enter each branch, pins that
table (ENTERED) and asserts that the cases as a whole enter every branch that can be entered - so that an edit of a scene cannot lose
one silently.

The branches (one trial is one pass of the do-while at :102-149):
    accept                 :134 rho > 0 and a finite tempChi: discardTop, lambda shrinks
    reject_accept          :143-147 a rejected trial (pop, lambda *= ni) followed by an accepted one inside the same iteration
    reject_twice           two or more rejected trials in a row in a problem with a free pose / vertex, every |rho| of that
                           iteration above 1e-6 (below it the sign of rho is rounding noise and the GPU tests do not compare counts)
    qmax                   :151 qmax == 10 with every one of the ten |rho| > 1e-6: Terminate
    nbad                   :155-161 _nBad >= 3: Terminate
    rho0                   :151 rho == 0: Terminate
    failed_solve           :126 ok2 == false: tempChi = DBL_MAX
    nonfinite_chi          a trial whose activeRobustChi2 is not finite (:124, before :126 may replace it)
Also counted, not required: qmax_noise (ten trials, some |rho| <= 1e-6) and reject_accept_noise (the same below the threshold).

How they are read.  Local bundle adjustment and the essential graph: from the restatements' traces (per iteration the rhos, the
trial chi2 as summed, the solver's ok; the way a round ended).  Pose optimisation and Sim3 refinement: their traces hold per round
`accepted`, `min_abs_rho`, the iterations and the trials; the per-iteration structure comes from wrappers around Edges.linearize
(a new iteration), solve6 / solve7 (a trial, its ok) and the trial evaluation (its chi2), counted while the restatement runs.  For
those two a round's ending is inferred: it ended before its iteration limit with fewer than ten trials in its last iteration, by
rho == 0 when that round's min |rho| is 0 and by _nBad otherwise; `decisive` uses the round's min |rho| for want of the iteration's.
Every solve is counted by a wrapper for all four (Round.solve, factor_solve, solve6, solve7) and must equal the trials reported.

Unreachable from valid input (finite float32 values that pass the argument checks), and therefore not required:
    essential graph, failed_solve (ORBG_END_SOLVER)   the Sim3 edge's error and its numeric Jacobian are quotients and elementary
                           functions of finite doubles built from finite floats with scales the argument check keeps positive:
                           no overflow, so Hd is finite; every diagonal entry of Hd + lambda I is a sum of squares plus
                           lambda >= 1e-16 > 0, a vertex without edges keeps the pivot lambda, and the factor's pivots are those of
                           a positive definite matrix.  (A pivot rounded to <= 0 would need a condition number near 2^52 at
                           lambda = 1e-16; no committed scene comes within orders of magnitude, and none is required to.)
    :134's g2o_isfinite(tempChi) as the DECIDING test   a chi2 is a sum of squares: tempChi is +inf or NaN when it is not finite,
                           which makes rho -inf or NaN, and rho > 0 has failed already.  nonfinite_chi above is the event, not this.
    pose, Sim3: failed_solve and nonfinite_chi   see "What is missing" - reachable in principle (a point on the camera plane), no scene.

What is missing, by optimiser (no new scene was required for these two):
    pose optimisation      MISSING_POSE below: many cases reject, twice and more in a row, and accept again; none fails a solve,
                           none has a non-finite chi2, none reaches ten trials with every |rho| above 1e-6 (four reach ten in noise).
    Sim3 refinement        MISSING_SIM3 below: rejections in five cases; no failed solve, no non-finite chi2, no ten trials.
    local bundle adjustment   no iteration reaches ten trials and none ends by rho == 0; both are the same two lines of the driver
                           that the essential graph (ten trials) and pose / Sim3 (rho == 0) enter in theirs.
    essential graph        reject_accept only below the noise threshold: see ESSENTIAL_REJECT_ACCEPT.

The failed-solve path of local bundle adjustment (`plane_point`: a point with z == 0.0 seen by a fixed keyframe whose Tcw is the
identity; 1 / z is infinite, that point's Hll and bl are NaN, every Schur pivot is NaN and all five solves of round 1 fail).
Before this census the kernels and tests/lba_ref.py disagreed there, on no scene that got there; g2o's sources decided:
    x after a failed solve      block_solver.hpp:447-457 returns false before anything is written to _x beyond what
                                LinearSolverEigen::solve wrote, and that (linear_solver_eigen.h:103-110) returns before `xx = ...`.
                                _x then holds the previous solve's step - or, at a call's first solve, what `new double[]` left
                                (solver.cpp:54; the memset at :56 is compiled out under NDEBUG).  SparseOptimizer::update applies it
                                all the same (:115) and pop() (:146) restores the estimates.  That reads uninitialised memory, so
                                the kernels' deterministic choice stays: x = 0 after a failed solve, every estimate copied.
    computeScale                :185-187 sums x[j] * (lambda * x[j] + b[j]) over EVERY j, failed solve or not.  With x = 0 that is
                                0 * b[j]: NaN where b[j] is not finite.  k_lba_update skipped every vertex after a failed solve
                                (scale = 0, so rho = (inf - DBL_MAX) / 1e-3 = +inf and the trial was ACCEPTED); it now sums as g2o
                                does, rho is NaN, the trial is rejected and the iteration ends after it (:149 rho < 0 is false).
    computeLambdaInit           :176 maxDiagonal = std::max(fabs(h), maxDiagonal).  std::max(a, b) is (a < b) ? b : a: a NaN h
                                replaces the running maximum and the next h replaces the NaN.  k_lba_lin_reduce used fmax (drops
                                the NaN), lba_ref.py numpy's max (keeps it); both now give the maximum over the entries after the
                                last NaN, in g2o's order (poses, then points), and NaN when the last entry is one.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_ref as ER       # noqa: E402
import essential_scene as ES     # noqa: E402
import lba_ref as LR             # noqa: E402
import lba_scene as LS           # noqa: E402
import pose_ref as PR            # noqa: E402
import pose_scene as PS          # noqa: E402
import sim3opt_ref as SR         # noqa: E402
import sim3opt_scene as SS       # noqa: E402

NOISE = 1e-6
REQUIRED = ("accept", "reject_accept", "reject_twice", "qmax", "nbad", "rho0", "failed_solve", "nonfinite_chi")
OPTIONAL = ("qmax_noise", "reject_accept_noise")
UNREACHABLE = {("essential", "failed_solve"): "Hd + lambda I is positive definite for finite Sim3 edges; a vertex without edges keeps the pivot lambda"}


@contextlib.contextmanager
def counting(owner, name, log, tag):
    """owner.name wrapped: every call appends (tag, result) to log"""
    orig = getattr(owner, name)

    def wrapper(*a, **kw):
        out = orig(*a, **kw)
        log.append((tag, out))
        return out
    setattr(owner, name, wrapper)
    try:
        yield
    finally:
        setattr(owner, name, orig)


def branches_of(rounds):
    """rounds: [dict(free, limit, end (None: by the limit, or 'qmax' / 'rho0' / 'nbad'), its: [dict(acc, ok, tmp, rho (per trial,
    or None), min_abs_rho)])] -> the set of branches entered"""
    got = set()
    for rd in rounds:
        for it in rd["its"]:
            acc, n = it["acc"], len(it["acc"])
            decisive = all(abs(r) > NOISE for r in it["rho"]) if it["rho"] is not None else it["min_abs_rho"] > NOISE
            if any(acc):
                got.add("accept")
            if n > 1 and acc[-1]:
                got.add("reject_accept" if decisive else "reject_accept_noise")
            if rd["free"] and decisive and any(not acc[k] and not acc[k + 1] for k in range(n - 1)):
                got.add("reject_twice")
            if n == 10:
                got.add("qmax" if decisive else "qmax_noise")
            if not all(it["ok"]):
                got.add("failed_solve")
            if not np.isfinite(it["tmp"]).all():
                got.add("nonfinite_chi")
        if rd["end"] in ("nbad", "rho0"):
            got.add(rd["end"])
    return got


def lba_rounds(res):
    out = []
    for r, tr in enumerate(res["trace"]):
        its, k = [], 0
        for i, q in enumerate(tr["trials_it"]):
            its.append(dict(acc=tr["accepted"][k:k + q], ok=tr["oks_it"][i], tmp=tr["tmps_it"][i], rho=tr["rhos_it"][i]))
            k += q
        assert k == len(tr["accepted"]) == tr["trials"]
        out.append(dict(free=res["info"]["free_poses"][r] > 0, end=tr["ends"][0] if tr["ends"] else None, its=its))
    return out


def essential_rounds(res):
    its = [dict(acc=[r > 0.0 and abs(t) <= ER.DBL_MAX for r, t, o in zip(it["rho"], it["tmp"], it["ok"])], ok=it["ok"], tmp=it["tmp"], rho=it["rho"])
           for it in res["trace"].iterations]
    end = {ER.END_ITERATIONS: None, ER.END_QMAX: "qmax", ER.END_RHO0: "rho0", ER.END_SOLVER: "solver", ER.END_NBAD: "nbad"}[res["info"]["end"]]
    return [dict(free=res["info"]["free_vertices"] > 0, end=end, its=its)]


def logged_rounds(res, log, limits):
    """pose / Sim3: the wrappers' log ('L' a linearisation, 'S' a solve -> (ok, x), 'T' a trial evaluation -> (chi2, ...)) cut into
    the rounds and iterations the trace counts"""
    its = []
    for tag, out in log:
        if tag == "L":
            its.append(dict(ok=[], tmp=[]))
        elif tag == "S":
            its[-1]["ok"].append(bool(out[0]))
        else:
            its[-1]["tmp"].append(float(out[0]))
    rounds, k = [], 0
    for r, tr in enumerate(res["trace"]):
        mine, a = its[k:k + tr["iterations"]], 0
        k += tr["iterations"]
        for it in mine:
            q = len(it["ok"])
            assert len(it["tmp"]) == q
            it.update(acc=tr["accepted"][a:a + q], rho=None, min_abs_rho=tr["min_abs_rho"])
            a += q
        assert a == len(tr["accepted"]) == tr["trials"]
        end = None
        if mine and len(mine[-1]["acc"]) == 10:
            end = "qmax"
        elif mine and len(mine) < limits[r]:
            end = "rho0" if tr["min_abs_rho"] == 0.0 and not mine[-1]["acc"][-1] else "nbad"
        rounds.append(dict(free=True, end=end, its=mine))
    assert k == len(its)
    return rounds


def census_pose():
    table = {}
    for name in PS.CASES:
        sc, log = PS.case(name), []
        with counting(PR.Edges, "linearize", log, "L"), counting(PR, "solve6", log, "S"), counting(PR.Edges, "robust_chi2", log, "T"):
            res = PR.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"])
        assert sum(t == "S" for t, _ in log) == sum(res["trials"])
        table[name] = branches_of(logged_rounds(res, log, [10] * 4))
    return table


def census_sim3():
    table = {}
    for name in SS.CASES:
        sc, log = SS.case(name), []
        with counting(SR.Edges, "linearize", log, "L"), counting(SR, "solve7", log, "S"), counting(SR.Edges, "evaluate", log, "T"):
            res = SR.optimize_sim3(sc["matches"], sc["prob"])
        assert sum(t == "S" for t, _ in log) == sum(res["trials"])
        limits = [5] + [10 if tr["flags"].any() else 5 for tr in res["trace"][:1]]      # :1196-1199: ten more iterations when round one dropped a match
        table[name] = branches_of(logged_rounds(res, log, limits))
    return table


def census_lba():
    table = {}
    for name in LS.CASES:
        sc, log = LS.case(name), []
        with counting(LR.Round, "solve", log, "S"):
            res = LR.optimize(sc["kfs"], sc["pts"], sc["obs"])
        ref = LS.reference(name)[1]
        assert res["info"] == ref["info"] and res["kf_est"].tobytes() == ref["kf_est"].tobytes()      # the counted run is the shared reference
        assert len(log) == sum(res["info"]["trials"]) and sum(not o[0] for _, o in log) == sum(not ok for tr in res["trace"] for oks in tr["oks_it"] for ok in oks)
        table[name] = branches_of(lba_rounds(res))
    return table


def census_essential():
    table = {}
    for name in ES.CASES:
        log = []
        with counting(ER, "factor_solve", log, "S"):
            res = ES.run(ES.case(name))
        ref = ES.reference(name)[1]
        assert res["info"] == ref["info"] and res["est"].tobytes() == ref["est"].tobytes()
        assert len(log) == res["info"]["trials"] and [o[1] for _, o in log] == [ok for it in res["trace"].iterations for ok in it["ok"]]
        table[name] = branches_of(essential_rounds(res))
    return table


_tables = {}


def table(opt):
    if opt not in _tables:
        _tables[opt] = dict(pose=census_pose, sim3=census_sim3, lba=census_lba, essential=census_essential)[opt]()
    return _tables[opt]


def entered(opt):
    """-> {branch: sorted cases entering it}"""
    t = table(opt)
    return {b: sorted(n for n in t if b in t[n]) for b in REQUIRED + OPTIONAL if any(b in t[n] for n in t)}


# ---- the pinned table ---------------------------------------------------------------------------------------------------------
# per optimiser the required branches its CASES enter (exactly these), and the cases a branch must keep
ENTERED = {
    "pose": {"accept", "reject_accept", "reject_twice", "nbad", "rho0"},
    "sim3": {"accept", "reject_accept", "reject_twice", "nbad", "rho0"},
    "lba": {"accept", "reject_accept", "reject_twice", "nbad", "failed_solve", "nonfinite_chi"},
    "essential": {"accept", "reject_twice", "qmax", "nbad"},
}
KEEP = {
    ("lba", "reject_accept"): ["far_outliers", "far_start", "outliers", "shuffled"],
    ("lba", "reject_twice"): ["far_outliers", "far_start"],
    ("lba", "failed_solve"): ["plane_point"],
    ("lba", "nonfinite_chi"): ["plane_point"],
    ("essential", "reject_twice"): ["ring_free_scale", "ring_rejected"],
    ("essential", "qmax"): ["ring_free_scale", "ring_rejected"],
    ("essential", "nbad"): ["ring_nbad"],
    ("pose", "reject_twice"): ["far"],
    ("sim3", "reject_twice"): ["far"],
}
# what the two optimisers without new scenes do not enter (the docstring's "What is missing")
MISSING_POSE = {"qmax", "failed_solve", "nonfinite_chi"}
MISSING_SIM3 = {"qmax", "failed_solve", "nonfinite_chi"}
# The essential graph enters reject_accept only below the noise threshold (`wide`, at convergence).  Searched: seeds 700-759 x
# group_rot 1.0-3.0 in steps of 0.25 for `branches`-, free-scale-ring- and fixed-scale-ring-like scenes, for one with a rejected
# and then an accepted trial in one iteration, every |rho| of it above 1e-6, whose 16 draws all show the restatement's `end` and
# `trials_it`: 67 scenes have such an iteration (all `branches`-like: trials [1, 8, ...], seven rho near -1e6 - line 199's B, of
# order 1 / sigma^3 - and then an accepted one), none has more than 2 of 16 draws equal.  Cut short after that iteration
# (iterations=2; seeds 700-733 x group_rot 1, 2, 2.5, 3) the counts often agree in all 16 draws, but S stays between 0.05 and 14:
# the accepted eighth trial itself lands somewhere else in every draw.  Such a scene is chaotic and is not committed; the estimate
# buffers after a reject-then-accept are checked where the same driver code runs on scenes that are not: local bundle adjustment's
# far_start, and ring_rejected's ten popped trials (tests/test_essential_gpu.py: iterations=2 against 3, byte for byte).
ESSENTIAL_REJECT_ACCEPT = "reject_accept_noise"


@pytest.mark.parametrize("opt", ["pose", "sim3", "lba", "essential"])
def test_branches_entered_per_optimiser(opt):
    got = entered(opt)
    for b, cases in got.items():
        print("%-10s %-20s %s" % (opt, b, " ".join(cases)))
    assert {b for b in got if b in REQUIRED} == ENTERED[opt], (opt, sorted(got))
    for (o, b), cases in KEEP.items():
        if o == opt:
            assert set(cases) <= set(got.get(b, [])), (o, b, got.get(b))
    assert not any((opt, b) in UNREACHABLE for b in got)


def test_the_cases_as_a_whole_enter_every_reachable_branch():
    union = set()
    for opt in ENTERED:
        union |= set(entered(opt))
    assert set(REQUIRED) <= union, sorted(set(REQUIRED) - union)
    # per optimiser every required branch is entered, named missing, or named unreachable - nothing is unaccounted for
    missing = {"pose": MISSING_POSE, "sim3": MISSING_SIM3, "lba": {"qmax", "rho0"}, "essential": {"reject_accept", "rho0", "nonfinite_chi"}}
    for opt in ENTERED:
        unreachable = {b for (o, b) in UNREACHABLE if o == opt}
        assert ENTERED[opt] | missing[opt] | unreachable == set(REQUIRED), opt
        assert not ENTERED[opt] & (missing[opt] | unreachable), opt
    assert ESSENTIAL_REJECT_ACCEPT in entered("essential")


def test_far_start_rejects_four_times_with_four_free_poses_and_recovers():
    """the conditions on far_start: the pattern, in the restatement and in each of its 16 draws; round 2's rejecting iteration has
    every |rho| > 1e-6 (so its counts are compared on the GPU); four free poses in both rounds; the same erase flags in every draw"""
    sc, ref, draws, dev = LS.reference("far_start")
    pat = lambda r: ["".join("A" if a else "r" for a in t["accepted"]) for t in r["trace"]]      # noqa: E731
    assert pat(ref) == ["AAAAA", "ArrrrAA"] and ref["info"]["free_poses"] == [4, 4] and len(sc["obs"]) > 150
    assert ref["trace"][1]["trials_it"] == [1, 5, 1] and min(abs(x) for x in ref["trace"][1]["rhos_it"][1]) > 1e-6
    assert ref["trace"][1]["min_abs_rho"] > 1e-6 and ref["trace"][0]["min_abs_rho"] > 1e-6
    for d in draws:
        assert pat(d) == pat(ref) and (d["erase"] == ref["erase"]).all() and (d["flag"] == ref["flag"]).all()
        assert d["trace"][1]["min_abs_rho"] > 1e-6
    assert dev < 1e-9


def test_far_outliers_rejects_in_three_iterations():
    """AAArrArrArrrrrA in every draw; its last trial's |rho| is rounding noise (so round 2's counts fall under the exemption of the
    GPU comparison: the case is kept for the estimates), the iterations that reject twice and accept are decisive"""
    sc, ref, draws, dev = LS.reference("far_outliers")
    pat = lambda r: ["".join("A" if a else "r" for a in t["accepted"]) for t in r["trace"]]      # noqa: E731
    assert pat(ref) == ["AAAAA", "AAArrArrArrrrrA"] and ref["trace"][1]["trials_it"] == [1, 1, 1, 3, 3, 6]
    assert ref["trace"][1]["min_abs_rho"] < 1e-6 and all(min(abs(x) for x in ref["trace"][1]["rhos_it"][i]) > 1e-6 for i in (3, 4))
    assert all(pat(d) == pat(ref) for d in draws)


def test_plane_point_fails_every_solve_of_round_one():
    """one trial per iteration, five iterations, every solve failed, every rho NaN, nothing moved; the plane edge is classified out
    by its depth, an exact 0.0; round 2 is an ordinary one"""
    sc, ref, draws, dev = LS.reference("plane_point")
    t1, t2 = ref["trace"]
    assert t1["trials_it"] == [1] * 5 and not any(t1["accepted"]) and not any(ok for oks in t1["oks_it"] for ok in oks)
    assert all(r != r for rs in t1["rhos_it"] for r in rs) and not np.isfinite([t for ts in t1["tmps_it"] for t in ts]).any()
    only1 = LR.optimize(sc["kfs"], sc["pts"], sc["obs"], schedule=dict(LR.schedule_local(), rounds=1))
    start = LR.optimize(sc["kfs"], sc["pts"], sc["obs"], stop=lambda: True)
    assert only1["kf_est"].tobytes() == start["kf_est"].tobytes() and only1["pt_est"].tobytes() == start["pt_est"].tobytes()
    e = np.nonzero(LS.depth_exempt("plane_point"))[0]
    assert len(e) == 1 and ref["flag"][e[0]] and ref["trace_class"][0]["depth"][e[0]] == 0.0
    assert sc["pts"]["z"][sc["special"]["plane_point"]] == 0.0
    assert (sc["kfs"]["Tcw"][sc["special"]["plane_kf"]].reshape(4, 4) == np.eye(4)).all() and sc["kfs"]["fixed"][sc["special"]["plane_kf"]]
    assert all(t2["oks_it"][i][0] for i in range(len(t2["oks_it"]))) and all(t2["accepted"]) and t2["min_abs_rho"] > 1e-6
    assert ref["info"]["free_poses"] == [4, 4] and ref["info"]["erased"] < len(sc["obs"]) // 4


def test_essential_ring_cases_end_as_named():
    _, nb, draws_nb, _ = ES.reference("ring_nbad")
    it = nb["info"]["iterations"]
    assert nb["info"]["end"] == ER.END_NBAD and nb["info"]["trials_it"][:it] == [1] * 5
    assert min(abs(x) for i in nb["trace"].iterations for x in i["rho"]) > 1e-6
    _, rj, draws_rj, _ = ES.reference("ring_rejected")
    it = rj["info"]["iterations"]
    assert rj["info"]["end"] == ER.END_QMAX and rj["info"]["trials_it"][:it] == [1, 1, 10]
    last = rj["trace"].iterations[-1]["rho"]
    assert max(last) < -0.1 and min(last) > -2.0
    for ref, draws in ((nb, draws_nb), (rj, draws_rj)):
        assert all(d["info"]["end"] == ref["info"]["end"] and d["info"]["trials_it"] == ref["info"]["trials_it"] for d in draws)
