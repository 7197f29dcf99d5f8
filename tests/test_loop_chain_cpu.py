"""No GPU: the loop-closing chain (tests/loop_chain.py) on the restatements alone, over the scenes of tests/loop_scene.py.

What is asserted here is what tests/test_loop_chain_gpu.py relies on:
  * each scene takes the branch of LoopClosing it is named for, and together they enter every one (EXPECT, CENSUS);
  * where a loop is accepted, Scw is the planted similarity and every matched or fused point is the planted counterpart;
  * the conditions of the device comparison hold on every stage call (test_conditions_of_the_device_comparison,
    test_one_ulp_of_every_sim3_changes_nothing);
  * every mutation of the bookkeeping is noticed by a scene; one batched iterate_all per keyframe replays to the sequential trace.

Measured on the CPU chain (printed by the tests; the seeds are loop_scene.SCENES'):
    scene          closes at / candidate / pass   |s - s_true|  |R - R_true|max  |t - t_true|max  matched (BoW+Sim3 kept by refine, +projection)  Fuse adds / replaces
    closed         15 / [3] 0 / 0                 1.6e-04       2.6e-04          1.4e-03          125 (79 + 46)                                  14 / 14
    too_recent     - (12, 13 are too recent)      -             -                -                -                                              -
    no_candidates  17 / [3] 0 / 0                 1.5e-04       4.2e-04          2.1e-03          119 (78 + 41)                                  15 / 19
    inconsistent   - (groups {2,3,4}, {1} in turn) -            -                -                -                                              -
    few_bow        15 / [0, 1, 3] 2 / 0           3.4e-04       1.3e-04          1.8e-03          122 (82 + 40)   (0: 3 BoW matches, 1: bad)     10 / 14
    decoy_first    15 / [0, 3] 1 / 3              2.8e-04       4.3e-04          2.3e-03          91 (46 + 45)    (0: 21 pairs, 3 iterations)    11 / 11
    weak_refine    15 / [0, 3] 1 / 0              7.0e-05       2.3e-04          1.0e-03          116 (74 + 42)   (0: 28 inliers, refine 17)     6 / 12
    few_total      - (refine 30, total 35 < 40)   -             -                -                35 (30 + 5)                                    -
    fixed_scale    15 / [3] 0 / 0                 3.1e-08       2.0e-04          1.6e-03          129 (84 + 45)                                  10 / 9
No matched, added or replaced point is another than the planted counterpart.  The bounds asserted are 4 x the largest measured: room
for another seed, not for another answer (a Scw without Smw, or a neighbour under the current keyframe's Sim3, is off by tenths).
Conditions: the solver's tolerance (sim3_scene.margins, +-2 ulp on atan2 / sin / cos) is 0 and its borderline set empty on all 9 solver
calls (0 of 13 023 evaluations); no database score within 1 ulp of minScore or of 0.75 bestAccScore in 36 queries; no window matcher's
best distance at TH_LOW / TH_HIGH; SearchByBoW meets `best == 0.75 second` 5 times and `best == TH_LOW` once, both exact and defined by
bow_scene.planted_case; all 848 matcher calls of the 16 perturbed reruns per scene give the unperturbed records.
decoy_first: with 21 correspondences SetRansacParameters leaves the decoy 3 iterations, so it answers bNoMore in pass 0; a candidate
that uses up all 300 AND is followed by a winner would need the winner to miss 59 passes.
Mutations, and the scenes whose checks (problems()) they trip; every other scene with a solver call at least gives other records:
    min_score_double        every scene: the minimum score handed on is no float (the callees narrow it again, so no decision moves)
    no_index_map            decoy_first: Scw is not the planted similarity
    sigma_from_slot         every scene with a solver: a pair's sigma2 is not that of the keypoints planted for its points
    keep_non_inliers        decoy_first, few_total: another branch
    groups_not_cleared      no_candidates: closes a keyframe early
    scw_is_scm              every accepting scene: Scw is not the planted similarity, the neighbours fuse nothing
    loop_points_duplicated  every scene with a match: a loop point listed twice
    fuse_with_current_scw   closed, no_candidates, few_bow, decoy_first, weak_refine: the neighbours fuse next to nothing"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_chain as LC     # noqa: E402
import loop_scene as LS     # noqa: E402
import sim3_scene           # noqa: E402

DRAWS = 16
S_MEASURED, ROT_MEASURED, T_MEASURED = 3.5e-4, 4.3e-4, 2.4e-3     # the largest |s - s_true|, |R - R_true|, |t - t_true| over the scenes (docstring table)


def steps_of(r, what):
    return [s for s in r["steps"] if s[2] == what]


def last_run(sc, r):
    return LC.closed(r) is not None and LC.closed(r)["kf"] == sc["run"][-1]


# scene -> what its CPU chain must show; the line numbers are src/LoopClosing.cc's
EXPECT = {
    "closed": lambda sc, r, b: last_run(sc, r) and LC.closed(r)["enough"] == [3] and LC.closed(r)["winner"] == 0 and "weak_refine" not in b,   # :395-400
    "too_recent": lambda sc, r, b: b.count("too_recent") == 2 and [s[0] for s in steps_of(r, "too_recent")] == [12, 13] and LC.closed(r) is None,   # :124
    "no_candidates": lambda sc, r, b: (b.count("no_candidates") == 1 and r["results"][1]["groups"] == [] and                                  # :154-157
                                       all(n == 0 for _, n in r["results"][2]["groups"]) and len(r["results"][2]["groups"]) > 0 and last_run(sc, r)),
    "inconsistent": lambda sc, r, b: ("no_candidates" not in b and b.count("not_enough") == len(sc["run"]) and                               # :204, :213-217
                                      all(len(x["candidates"]) > 0 and all(n == 0 for _, n in x["groups"]) for x in r["results"])),
    "few_bow": lambda sc, r, b: "few_bow" in b and "kf_bad" in b and min(s[3] for s in steps_of(r, "bow_matches")) < 20 and last_run(sc, r),  # :269, :277
    "decoy_first": lambda sc, r, b: (any(s[1] == 0 for s in steps_of(r, "no_more")) and last_run(sc, r) and LC.closed(r)["winner"] >= 1       # :314
                                     and LC.closed(r)["pass"] >= 1),
    "weak_refine": lambda sc, r, b: ("weak_refine" in b and min(s[3] for s in steps_of(r, "refine")) < 20 and last_run(sc, r)                  # :339
                                     and b.index("weak_refine") < b.index("matched")),
    "few_total": lambda sc, r, b: ("few_total" in b and LC.closed(r) is None and steps_of(r, "refine")[-1][3] >= 20                           # :395, :402
                                   and steps_of(r, "total")[-1][3] < 40),
    "fixed_scale": lambda sc, r, b: last_run(sc, r) and sc["fix_scale"] and scale_of(LC.closed(r)["mScw"]) == pytest.approx(1.0, abs=1e-6),
}
CENSUS = ("too_recent", "no_candidates", "not_enough", "enough", "kf_bad", "few_bow", "no_more", "sim3", "weak_refine", "matched", "few_total", "accepted")


def scale_of(S):
    return float(np.sqrt((np.asarray(S, np.float64)[0, :3] ** 2).sum()))


def pose_error(sc, res):
    St, S = sc["Scw_true"][res["kf"]], res["mScw"].astype(np.float64)
    s, st = scale_of(S), scale_of(St)
    return abs(s - st), float(np.abs(S[:3, :3] / s - St[:3, :3] / st).max()), float(np.abs(S[:3, 3] - St[:3, 3]).max())


def wrong_points(sc, res):
    """matched or fused points that are not the planted counterpart -> (matched wrong, added wrong, replaced wrong, totals)"""
    origin = sc["map"]["origin"]
    cur = sc["kfs"][res["kf"]]
    mt = res["matched"]
    w_m = int(((mt >= 0) & (origin[np.maximum(mt, 0)] != cur["planted"])).sum())
    w_a = w_r = na = nr = 0
    for k, f in res["fused"].items():
        for j, p in f["added"]:
            na += 1
            w_a += int(origin[p] != sc["kfs"][k]["planted"][j])
        for old, new in f["replaced"]:
            nr += 1
            w_r += int(origin[old] != origin[new])
    return w_m, w_a, w_r, int((mt >= 0).sum()), na, nr


def problems(sc, ch):
    """what a run of the chain shows that a right run of this scene must not -> list of findings"""
    r, out = ch.result, []
    b = LC.branches(r)
    try:
        if not EXPECT[sc["name"]](sc, r, b):
            out.append("branch")
    except (IndexError, ValueError, KeyError, TypeError):
        out.append("branch")
    for s in steps_of(r, "min_score"):
        v = float.fromhex(s[3])
        if float(np.float32(v)) != v:
            out.append("min_score is no float")
    m = sc["map"]
    where = {m["pos"][j].tobytes(): j for j in range(len(m["pos"]))}
    for e in ch.trace:                                                   # a pair's sigma2 against the keypoints that were PLANTED for its two points
        if e["stage"] != "sim3":
            continue
        for side, kf in (("1", sc["kfs"][e["kf"]]), ("2", sc["kfs"][e["cand"]])):
            for pr in e["in"]["pairs"]:
                o = m["origin"][where[pr["w" + side].tobytes()]]
                at = np.nonzero(kf["planted"] == o)[0] if o >= 0 else []
                if len(at) and pr["sigma2_" + side] != LS.LEVEL_SIGMA2[kf["k"]["octave"][at[0]]]:
                    out.append("a pair's sigma2 is not its keypoint's")
    for res in r["results"]:
        if "loop_points" in res and len(set(res["loop_points"].tolist())) != len(res["loop_points"]):
            out.append("a loop point listed twice")
        if res["closed"]:
            es, er, et = pose_error(sc, res)
            if not (es <= 4 * S_MEASURED and er <= 4 * ROT_MEASURED and et <= 4 * T_MEASURED):
                out.append("Scw is not the planted similarity")
            w = wrong_points(sc, res)
            if w[0] or w[1] or w[2]:
                out.append("a matched or fused point is not the planted one")
            if w[3] < 40:
                out.append("fewer than 40 matches")
            nb = [k for k in res["fused"] if k != res["kf"]]
            if sum(res["fused"][k]["n"] for k in nb) < 2 * len(nb):
                out.append("the neighbours fuse next to nothing")
    return out


def test_scenes_are_small():
    for name in LS.SCENES:
        sc = LS.scene(name)
        assert all(len(k["k"]) <= 300 for k in sc["kfs"].values()) and 10 <= len(sc["kfs"]) <= 14, name
        assert sc["map"]["bad"].any() and all((sc["kfs"][i]["mp"] < 0).any() for i in (2, 3, 4) + tuple(sc["run"])), name
        assert len(sc["run"]) >= 4 and min(sc["run"]) >= 10
    assert any(k["bad"] for k in LS.scene("few_bow")["kfs"].values())
    assert LS.scene("fixed_scale")["fix_scale"] and LS.scene("closed")["scale"] != 1.0


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_scene_takes_its_branch(name):
    ch = LC.cpu_chain(name)
    sc, r = LS.scene(name), ch.result
    b = LC.branches(r)
    print("%s: %.2f s; %s" % (name, ch.seconds, " ".join("%s%s" % (s[2], "" if s[3] is None or s[2] in ("groups", "min_score") else "=%s" % (s[3],)) for s in r["steps"]
                                                        if s[2] not in ("groups", "min_score", "fused"))))
    assert EXPECT[name](sc, r, b), (name, r["steps"])
    assert ch.seconds < 5.0, "the restatement of %s takes %.1f s: shrink the scene" % (name, ch.seconds)


def test_every_branch_is_entered_by_some_scene():
    seen = {}
    for name in LS.SCENES:
        for what in LC.branches(LC.cpu_chain(name).result):
            seen.setdefault(what, []).append(name)
    for what in CENSUS:
        print("%-14s %s" % (what, sorted(set(seen.get(what, [])))))
    assert all(what in seen for what in CENSUS), [w for w in CENSUS if w not in seen]
    # the state is carried: some group reaches consistency 3, some solver is iterated in more than one pass, some scene fuses by Replace
    assert any(n >= 3 for name in LS.SCENES for x in LC.cpu_chain(name).result["results"] for _, n in x["groups"])
    assert any(LC.closed(LC.cpu_chain(n).result) and LC.closed(LC.cpu_chain(n).result)["pass"] >= 1 for n in LS.SCENES)
    assert any(f["replaced"] for n in LS.SCENES if LC.closed(LC.cpu_chain(n).result) for f in LC.closed(LC.cpu_chain(n).result)["fused"].values())


def test_accepted_loops_are_the_planted_similarity_and_the_planted_points():
    accepted = 0
    worst = [0.0, 0.0, 0.0]
    for name in LS.SCENES:
        sc, r = LS.scene(name), LC.cpu_chain(name).result
        res = LC.closed(r)
        if res is None:
            continue
        accepted += 1
        e = pose_error(sc, res)
        worst = [max(a, b) for a, b in zip(worst, e)]
        w = wrong_points(sc, res)
        print("%-14s |s - s_true| %.2e  |R - R_true| %.2e  |t - t_true| %.2e; matched %d (%d wrong), added by Fuse %d (%d wrong), replaced %d (%d wrong)" % (
            name, e[0], e[1], e[2], w[3], w[0], w[4], w[1], w[5], w[2]))
        assert e[0] <= 4 * S_MEASURED and e[1] <= 4 * ROT_MEASURED and e[2] <= 4 * T_MEASURED, (name, e)
        assert w[:3] == (0, 0, 0) and w[3] >= 40, (name, w)
        assert not sc["map"]["bad"][res["matched"][res["matched"] >= 0]].any()
    print("largest: %.2e %.2e %.2e" % tuple(worst))
    assert accepted >= 6
    for name in LS.SCENES:
        assert problems(LS.scene(name), LC.cpu_chain(name)) == [], name


def one_ulp_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, np.float32(np.inf)) == b or np.nextafter(a, np.float32(-np.inf)) == b


def tie_census(sc, ch):
    """best distances that sit AT a threshold (TH_LOW for SearchByBoW's `<` and the projections' `<=`, TH_HIGH for SearchBySim3's `>`), and
    SearchByBoW ratios that are equalities -> counts"""
    import oracle
    geom, cam = oracle.grid_geom(LS.W, LS.H), oracle.Cam(*LS.CAM)
    at = dict(bow=0, ratio=0, by_sim3=0, project=0, fuse=0)
    bits = lambda d: np.unpackbits(d, axis=1).astype(np.int16)   # noqa: E731
    tables, bad = {i: k["mp"] for i, k in sc["kfs"].items()}, sc["map"]["bad"]   # before any fusion: SearchByBoW runs before it
    for e in ch.trace:
        i = e["in"]
        if e["stage"] == "bow":
            cur, kf2 = sc["kfs"][e["kf"]], sc["kfs"][e["cand"]]
            qd, _, qv, cd, _, cv = LC.CpuBackend.bow_args(cur, kf2, tables, bad)[:6]
            D = (bits(qd)[:, None, :] != bits(cd)[None, :, :]).sum(axis=2)[qv != 0][:, cv != 0]
            if D.size and D.shape[1] >= 2:
                srt = np.sort(D, axis=1)
                at["bow"] += int((srt[:, 0] == LC.TH_LOW).sum())
                at["ratio"] += int((srt[:, 0].astype(np.float32) == np.float32(0.75) * srt[:, 1].astype(np.float32)).sum())
        elif e["stage"] == "search_by_sim3":
            k1, k2 = sc["kfs"][e["kf"]], sc["kfs"][e["cand"]]
            q1, q2 = oracle.sim3_pair_window_queries(geom, LS.SF, LS.LOG_SF, cam, k1["Tcw"], k2["Tcw"], i["s"], i["R"], i["t"], i["pts1"], i["pts2"], 7.5)
            at["by_sim3"] += int((oracle.best_in_windows(k2["k"], k2["d"], None, geom, q1, i["pd1"])[1] == LC.TH_HIGH).sum())
            at["by_sim3"] += int((oracle.best_in_windows(k1["k"], k1["d"], None, geom, q2, i["pd2"])[1] == LC.TH_HIGH).sum())
        elif e["stage"] in ("project_sim3", "fuse_sim3"):
            kf = sc["kfs"][e["kf"] if e["stage"] == "project_sim3" else e["cand"]]
            q = oracle.sim3_window_queries(i["pts"], geom, LS.SF, LS.LOG_SF, cam, i["Scw"], 10.0 if e["stage"] == "project_sim3" else 4.0)
            at["project" if e["stage"] == "project_sim3" else "fuse"] += int((oracle.best_in_windows(kf["k"], kf["d"], None, geom, q, i["pd"])[1] == LC.TH_LOW).sum())
    return at


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_conditions_of_the_device_comparison(name):
    """asserted on the restatements alone; a seed under which one fails is not used"""
    sc, ch = LS.scene(name), LC.cpu_chain(name)
    nsim = ndet = 0
    bl_total = ev_total = 0
    tol = 0.0
    for e in ch.trace:
        if e["stage"] == "sim3":
            key = LC.sim3_case(e["in"])
            dm, de = sim3_scene.margins(key)
            _, _, bl = sim3_scene.assert_conditions(key, 4 * de)
            tol = max(tol, 4 * dm)
            bl_total += int(bl.sum())
            ev_total += bl.size
            nsim += 1
        if e["stage"] == "detect":
            t, ms = e["aux"], np.float32(e["in"]["min_score"])
            for k in t["scored"]:
                assert not one_ulp_apart(k.mLoopScore, ms), "%s: keyframe %d scores within 1 ulp of minScore - choose another seed" % (name, k.mnId)
            for a, _ in t["acc"]:
                assert not one_ulp_apart(a, t["minScoreToRetain"]), "%s: an accumulated score within 1 ulp of 0.75 bestAccScore - choose another seed" % name
            ndet += 1
    at = tie_census(sc, ch)
    print("%s: %d solver calls (tolerance %g, %d borderline of %d evaluations), %d database queries; best distances at a threshold: %s" % (
        name, nsim, tol, bl_total, ev_total, ndet, at))
    # SearchByBoW's two edges are defined by tests/bow_scene.py: planted_case (at_max_dist, over_max_dist, *_edge: d1 == 0.75 d2) and are exact
    # in integers and floats; the window matchers' are not planted anywhere, so none may occur here
    assert not (at["by_sim3"] or at["project"] or at["fuse"]), (name, at)


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_one_ulp_of_every_sim3_changes_nothing(name):
    """every Sim3 that leaves the solver or the refine stage is moved by +-1 float ulp in random entries, 16 draws: every matcher call
    that follows gives the same records, and every decision, list and table is the same"""
    sc, base = LS.scene(name), LC.cpu_chain(name)
    want = LC.digest(base, scw=False)
    calls = sum(e["stage"] in ("search_by_sim3", "project_sim3", "fuse_sim3") for e in base.trace)
    for draw in range(DRAWS):
        ch = LC.Chain(LC.PerturbedBackend(sc, draw), sc)
        ch.run()
        assert LC.digest(ch, scw=False) == want, (name, draw)
    print("%s: %d of %d matcher calls unchanged under +-1 ulp of the Sim3s" % (name, DRAWS * calls, DRAWS * calls))


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_batched_replay_equals_the_sequential_loop(name):
    sc = LS.scene(name)
    ch = LC.Chain(LC.CpuBatchedBackend(sc), sc)
    ch.run()
    assert LC.digest(ch) == LC.digest(LC.cpu_chain(name)), name


def test_every_mutation_is_noticed():
    """a chain with one point of the bookkeeping wrong gives, on some scene, other decisions or records than the right chain
    (`differs`), and on the scenes named here a finding of problems() as well"""
    noticed = {}
    for mut in LC.MUTATIONS:
        for name in LS.SCENES:
            sc = LS.scene(name)
            ch = LC.Chain(LC.CpuBackend(sc), sc, mutate=mut)
            ch.run()
            found = problems(sc, ch)
            if found or LC.digest(ch) != LC.digest(LC.cpu_chain(name)):
                noticed.setdefault(mut, []).append((name, sorted(set(found)) or ["differs"]))
    for mut in LC.MUTATIONS:
        print("%-24s %s" % (mut, "; ".join("%s: %s" % (n, ", ".join(f)) for n, f in noticed.get(mut, []))))
    assert all(mut in noticed for mut in LC.MUTATIONS), [m for m in LC.MUTATIONS if m not in noticed]
    assert all(any(f != ["differs"] for _, f in noticed[mut]) for mut in LC.MUTATIONS), "a mutation changes records but trips no check"


STAGE_FIELD = dict(score="scores", detect="candidates", bow="match", sim3="counts", search_by_sim3="match", project_sim3="matched", fuse_sim3="replace")


@pytest.mark.parametrize("stage", list(STAGE_FIELD))
def test_stage_check_fails_at_the_stage_whose_result_is_altered(stage):
    """loop_chain.check_stages, which holds the device chain to the restatements stage by stage, on the CPU chain's own trace: it passes;
    with ONE element of one stage's result altered it fails, and names that stage"""
    import copy
    sc, ch = LS.scene("closed"), LC.cpu_chain("closed")
    n, tol = LC.check_stages(sc, ch)
    assert all(v > 0 for v in n.values()) and tol == 0, n
    fake = copy.copy(ch)
    fake.trace = [dict(e, out=dict(e["out"])) for e in ch.trace]
    e = [x for x in fake.trace if x["stage"] == stage][-1]
    v = e["out"][STAGE_FIELD[stage]]
    if stage == "detect":
        e["out"]["candidates"] = list(v) + [5]
    else:
        v = np.array(v).copy()
        v.flat[len(v.flat) // 2] += 1
        e["out"][STAGE_FIELD[stage]] = v
    with pytest.raises(AssertionError, match="stage %s," % stage):
        LC.check_stages(sc, fake)


def test_sets_depend_on_scene_and_the_two_keyframes_only():
    a, b = LC.scene_sets(3, 15, 3, 40, 35), LC.scene_sets(3, 15, 3, 40, 35)
    assert (a == b).all() and a.shape == (35, 3) and (np.sort(a, axis=1)[:, 1:] != np.sort(a, axis=1)[:, :-1]).all() and a.max() < 40
    assert not (a == LC.scene_sets(3, 15, 0, 40, 35)).all() and not (a == LC.scene_sets(3, 14, 3, 40, 35)).all()
    assert len(LC.scene_sets(3, 15, 3, 9, 0)) == 0
