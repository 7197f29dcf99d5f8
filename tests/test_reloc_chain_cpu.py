"""No GPU: the relocalisation chain (tests/reloc_chain.py) on the restatements alone, over the scenes of tests/reloc_scene.py.

What is asserted here is what tests/test_reloc_chain_gpu.py relies on:
  * each scene takes the branch of Tracking::Relocalization it is named for, and together they enter every one (EXPECT, CENSUS);
  * where the chain says true, the pose is the true one and every map point the frame keeps is the planted one;
  * the conditions of the device comparison hold on every stage call of every scene: pnp_scene.assert_conditions for each PnP
    call, test_poseopt_gpu.MARGIN for each optimisation, and no decision changes when every optimised pose is moved by +-1 float
    ulp in random entries (16 draws per scene);
  * replaying one batched iterate call per pass gives the sequential loop's trace.

Measured on the CPU chain (printed by the tests; the seeds are reloc_scene.SCENES'):
    scene          verdict  winner / pass   |R - R_true|max  |t - t_true|max   wall time of the chain
    direct         true     0 / 0           7.3e-04          1.6e-03           0.3 s
    widen          true     0 / 0           8.2e-04          4.6e-03           0.3 s
    narrow         true     0 / 0           2.7e-04          4.7e-04           0.3 s
    decoy_first    true     1 / 8           2.3e-03          1.8e-02           1.4 s   (its map points are copies moved by 0.03)
    few_matches    true     2 / 0           4.1e-04          2.3e-03           0.3 s
    weak_pose      true     1 / 0           1.2e-03          6.1e-03           0.5 s
    lost           false    -               -                -                 0.4 s
    no_candidates  false    -               -                -                 0.0 s
All 336 projection searches of the 16 perturbed reruns per scene (0 / 16 / 32 / 272 / 0 / 16 / 0 / 0) give the unperturbed result.
The bounds asserted are 4 x the largest measured: room for another seed, not for another answer (a pose that is wrong is off by
tenths, not by thousandths)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_scene            # noqa: E402
import reloc_chain as RC    # noqa: E402
import reloc_scene as RS    # noqa: E402
import test_poseopt_gpu     # noqa: E402  (its MARGIN is the optimiser's rule; importing it needs no GPU)

MARGIN = test_poseopt_gpu.MARGIN
ROT_MEASURED, T_MEASURED = 2.3e-3, 1.8e-2                 # the largest over the scenes (decoy_first: its map points are noisy copies)
DRAWS = 16


def has(steps, p, i, what):
    return any(s[0] == p and s[1] == i and s[2] == what for s in steps)


def value(steps, what, nth=0):
    return [s[3] for s in steps if s[2] == what][nth]


# scene -> what its CPU chain must show; the line numbers are src/Tracking.cc's
EXPECT = {
    "direct": lambda r, b: r["ok"] and value(r["steps"], "ngood_1") >= 50 and "widen" not in b,                                       # :1628
    "widen": lambda r, b: r["ok"] and 10 <= value(r["steps"], "ngood_1") < 50 and value(r["steps"], "ngood_2") >= 50 and "narrow" not in b,   # :1595-1601
    "narrow": lambda r, b: (r["ok"] and 30 < value(r["steps"], "ngood_2") < 50 and value(r["steps"], "narrow") > 0                    # :1605-1621
                            and value(r["steps"], "ngood_3") >= 50 > value(r["steps"], "ngood_2")),
    "decoy_first": lambda r, b: r["ok"] and has(r["steps"], 0, 0, "no_more") and r["winner"] >= 1 and r["pass"] >= 1,                 # :1559
    "few_matches": lambda r, b: "few_matches" in b and "kf_bad" in b and min(s[3] for s in r["steps"] if s[2] == "bow_matches") < 15,   # :1518, :1523
    "weak_pose": lambda r, b: "ngood_lt_10" in b and b.index("ngood_lt_10") < len(b) - 1,                                              # :1587
    "lost": lambda r, b: not r["ok"] and r["Tcw"] is None and b[-1] == "lost" and len(r["candidates"]) >= 2,                           # :1637-1641
    "no_candidates": lambda r, b: not r["ok"] and b == ["no_candidates"] and r["candidates"] == [],                                    # :1495
}
CENSUS = ("no_candidates", "kf_bad", "few_matches", "no_more", "pose", "ngood_lt_10", "widen", "ngood_2", "narrow", "ngood_3", "match", "lost")


def test_scenes_are_small():
    for name in RS.SCENES:
        sc = RS.scene(name)
        assert len(sc["query"]["k"]) <= 300 and all(len(k["k"]) <= 300 for k in sc["kfs"]) and 4 <= len(sc["kfs"]) <= 6, name
        assert 100 <= len(sc["map"]["pos"]) and sc["map"]["bad"].any() and any((k["mp"] < 0).any() for k in sc["kfs"]), name


@pytest.mark.parametrize("name", list(RS.SCENES))
def test_scene_takes_its_branch(name):
    t0 = time.perf_counter()
    ch = RC.cpu_chain(name)
    r = ch.result
    b = RC.branches(r)
    print("%s: %.2f s (first run of the process), candidates %s, verdict %s, winner %d in pass %d" % (name, ch.seconds, r["candidates"], r["ok"], r["winner"], r["pass"]))
    print("    " + " ".join("%s%s" % (s[2], "" if s[3] is None else "=%d" % s[3]) for s in r["steps"][:40]))
    assert EXPECT[name](r, b), (name, r["steps"][:40])
    assert ch.seconds < 5.0, "the restatement of %s takes %.1f s: shrink the scene" % (name, ch.seconds)
    assert time.perf_counter() - t0 < 10.0


def test_every_branch_is_entered_by_some_scene():
    seen = {}
    for name in RS.SCENES:
        for what in RC.branches(RC.cpu_chain(name).result):
            seen.setdefault(what, []).append(name)
    for what in CENSUS:
        print("%-14s %s" % (what, sorted(set(seen.get(what, [])))))
    assert all(what in seen for what in CENSUS), [w for w in CENSUS if w not in seen]
    # the frame's state is carried: some scene adopts a pose more than once, and some scene passes the loop more than once
    assert any(RC.branches(RC.cpu_chain(n).result).count("pose") >= 2 for n in RS.SCENES)
    assert any(max(s[0] for s in RC.cpu_chain(n).result["steps"]) >= 2 for n in RS.SCENES)


def pose_error(sc, r):
    Tt = sc["query"]["Tcw_true"]
    return float(np.abs(r["Tcw"][:3, :3] - Tt[:3, :3]).max()), float(np.abs(r["Tcw"][:3, 3] - Tt[:3, 3]).max())


def test_true_verdicts_are_the_true_pose_and_the_planted_points():
    said_true = 0
    for name in RS.SCENES:
        sc, r = RS.scene(name), RC.cpu_chain(name).result
        if not r["ok"]:
            assert r["Tcw"] is None, name
            continue
        said_true += 1
        er, et = pose_error(sc, r)
        kept = r["mp"] >= 0
        origin = sc["map"]["origin"][np.maximum(r["mp"], 0)]
        wrong = int((kept & (origin != sc["query"]["planted"])).sum())
        print("%s: |R - R_true| %.2e, |t - t_true| %.2e, %d points kept, %d not the planted one" % (name, er, et, kept.sum(), wrong))
        assert er <= 4 * ROT_MEASURED and et <= 4 * T_MEASURED, (name, er, et)
        assert kept.sum() >= 50 and wrong == 0, (name, wrong)
        assert not sc["map"]["bad"][r["mp"][kept]].any()
    assert said_true >= 5


@pytest.mark.parametrize("name", list(RS.SCENES))
def test_conditions_of_the_device_comparison(name):
    """asserted on the restatements alone; a seed under which one fails is not used"""
    ch = RC.cpu_chain(name)
    npnp = nopt = 0
    for e in ch.trace:
        if e["stage"] == "pnp" and e["out"]:
            key = "reloc/%s/%d/%d" % (name, e["pass"], e["cand"])
            pnp_scene._cache[key] = dict(e["in"])                        # the case and its restatement, under a name of their own
            pnp_scene._cache[("ref", key)] = e["out"]
            pnp_scene.assert_conditions(key)
            npnp += 1
        if e["stage"] == "optimize":
            for rnd, tr in enumerate(e["out"]["info"]["trace"]):
                assert tr["min_margin"] > MARGIN, "%s: an edge is %.2e from its threshold in round %d - choose another seed" % (name, tr["min_margin"], rnd)
            nopt += 1
    print("%s: %d PnP calls and %d optimisations meet their stage's conditions" % (name, npnp, nopt))


@pytest.mark.parametrize("name", list(RS.SCENES))
def test_one_ulp_of_the_optimised_pose_changes_nothing(name):
    """the device's float pose may differ from the restatement's by 1 ulp (the optimiser's rule).  Every optimised pose of the chain is
    moved by +-1 ulp in random entries, 16 draws: every projection search that follows gives the same matches and nadditional, and
    every later decision and the final map points are the same"""
    sc, base = RS.scene(name), RC.cpu_chain(name)
    want = [(e["out"]["n"], e["out"]["holder"].tobytes()) for e in base.trace if e["stage"] == "project"]
    survived = 0
    for draw in range(DRAWS):
        ch = RC.Chain(RC.PerturbedBackend(sc, draw), sc)
        r = ch.run()
        got = [(e["out"]["n"], e["out"]["holder"].tobytes()) for e in ch.trace if e["stage"] == "project"]
        assert got == want, (name, draw)
        assert r["steps"] == base.result["steps"] and (r["mp"] == base.result["mp"]).all() and r["ok"] == base.result["ok"], (name, draw)
        survived += len(got)
    print("%s: %d of %d projection searches unchanged under +-1 ulp of the pose" % (name, survived, DRAWS * len(want)))
    assert survived == DRAWS * len(want)


@pytest.mark.parametrize("name", list(RS.SCENES))
def test_batched_replay_equals_the_sequential_loop(name):
    sc = RS.scene(name)
    ch = RC.Chain(RC.CpuBatchedBackend(sc), sc)
    ch.run()
    assert RC.digest(ch) == RC.digest(RC.cpu_chain(name)), name


def test_sets_depend_on_scene_keyframe_and_call_only():
    a, b = RC.scene_sets(3, 1, 0, 40, 35), RC.scene_sets(3, 1, 0, 40, 35)
    assert (a == b).all() and a.shape == (35, 4) and (np.sort(a, axis=1)[:, 1:] != np.sort(a, axis=1)[:, :-1]).all() and a.max() < 40
    assert not (a == RC.scene_sets(3, 1, 1, 40, 35)).all() and not (a == RC.scene_sets(3, 2, 0, 40, 35)).all()
    assert len(RC.scene_sets(3, 1, 0, 9, 0)) == 0
