"""GPU: Tracking::Relocalization chained on the device (tests/reloc_chain.py) over the scenes of tests/reloc_scene.py: keyframe
database -> SearchByBoW -> PnPsolver -> PoseOptimization -> SearchByProjection against the keyframe, each stage fed with what the
stage before it gave ON THE DEVICE; nothing is corrected in between.

Demand 1, stage by stage: the restatement of every stage is run on the inputs the device chain actually gave that stage and held
to that stage's own rule - database candidates and order equal; BoW matches equal; PnP every output byte equal (a NaN equal to a
NaN, pnp_scene.assert_equals_restatement); pose optimisation flags and counts equal and the float pose within 1 ulp
(test_poseopt_gpu.check_against_reference's rule); projection matches equal.  The restatements are memoised by input bytes
(reloc_chain.memo): where the device's inputs equal the CPU chain's, the CPU chain's results are reused.

Demand 2, end to end: verdict, winning candidate, the pass in which it won, every nGood and nadditional, the branches taken and the
final mvpMapPoints equal the CPU chain's; the final pose within the optimiser's 1-ulp rule.

The conditions under which equality may be demanded (no count at its borderline, no edge at its threshold, no decision that a
1-ulp pose difference changes) are asserted in tests/test_reloc_chain_cpu.py on the restatements alone."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_scene            # noqa: E402
import reloc_chain as RC    # noqa: E402
import reloc_scene as RS    # noqa: E402

pytestmark = pytest.mark.gpu
_runs = {}


def gpu_chain(name, backend=RC.GpuBackend):
    """one device chain per scene and backend, shared by the tests"""
    key = (name, backend.name)
    if key not in _runs:
        sc = RS.scene(name)
        ch = RC.Chain(backend(sc), sc)
        ch.run()
        _runs[key] = ch
    return _runs[key]


def within_one_ulp(T, ref):
    ulp = np.spacing(np.maximum(np.float32(1), np.abs(ref)).astype(np.float32))
    return bool((np.abs(T.astype(np.float64) - ref.astype(np.float64)) <= ulp).all())


def check_stages(name, ch):
    """Demand 1 on a device chain's trace"""
    sc = RS.scene(name)
    cpu = RC.CpuBackend(sc)
    n = dict(detect=0, bow=0, pnp=0, optimize=0, project=0)
    for e in ch.trace:
        i, o, where = e["in"], e["out"], (name, e["stage"], e["pass"], e["cand"])
        if e["stage"] == "detect":
            assert list(o["candidates"]) == list(cpu.detect(i["bow"])), where
        elif e["stage"] == "bow":
            rn, rm = cpu.bow(sc["kfs"][i["kf"]], sc["query"], sc["map"]["bad"])
            assert o["n"] == rn and (o["match"] == rm).all(), where
        elif e["stage"] == "pnp":
            if not o:                                                    # fewer correspondences than min_inliers: no device call
                assert len(i["corrs"]) < i["min_inliers"], where
                continue
            pnp_scene.assert_equals_restatement(dict(o, info=o, rcounts=o["refined_counts"]), RC.restated_pnp(i), full=False)
        elif e["stage"] == "optimize":
            r = RC.restated_optimize(i["obs"], i["Tcw"], i["outlier"])
            info = o["info"]
            assert (o["ngood"], info["correspondences"], info["bad"], info["rounds"]) == (r["ngood"], r["correspondences"], r["bad"], r["rounds"]), where
            assert (o["outlier"] == r["outlier"]).all(), where
            assert within_one_ulp(o["Tcw"], r["Tcw"]), (where, o["Tcw"], r["Tcw"])
            for rnd, tr in enumerate(r["trace"]):
                if tr["min_abs_rho"] > 1e-6:
                    assert (info["iterations"][rnd], info["trials"][rnd]) == (r["iterations"][rnd], r["trials"][rnd]), (where, rnd)
        elif e["stage"] == "project":
            rn, rh = cpu.project(sc["query"], i["kf"], i["desc"], i["Tcw"], i["holder"], i["th"], i["dist"])
            assert o["n"] == rn and (o["holder"] == rh).all(), where
        else:
            continue
        n[e["stage"]] += 1
    return n


def check_decisions(name, ch):
    """Demand 2 against the CPU chain"""
    g, c = ch.result, RC.cpu_chain(name).result
    assert (g["ok"], g["winner"], g["winner_kf"], g["pass"], g["candidates"]) == (c["ok"], c["winner"], c["winner_kf"], c["pass"], c["candidates"]), name
    assert g["steps"] == c["steps"], (name, [(a, b) for a, b in zip(g["steps"], c["steps"]) if a != b][:3])
    assert (g["mp"] == c["mp"]).all(), name
    assert (g["Tcw"] is None) == (c["Tcw"] is None) and (g["Tcw"] is None or within_one_ulp(g["Tcw"], c["Tcw"])), (name, g["Tcw"], c["Tcw"])


@pytest.mark.parametrize("name", list(RS.SCENES))
def test_device_chain(name):
    ch = gpu_chain(name)
    n = check_stages(name, ch)
    check_decisions(name, ch)
    r = ch.result
    print("%s: verdict %s, winner %d in pass %d; stage calls held to their restatements: %s; final pose equal to the CPU chain's: %s" % (
        name, r["ok"], r["winner"], r["pass"], n, r["Tcw"] is None or bool((r["Tcw"] == RC.cpu_chain(name).result["Tcw"]).all())))


@pytest.mark.parametrize("name", list(RS.SCENES))
def test_batched_device_chain(name):
    """the live candidates of a pass through one iterate_all call, replayed in candidate order up to the first match"""
    ch = gpu_chain(name, RC.GpuBatchedBackend)
    check_stages(name, ch)
    check_decisions(name, ch)
    assert RC.digest(ch) == RC.digest(gpu_chain(name)), name


def test_two_runs_give_the_same_bytes():
    for name in ("narrow", "decoy_first"):
        sc = RS.scene(name)
        again = RC.Chain(RC.GpuBackend(sc), sc)
        again.run()
        assert RC.digest(again) == RC.digest(gpu_chain(name)), name


def test_second_host_thread_after_release(pkg):
    """a second host thread builds its own scratch, mirrors and streams for all five stages and gets the first thread's bytes"""
    first = RC.digest(gpu_chain("decoy_first"))
    assert pkg.matcher_lib().orbx_thread_release_scratch() == pkg.ORBX_OK
    got = {}

    def worker():
        try:
            sc = RS.scene("decoy_first")
            ch = RC.Chain(RC.GpuBackend(sc), sc)
            ch.run()
            got["digest"] = RC.digest(ch)
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001  (shown by the assert below)
            got["error"] = repr(e)
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "error" not in got, got["error"]
    assert got["rc"] == pkg.ORBX_OK and got["digest"] == first
