"""GPU: the loop-closing chain (tests/loop_chain.py, imported and not edited) closed with the REAL optimiser: the refine stage between
SearchBySim3 and Scw = Scm * Smw is Optimizer::OptimizeSim3 - orbz_optimize_sim3 on the device chain, its restatement
tests/sim3opt_ref.py on the numpy chain - instead of loop_chain.refine's stand-in.  Both chains feed the optimiser the rows the
reference's filter accepts (src/Optimizer.cc:1104-1141), built once by the same code.  On the scenes `closed` and `weak_refine`:
every step decision of the two chains is equal, the loop closes at the keyframe the scene is built to close at, and the refined
Sim3 is at least as close to the scene's truth as the solver's estimate that went in.  The condition of the comparison - no edge of
any optimiser call within MARGIN of th2 - is asserted on the restatement's trace.

`weak_refine` runs at another seed of its generator than tests/loop_scene.py keeps for the stand-in (107 instead of 7).  The scene is
built so that a biased copy of the place is answered first and fails the optimiser's `>= 20`.  The stand-in's closed-form fit kept
17 of its matches at seed 7; the real optimiser - Levenberg-Marquardt under the Huber kernel - keeps 25 there, so the copy wins, the
projection search then finds only 30 matches in all and the loop is not closed at all.  Of the seeds 1..160, looked at on the numpy
chain, the biased copy is answered first AND refined below 20 by the real optimiser at two (107: 18 of 50 rows, 113: 18 of 52); both
then close on keyframe 3 with 74 / 73 inliers, no optimiser edge is nearer than 2.8e-2 to th2, and every solver call meets the
conditions of tests/test_sim3_gpu.py with tolerance 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_chain as LC        # noqa: E402
import loop_scene as LS        # noqa: E402
import sim3opt_ref as R        # noqa: E402
from sim3opt_scene import MARGIN   # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TH2 = 10.0          # src/LoopClosing.cc:336


class RefinedChain(LC.Chain):
    """loop_chain.Chain with Optimizer::OptimizeSim3 as its refine stage; optimise(rows, problem) is the backend's"""

    def __init__(self, backend, sc, optimise):
        super().__init__(backend, sc)
        self.optimise, self.refines = optimise, []

    def _refine(self, cur, kf2, vp, srt):
        t1, t2 = self.tables[cur["id"]], self.tables[kf2["id"]]
        m = self.sc["map"]
        at, a2 = [], []
        for i in range(len(vp)):                                         # src/Optimizer.cc:1104-1141
            if vp[i] < 0 or t1[i] < 0 or self.bad[t1[i]] or self.bad[vp[i]]:
                continue
            i2 = LC.index_in(t2, vp[i])
            if i2 >= 0:
                at.append(i)
                a2.append(i2)
        at, a2 = np.array(at, np.int64), np.array(a2, np.int64)
        rows = np.zeros(len(at), R.MATCH_DTYPE)
        if len(at):
            rows["w1"], rows["w2"] = m["pos"][t1[at]], m["pos"][vp[at]]
            rows["u1"], rows["v1"] = cur["k"]["x"][at], cur["k"]["y"][at]
            rows["u2"], rows["v2"] = kf2["k"]["x"][a2], kf2["k"]["y"][a2]
            rows["inv_sigma2_1"], rows["inv_sigma2_2"] = LS.INV_LEVEL_SIGMA2[cur["k"]["octave"][at]], LS.INV_LEVEL_SIGMA2[kf2["k"]["octave"][a2]]
        prob = np.zeros(1, R.PROBLEM_DTYPE)
        prob["Tcw1"], prob["Tcw2"], prob["K1"], prob["K2"] = cur["Tcw"].reshape(16), kf2["Tcw"].reshape(16), LS.K, LS.K
        prob["s"], prob["R"], prob["t"] = srt[0], np.asarray(srt[1], f32).reshape(9), np.asarray(srt[2], f32).reshape(3)
        prob["th2"], prob["fix_scale"] = TH2, int(self.sc["fix_scale"])
        n, dropped, rounds, q, t, s = self.optimise(rows, prob[0])
        kept = np.full(len(vp), -1, np.int64)
        live = dropped == 0
        kept[at[live]] = vp[at[live]]                                    # a dropped match becomes null (:1201, :1235); so does one without an edge
        out = (f32(s), R.quat_to_R(q).astype(f32), np.asarray(t, f64).astype(f32)) if rounds == 2 else (f32(srt[0]), np.asarray(srt[1], f32), np.asarray(srt[2], f32))
        self.refines.append(dict(kf=cur["id"], cand=kf2["id"], rows=rows, prob=prob[0].copy(), n=int(n), rounds=int(rounds), srt_in=srt, srt_out=out))
        return int(n), out, kept


def device_optimise(pkg):
    def run(rows, prob):
        _, dropped, n, info = pkg.optimize_sim3(rows, prob)
        return n, dropped, info["rounds"], info["q"], info["t"], info["s"]
    return run


def restated_optimise(traces):
    def run(rows, prob):
        r = R.optimize_sim3(rows, prob)
        traces.append(r["trace"])
        return r["ninliers"], r["dropped"], r["rounds"], r["q"], r["t"], r["s"]
    return run


def distance(sc, cid, kid, srt):
    """how far Scw = Scm * Smw made of (s, R, t) is from the scene's true Scw of keyframe cid: the largest entry of the difference"""
    Scw = LC.sim3_matrix(*srt) @ sc["kfs"][kid]["Tcw"].astype(f64)
    return float(np.abs(Scw[:3] - np.asarray(sc["Scw_true"][cid], f64)[:3]).max())


SEEDS = {"closed": None, "weak_refine": 107}       # None: the seed tests/loop_scene.py keeps


@pytest.mark.parametrize("name", ["closed", "weak_refine"])
def test_chain_closes_with_the_real_optimiser(pkg, name):
    sc = LS.scene(name, SEEDS[name])
    traces = []
    cpu = RefinedChain(LC.CpuBackend(sc), sc, restated_optimise(traces))
    cpu.run()
    gpu = RefinedChain(LC.GpuBackend(sc), sc, device_optimise(pkg))
    gpu.run()
    # the condition: no optimiser call of this scene has an edge within MARGIN of th2 (else: another seed of the scene generator)
    assert traces and all(tr["min_margin"] > MARGIN for call in traces for tr in call), name
    assert gpu.result["steps"] == cpu.result["steps"], [(a, b) for a, b in zip(gpu.result["steps"], cpu.result["steps"]) if a != b][:3]
    # the float Scw carries the optimiser's own deviation: 64 x S by the rule of tests/test_sim3opt_gpu.py, with S = 1e-7, what the
    # restatement shows at these sizes (tests/test_sim3opt_cpu.py prints it per case: 3e-8 .. 3e-7), + a float ulp of entries below 8
    tol = max(LC.check_stages(sc, gpu)[1], 64 * 1e-7 + 5e-7)
    LC.check_decisions(gpu, cpu, tol)
    for ch in (cpu, gpu):
        res = LC.closed(ch.result)
        assert res is not None and res["kf"] == sc["run"][-1] and res["winner_kf"] == 3, name      # M(): keyframe 3 holds the place
        win = [r for r in ch.refines if r["kf"] == res["kf"] and r["cand"] == res["winner_kf"] and r["n"] >= 20][-1]
        d_in, d_out = distance(sc, win["kf"], win["cand"], win["srt_in"]), distance(sc, win["kf"], win["cand"], win["srt_out"])
        print("%s (%s): %d optimiser calls; winner %d rows -> %d inliers; distance to the true Scw %.3e -> %.3e" % (
            name, ch.be.name, len(ch.refines), len(win["rows"]), win["n"], d_in, d_out))
        assert win["rounds"] == 2 and d_out <= d_in
        if name == "weak_refine":                                                                  # the biased copy came first and failed `>= 20`
            b = LC.branches(ch.result)
            assert "weak_refine" in b and b.index("weak_refine") < b.index("matched") and ch.refines[0]["cand"] == 0 and ch.refines[0]["n"] < 20
    assert [(r["kf"], r["cand"], r["n"], r["rounds"]) for r in gpu.refines] == [(r["kf"], r["cand"], r["n"], r["rounds"]) for r in cpu.refines]
    assert all((a["rows"].tobytes(), a["prob"].tobytes()) == (b["rows"].tobytes(), b["prob"].tobytes()) for a, b in zip(gpu.refines, cpu.refines))
