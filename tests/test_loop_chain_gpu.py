"""GPU: LoopClosing chained on the device (tests/loop_chain.py) over the scenes of tests/loop_scene.py: keyframe database ->
SearchByBoW(KF, KF) -> Sim3Solver -> SearchBySim3 -> SearchByProjection(KF, Scw) -> Fuse(KF, Scw), each stage fed with what the stage
before it gave ON THE DEVICE; nothing is corrected in between.  The refine stage between SearchBySim3 and Scw is the caller's
(loop_chain.refine, a stand-in for Optimizer::OptimizeSim3, the same numpy for every backend).

Demand 1, stage by stage (loop_chain.check_stages): the restatement of every stage is run on the inputs the device chain actually gave
that stage and held to that stage's own rule - database scores equal as doubles, candidates and their order equal; BoW matches equal;
the solver by tests/test_sim3_gpu.py's rule with the tolerance and borderline set of sim3_scene.margins (measured: 0 and empty on every
solver call of these scenes, so every count, flag and model byte is equal); SearchBySim3, projection and Fuse records equal.  The
solver's restatement is memoised by input bytes: where the device's inputs equal the CPU chain's, the CPU chain's result is reused.

Demand 2, end to end (loop_chain.check_decisions): the verdict per current keyframe, the consistency groups after each, the winning
candidate and its pass, every count, the final mvpCurrentMatchedPoints, the loop points, what every Fuse added and replaced and the final
keyframe tables equal the CPU chain's; Scw within the solver's tolerance.

The conditions under which equality may be demanded are asserted in tests/test_loop_chain_cpu.py on the restatements alone."""
import os
import sys
import threading

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_chain as LC     # noqa: E402
import loop_scene as LS     # noqa: E402

pytestmark = pytest.mark.gpu
_runs = {}


def gpu_chain(name, backend=LC.GpuBackend):
    """one device chain per scene and backend, shared by the tests"""
    key = (name, backend.name)
    if key not in _runs:
        sc = LS.scene(name)
        ch = LC.Chain(backend(sc), sc)
        ch.run()
        _runs[key] = ch
    return _runs[key]


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_device_chain(name):
    ch = gpu_chain(name)
    n, tol = LC.check_stages(LS.scene(name), ch)
    LC.check_decisions(ch, LC.cpu_chain(name), tol)
    res = LC.closed(ch.result)
    print("%s: closed %s; stage calls held to their restatements: %s; solver tolerance %g" % (name, None if res is None else (res["kf"], res["winner_kf"], res["pass"]), n, tol))


@pytest.mark.parametrize("name", list(LS.SCENES))
def test_batched_device_chain(name):
    """the live solvers of a keyframe primed by one Sim3Solver.iterate_all call, then the round-robin over the stored results"""
    ch = gpu_chain(name, LC.GpuBatchedBackend)
    _, tol = LC.check_stages(LS.scene(name), ch)
    LC.check_decisions(ch, LC.cpu_chain(name), tol)
    assert LC.digest(ch) == LC.digest(gpu_chain(name)), name


def test_two_runs_give_the_same_bytes():
    for name in ("weak_refine", "decoy_first"):
        sc = LS.scene(name)
        again = LC.Chain(LC.GpuBackend(sc), sc)
        again.run()
        assert LC.digest(again) == LC.digest(gpu_chain(name)), name


def test_second_host_thread_after_release(pkg):
    """a second host thread builds its own scratch, mirrors and streams for every stage and gets the first thread's bytes"""
    first = LC.digest(gpu_chain("weak_refine"))
    assert pkg.matcher_lib().orbx_thread_release_scratch() == pkg.ORBX_OK
    got = {}

    def worker():
        try:
            sc = LS.scene("weak_refine")
            ch = LC.Chain(LC.GpuBackend(sc), sc)
            ch.run()
            got["digest"] = LC.digest(ch)
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001  (shown by the assert below)
            got["error"] = repr(e)
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "error" not in got, got["error"]
    assert got["rc"] == pkg.ORBX_OK and got["digest"] == first
