"""GPU: the C++ host classes from three std::threads at once - SearchLocalPointsHIP (Tracking), ORBmatcher::SearchForTriangulation
(LocalMapping) and both ORBmatcher::SearchByBoW overloads with ComputeBoW (LoopClosing) - through the `threads` mode of
tests/cpp/host_driver.cc: each thread runs its mode's body 20 times on the inputs of the single-threaded tests, compares every
result with its first inside the driver, and ends with orbx_thread_release_scratch(); the first results are dumped as the
single-threaded modes dump theirs and compared here with the CPU oracle by the same code (tests/host_cpp_cases.py).  This is the
only test in which the classes' process-wide state (ORBmatcher::device, the Frame statics) is shared by running threads."""
import os
import subprocess

import pytest

import host_cpp_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")
FATAL = (124, 134, 137, 139, -6, -11)
ITERS = 20


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "host_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "host_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_host_classes_from_three_threads(driver, oracle, synth, tmp_path):
    dirs = {name: tmp_path / name for name in ("local", "tri", "bow")}
    for d in dirs.values():
        d.mkdir()
    cases = {"local": host_cpp_cases.local_points_case(oracle, synth, dirs["local"]),
             "tri": host_cpp_cases.triangulation_case(oracle, dirs["tri"], 0),
             "bow": host_cpp_cases.bow_case(oracle, dirs["bow"])}
    cmd = [driver, "threads", ITERS]
    for name in ("local", "tri", "bow"):
        cmd += [name] + list(cases[name][0]) + [dirs[name] / "o"]
    env = dict(os.environ)
    env.setdefault("ORBX_GAUSS_ROUNDING", os.environ.get("ORBX_TEST_GAUSS_FLAVOUR", "half_up"))
    try:
        out = subprocess.run([str(a) for a in cmd], capture_output=True, text=True, env=env, timeout=300)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("the driver did not finish within 300 s\n" + err[-4000:])
    if out.returncode in FATAL:
        pytest.fail("the driver died with status %d\n%s" % (out.returncode, out.stderr[-4000:]))
    assert out.returncode == 0, "status %d\n%s\n%s" % (out.returncode, out.stderr[-4000:], out.stdout[-2000:])   # 7: a thread's iteration differed from its first
    lines = {l.split()[0]: [int(t) for t in l.split()[1:]] for l in out.stdout.splitlines()}
    assert sorted(lines) == ["bow", "local", "tri"], out.stdout
    for name in ("local", "tri", "bow"):
        cases[name][1](lines[name], dirs[name] / "o")
