"""One DetectRelocalizationCandidates call on a long session (orbv_db_detect_reloc), against the reference's algorithm on the host.

  python tools/bench_kfdb.py 4096 1500 20 5          # keyframes, words per vector, timed calls, warm-ups
  rocprofv3 --kernel-trace --stats -- python tools/bench_kfdb.py 4096 1500 20 5 --no-host     # per-kernel times (profiles/README.md)

Scene: a vocabulary of 10^6 words; the session visits 64 places, a place has 6000 words of its own, a keyframe draws its words from
its place (values as tests/kfdb_scene.py makes them: positive, L1-normalised), the query is one more frame of place 0.  The call is
synchronous (it returns the candidates), so a host clock around it is the call's time, PCIe both ways included.  The host figure is
tests/cpp/kfdb_driver.cc's `bench` mode compiled -O3: real inverted lists (std::list per word), stamps, std::map BoW vectors and
L1Scoring::score with its lower_bound skips - the reference's algorithm - on the same database and query, one thread.
"""
import importlib, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("orb_slam2v2-1_amd")

NWORDS, PLACES, PLACE_WORDS = 1000000, 64, 6000


def vector(rng, pool, n):
    w = np.sort(rng.choice(pool, n, replace=False)).astype(np.uint32)
    v = rng.uniform(0.05, 1.0, n)
    return w, v / np.cumsum(v)[-1]


def text(w, v):
    return "%d %s" % (len(w), " ".join("%d %s" % (a, float(b).hex()) for a, b in zip(w, v)))


nkf, nw, calls, warm = [int(a) for a in sys.argv[1:5]]
rng = np.random.default_rng(5)
pools = rng.permutation(NWORDS)[:PLACES * PLACE_WORDS].reshape(PLACES, PLACE_WORDS)
kfs = [vector(rng, pools[i % PLACES], nw) for i in range(nkf)]
qw, qv = vector(rng, pools[0], nw)
db = pkg.KeyFrameDatabase(NWORDS)
t0 = time.perf_counter()
for i, (w, v) in enumerate(kfs):
    db.add(i + 1, w, v)
print("%d adds: %.1f ms; %s" % (nkf, (time.perf_counter() - t0) * 1e3, db.info()), flush=True)
ms = []
for i in range(warm + calls):
    t0 = time.perf_counter()
    cand, hits = db.detect_relocalization_candidates(qw, qv, hits=True)
    ms.append((time.perf_counter() - t0) * 1e3)
ms = ms[warm:]
print("listed %d scored %d candidates %d" % (len(hits), int((hits["flags"] & 1).sum()), len(cand)))
print("detect_reloc ms per call:", " ".join("%.3f" % v for v in ms), "| median %.3f" % float(np.median(ms)), flush=True)
if "--no-host" not in sys.argv:
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "scene.txt"), "w") as f:
            for i, (w, v) in enumerate(kfs):
                f.write("add %d %s\n" % (i + 1, text(w, v)))
            f.write("reloc %s\n" % text(qw, qv))
        lib = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")
        exe = os.path.join(d, "kfdb_driver")
        subprocess.check_call(["g++", "-std=c++11", "-O3", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"),
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "kfdb_driver.cc"), "-L" + lib, "-lorb_host", "-lorbx_hip", "-Wl,-rpath," + lib])
        print(subprocess.run([exe, "bench", str(NWORDS), os.path.join(d, "scene.txt"), str(calls), str(warm)], capture_output=True, text=True,
                             check=True, timeout=600).stdout, flush=True)
