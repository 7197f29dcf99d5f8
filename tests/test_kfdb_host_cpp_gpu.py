"""GPU: ORB_SLAM2::KeyFrameDatabaseHIP (orb_slam2v2-1_amd/host/KeyFrameDatabase.h) through tests/cpp/kfdb_driver.cc, fed from a
script file: its printed candidates and scores are what the restatement tests/kfdb_ref.py gives for the same calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdb_ref as R        # noqa: E402
import kfdb_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "kfdb_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "kfdb_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def bow_text(v):
    return "%d %s" % (len(v), " ".join("%d %s" % (w, float(x).hex()) for w, x in v))


def ids_text(ids):
    return " ".join(str(i) for i in [len(ids)] + list(ids))


def test_database_class_from_a_script(driver, tmp_path):
    rng = np.random.default_rng(41)
    nwords = 300
    ref = R.Session(nwords)
    kfs, cov = S.crowd(rng, nwords, 70, 40, absent_id=9999)
    script, expect = [], []

    def add(i, v):
        ref.add(i, v); script.append("add %d %s" % (i, bow_text(v)))

    def setcov(i, c):
        ref.set_covisible(i, c); script.append("cov %d %s" % (i, ids_text(c)))

    def queries(q, connected, min_score):
        cand, _, t = ref.detect_reloc(q)
        script.append("reloc " + bow_text(q)); expect.append("reloc:" + "".join(" %d" % i for i in cand))
        cand, _, t = ref.detect_loop(q, connected, min_score)
        script.append("loop %s %s %s" % (bow_text(q), ids_text(connected), float(np.float32(min_score)).hex()))
        expect.append("loop:" + "".join(" %d" % i for i in cand))
        ids = [int(i) for i in rng.choice(sorted(ref.kf), 9, replace=False)]
        script.append("score %s %s" % (bow_text(q), ids_text(ids)))
        expect.append("score:" + "".join(" " + x.hex() for x in ref.score(q, ids)))
        return len(cand), len(t["listed"])

    for i in kfs:
        add(i, kfs[i])
    for i, c in cov.items():
        setcov(i, c)
    stats = [queries(S.random_bow(rng, nwords, 60), [3, 9, 12, 4242], 0.01)]
    for i in (5, 6, 7):
        ref.erase(i); script.append("erase %d" % i)
    add(6, kfs[5]); setcov(6, [1, 2, 3])
    stats.append(queries(S.random_bow(rng, nwords, 60), [], 0.02))
    ref.clear(); script.append("clear")
    for i in list(kfs)[:20]:
        add(i, kfs[i])
    stats.append(queries(S.random_bow(rng, nwords, 50), [1], 0.0))
    expect.append("size: 20")
    assert all(c >= 1 and l >= 15 for c, l in stats), stats
    (tmp_path / "script.txt").write_text("\n".join(script) + "\n")
    out = subprocess.run([driver, "db", str(nwords), "256", str(tmp_path / "script.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    got = out.stdout.strip().split("\n")
    assert len(got) == len(expect)
    for g, e in zip(got, expect):
        if e.startswith("score:"):
            assert [float.fromhex(x) for x in g.split()[1:]] == [float.fromhex(x) for x in e.split()[1:]], (g, e)
        else:
            assert g == e
