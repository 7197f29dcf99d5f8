"""CPU: bench.py --dump-outputs writes the last timed step's results as float32 .npy files in a fixed layout, and a step that would
exceed the size limit is cut down to a fixed, seeded sample of whole frames."""
import importlib
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    return importlib.import_module("bench")


def _step(pkg, B, stereo, seed=3):
    """Host results in the shape FrontEnd.results returns them: per image (keypoints, descriptors), per frame (uright, depth, n)."""
    rng = np.random.default_rng(seed)
    imgs = []
    for _ in range(2 * B if stereo else B):
        n = int(rng.integers(5, 40))
        k = np.zeros(n, pkg.KP_DTYPE)
        for f in ("x", "y", "size", "angle", "response"):
            k[f] = rng.random(n).astype(np.float32) * 100
        k["octave"] = rng.integers(0, 8, n)
        k["class_id"] = -1
        imgs.append((k, rng.integers(0, 256, (n, 32), dtype=np.uint8)))
    frames = []
    if stereo:
        for b in range(B):
            n = len(imgs[b][0])
            frames.append((rng.random(n).astype(np.float32), rng.random(n).astype(np.float32), int(rng.integers(0, n))))
    return imgs, frames


def test_dump_layout_stereo(pkg, tmp_path):
    bench = _bench()
    B = 4
    last = _step(pkg, B, True)
    fe = types.SimpleNamespace(B=B, stereo=True)
    files = bench.dump_outputs(fe, last, str(tmp_path))
    assert files == sorted(["frames.npy", "keypoint_counts.npy", "keypoints.npy", "descriptors.npy", "mvuRight.npy", "mvDepth.npy",
                            "stereo_matches.npy"])
    d = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in files}
    assert all(a.dtype == np.float32 for a in d.values())
    imgs, st = last
    assert d["frames"].tolist() == list(range(B))
    assert d["keypoint_counts"].tolist() == [len(k) for k, _ in imgs]
    kp = np.concatenate([np.stack([k[f].astype(np.float32) for f in ("x", "y", "size", "angle", "response", "octave", "class_id")], 1)
                         for k, _ in imgs])
    assert np.array_equal(d["keypoints"], kp)
    assert np.array_equal(d["descriptors"], np.concatenate([dd for _, dd in imgs]).astype(np.float32))
    assert np.array_equal(d["mvuRight"], np.concatenate([s[0] for s in st]))
    assert np.array_equal(d["mvDepth"], np.concatenate([s[1] for s in st]))
    assert d["stereo_matches"].tolist() == [s[2] for s in st]


def test_dump_sample_under_the_limit_is_fixed(pkg, tmp_path):
    bench = _bench()
    B = 16
    last = _step(pkg, B, False)
    fe = types.SimpleNamespace(B=B, stereo=False)
    limit = 20000
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(fe, last, a, limit=limit)
    bench.dump_outputs(fe, last, b, limit=limit)
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= limit + 128 * len(os.listdir(a))          # (+ the .npy headers)
    fr = np.load(os.path.join(a, "frames.npy"))
    assert 0 < len(fr) < B and (np.diff(fr) > 0).all()
    assert np.load(os.path.join(a, "keypoint_counts.npy")).tolist() == [len(last[0][int(i)][0]) for i in fr]
    for f in os.listdir(a):
        assert np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))), f
    assert not os.path.exists(os.path.join(a, "mvuRight.npy"))


def test_bench_options():
    """--full and --dump-outputs are there; --steps 0 is refused before anything runs."""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr
