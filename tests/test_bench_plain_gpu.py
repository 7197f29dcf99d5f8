"""A plain `bench.py --gpus 1 --steps K --warmup W` times K steps and prints the headline line only (everything else is behind
--full); --dump-outputs writes what the last timed step computed, which is checked here against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


def test_plain_line_and_dumped_outputs(tmp_path, oracle):
    B, steps = 4, 5
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), "--steps", str(steps),
                        "--warmup", "2", "--ramp-steps", "0", "--gen-workers", "1", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, "bench.py failed (%d)\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] / 1e3 - B) < 1e-2 * B
    for k in ("cpu_baseline", "other_workloads", "roofline", "stage_ms_per_call", "long_run", "end_to_end", "tracking_front_end"):
        assert k not in out, k
    d = {f[:-4]: np.load(str(tmp_path / f)) for f in out["dumped_outputs"]["files"]}
    assert all(a.dtype == np.float32 for a in d.values())
    assert d["frames"].tolist() == list(range(B))
    cnt = d["keypoint_counts"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    ref = __import__("importlib").import_module("oracle.reference_frames")
    mbf = 386.1448
    mb = float(np.float32(mbf) / np.float32(718.856))
    for b in (0, B - 1):
        e = ref.stereo_frame((1241, 376, 1000, b, mbf, mb))
        for i, k, desc in ((b, e["kl"], e["dl"]), (B + b, e["kr"], e["dr"])):
            got = d["keypoints"][off[i]:off[i + 1]]
            assert len(got) == len(k), (b, i)
            exp = np.stack([k[f].astype(np.float32) for f in KP_FIELDS], 1)
            assert np.array_equal(np.delete(got, 3, 1), np.delete(exp, 3, 1)), (b, i)
            assert np.abs(got[:, 3] - exp[:, 3]).max(initial=0) <= 1e-4
            assert np.array_equal(d["descriptors"][off[i]:off[i + 1]], desc.astype(np.float32)), (b, i)
        assert np.array_equal(d["mvuRight"][off[b]:off[b + 1]], e["uright"]) and np.array_equal(d["mvDepth"][off[b]:off[b + 1]], e["depth"])
        assert d["stereo_matches"][b] == e["nmatch"]
