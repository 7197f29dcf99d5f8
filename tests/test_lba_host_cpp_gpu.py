"""GPU: ORB_SLAM2::Optimizer::LocalBundleAdjustment and GlobalBundleAdjustemnt (orb_slam2v2-1_amd/host/Optimizer.h) through
tests/cpp/lba_driver.cc on shim KeyFrames and MapPoints built from a scene file.  The class builds the three lists of
src/Optimizer.cc:455-504 itself; the test builds the same flat problem in Python, calls local_bundle_adjustment and expects the
class to leave exactly that: the poses of the local keyframes and the positions of the local points bit for bit, the matches and
observations erased where the call flags them (a point left with two observations or fewer goes bad and loses all its matches),
the mnBALocalForKF / mnBAFixedForKF marks, and UpdateNormalAndDepth applied to every local point that is not bad."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")
f32 = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "lba_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "lba_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def hx(x):
    return float(x).hex()


class World:
    """the keyframes and points of a scene as the driver holds them: keyframe k of the FILE is scene keyframe order[k]"""

    def __init__(self, sc, order, ids, ncov):
        self.sc, self.order, self.ids, self.ncov = sc, list(order), list(ids), ncov
        obs = sc["obs"]
        self.octave = np.array([int(np.nonzero(S.INV_SIGMA2 == v)[0][0]) for v in obs["inv_sigma2"]])
        pos = {k: i for i, k in enumerate(self.order)}
        self.feat = [[] for _ in self.order]          # per file keyframe: the scene observations that are its features, in order
        for e in range(len(obs)):
            self.feat[pos[int(obs["kf"][e])]].append(e)
        self.P = len(sc["pts"])

    def write(self, path, mode, stop):
        sc, obs = self.sc, self.sc["obs"]
        lines = ["%d %d %d %d %d %s" % (mode, stop, len(self.order), self.P, self.ncov, " ".join(str(i) for i in range(1, 1 + self.ncov))),
                 "%d %s %s" % (S.NLEVELS, " ".join(hx(x) for x in S.SF), " ".join(hx(x) for x in S.INV_SIGMA2))]
        for k, sk in enumerate(self.order):
            kf = sc["kfs"][sk]
            lines.append("%d 0 %s" % (self.ids[k], " ".join(hx(kf[f]) for f in ("fx", "fy", "cx", "cy", "bf"))))
            lines.append(" ".join(hx(x) for x in kf["Tcw"]))
            lines.append(str(len(self.feat[k])))
            for e in self.feat[k]:
                lines.append("%s %s %d %s %d" % (hx(obs["u"][e]), hx(obs["v"][e]), self.octave[e], hx(obs["ur"][e]), obs["pt"][e]))
        for p in sc["pts"]:
            lines.append("%s %s %s 0" % (hx(p["x"]), hx(p["y"]), hx(p["z"])))
        path.write_text("\n".join(lines) + "\n")

    def flat_local(self, pkg):
        """the problem Optimizer::LocalBundleAdjustment hands to the C ABI -> (kfs, pts, obs, file keyframe of each flat keyframe, scene
        point of each flat point, (file keyframe, feature) of each flat observation, the local file keyframes)"""
        sc, obs = self.sc, self.sc["obs"]
        local = list(range(0, 1 + self.ncov))
        lpts = []
        for k in local:
            for e in self.feat[k]:
                if int(obs["pt"][e]) not in lpts:
                    lpts.append(int(obs["pt"][e]))
        observers = {p: [] for p in lpts}
        for k in range(len(self.order)):                  # a map<KeyFrame *, size_t> walks the keyframes in address order: the file's
            for i, e in enumerate(self.feat[k]):
                if int(obs["pt"][e]) in observers:
                    observers[int(obs["pt"][e])].append((k, i, e))
        fixed = []
        for p in lpts:
            for k, _, _ in observers[p]:
                if k not in local and k not in fixed:
                    fixed.append(k)
        fk = local + fixed
        kfs = np.zeros(len(fk), pkg.LBA_KEYFRAME_DTYPE)
        for j, k in enumerate(fk):
            kfs[j] = sc["kfs"][self.order[k]]
            kfs["fixed"][j] = 1 if (k in fixed or self.ids[k] == 0) else 0
        pts = sc["pts"][lpts]
        rows, where = [], []
        for j, p in enumerate(lpts):
            for k, i, e in observers[p]:
                rows.append((fk.index(k), j, obs["u"][e], obs["v"][e], obs["ur"][e] if obs["ur"][e] >= 0 else -1.0, obs["inv_sigma2"][e]))
                where.append((k, i))
        return kfs, pts, np.array(rows, pkg.LBA_OBSERVATION_DTYPE), fk, lpts, where, local, fixed


def camera_centre(T):
    """KeyFrame::SetPose on the shim: Ow = -Rwc * tcw as one gemm with alpha = -1"""
    T = np.asarray(T, f32).reshape(4, 4)
    return np.array([f32((np.float64(T[0, i]) * np.float64(T[0, 3]) + np.float64(T[1, i]) * np.float64(T[1, 3]) + np.float64(T[2, i]) * np.float64(T[2, 3])) * -1.0)
                     for i in range(3)], f32)


def normal_and_depth(pos, centres, ref_centre, ref_level):
    """MapPoint::UpdateNormalAndDepth on the shim -> (min, max, normal)"""
    normal = np.zeros(3, f32)
    for Ow in centres:
        ni = (pos - Ow).astype(f32)
        inv = f32(1.0 / np.sqrt(np.sum(ni.astype(np.float64) ** 2 * 1.0)))
        normal = (ni * inv + normal).astype(f32)
    d = (pos - ref_centre).astype(f32)
    dist = f32(np.sqrt(np.sum(d.astype(np.float64) ** 2)))
    mx = f32(dist * S.SF[ref_level])
    mn = f32(mx / S.SF[S.NLEVELS - 1])
    return mn, mx, (normal.astype(np.float64) * (1.0 / len(centres))).astype(f32)


def run(driver, tmp_path, world, mode, stop):
    world.write(tmp_path / "scene.txt", mode, stop)
    out = subprocess.run([driver, str(tmp_path / "scene.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    kf, pt = [], []
    for ln in out.stdout.strip().split("\n"):
        w = ln.split()
        if w[0] == "kf":
            kf.append((int(w[1]), int(w[2]), np.array([float.fromhex(x) for x in w[3:19]], f32), [int(x) for x in w[19:]]))
        else:
            pt.append((np.array([float.fromhex(x) for x in w[1:4]], f32), int(w[4]), int(w[5]), int(w[6]), f32(float.fromhex(w[7])), f32(float.fromhex(w[8])),
                       np.array([float.fromhex(x) for x in w[9:12]], f32)))
    return kf, pt


@pytest.mark.parametrize("name", ["outliers", "id0"])
def test_local_bundle_adjustment_class_on_shim_keyframes(pkg, driver, tmp_path, name):
    sc = S.case(name)
    K = len(sc["kfs"])
    nlocal = int((sc["kfs"]["fixed"] == 0).sum()) + (1 if name == "id0" else 0)
    if name == "id0":      # keyframe 0 of the map is a covisible neighbour of the current keyframe, not the current one
        order, ids = [1, 0] + list(range(2, K)), [2, 0] + list(range(3, K + 1))
    else:
        order, ids = list(range(K)), list(range(1, K + 1))
    world = World(sc, order, ids, nlocal - 1)
    kfs, pts, obs, fk, lpts, where, local, fixed = world.flat_local(pkg)
    assert len(fk) == K and len(fixed) == K - nlocal and len(lpts) > 40 and (kfs["fixed"][:nlocal] == [int(i == 0) for i in np.array(ids)[local]]).all()
    T, X, erase, info, _, _ = pkg.local_bundle_adjustment(kfs, pts, obs)
    assert info["rounds"] == 2 and (erase.any() or name == "id0")
    got_kf, got_pt = run(driver, tmp_path, world, 0, 0)
    cur = ids[0]
    # the expected state: matches and observations erased, points with two observations or fewer bad
    match = [[int(sc["obs"]["pt"][e]) for e in world.feat[k]] for k in range(K)]
    observers = {p: {} for p in range(world.P)}
    for k in range(K):
        for i, p in enumerate(match[k]):
            observers[p][k] = i
    nobs = {p: sum(2 if sc["obs"]["ur"][world.feat[k][i]] >= 0 else 1 for k, i in observers[p].items()) for p in observers}
    ref = {p: (min(observers[p]) if observers[p] else -1) for p in observers}
    bad = set()
    for j in np.nonzero(erase)[0]:
        k, i = where[j]
        p = int(obs["pt"][j]); p = lpts[p]
        if p in bad or k not in observers[p]:
            continue
        match[k][i] = -1
        nobs[p] -= 2 if sc["obs"]["ur"][world.feat[k][i]] >= 0 else 1
        del observers[p][k]
        if ref[p] == k:
            ref[p] = min(observers[p]) if observers[p] else -1
        if nobs[p] <= 2:
            bad.add(p)
            for k2, i2 in observers[p].items():
                match[k2][i2] = -1
            observers[p] = {}
    poses = {k: sc["kfs"]["Tcw"][order[k]] for k in range(K)}
    for j, k in enumerate(fk):
        if k in local:
            poses[k] = T[j].reshape(16)
    for k in range(K):
        la, fa, pose, mp = got_kf[k]
        assert (la, fa) == ((cur, 0) if k in local else (0, cur)), k
        assert pose.tobytes() == np.asarray(poses[k], f32).tobytes(), k
        assert mp == match[k], k
    fixed_id0 = [k for k in local if ids[k] == 0]
    for k in fixed_id0:      # byte for byte
        assert got_kf[k][2].tobytes() == sc["kfs"]["Tcw"][order[k]].tobytes()
    assert (name == "id0") == bool(fixed_id0)
    centres = {k: camera_centre(poses[k]) for k in range(K)}
    checked = 0
    for p in range(world.P):
        pos, isbad, n, r, mn, mx, normal = got_pt[p]
        if p in lpts:
            assert pos.tobytes() == X[lpts.index(p)].tobytes(), p
        assert (isbad, n, r) == (int(p in bad), len(observers[p]), ref[p] if p not in bad else r), p
        if p in lpts and p not in bad:
            ks = sorted(observers[p])
            emn, emx, en = normal_and_depth(pos, [centres[k] for k in ks], centres[ref[p]], int(world.octave[world.feat[ref[p]][observers[p][ref[p]]]]))
            assert (mn, mx) == (emn, emx) and np.abs(normal - en).max() <= 1e-6 and np.linalg.norm(normal) > 0.5, p
            checked += 1
    assert checked > 40 and (bad or name == "id0")


def test_stop_flag_set_on_entry_writes_nothing(pkg, driver, tmp_path):
    sc = S.case("outliers")
    K = len(sc["kfs"])
    world = World(sc, list(range(K)), list(range(1, K + 1)), int((sc["kfs"]["fixed"] == 0).sum()) - 1)
    got_kf, got_pt = run(driver, tmp_path, world, 0, 1)
    for k in range(K):
        assert got_kf[k][2].tobytes() == sc["kfs"]["Tcw"][k].tobytes() and -1 not in got_kf[k][3]
    for p in range(world.P):
        assert got_pt[p][0].tobytes() == np.array([sc["pts"][p][f] for f in ("x", "y", "z")], f32).tobytes() and got_pt[p][4] == 0      # no UpdateNormalAndDepth


def test_global_bundle_adjustment_class_on_an_initial_map(pkg, driver, tmp_path):
    """GlobalBundleAdjustemnt(mpMap, 20) on two keyframes, the first with mnId == 0: the poses and points of bundle_adjustment"""
    sc = dict(S.initial_map())
    sc["obs"] = sc["obs"][~np.isin(sc["obs"]["pt"], [3, 7])]      # two points without an observation: not part of the problem (:175-179)
    world = World(sc, [0, 1], [0, 1], 0)
    got_kf, got_pt = run(driver, tmp_path, world, 1, 0)
    seen = sorted(set(int(p) for p in sc["obs"]["pt"]))
    remap = {p: j for j, p in enumerate(seen)}
    obs = sc["obs"].copy()
    order = np.lexsort((obs["kf"], obs["pt"]))      # per point, its observations in keyframe order
    obs = obs[order]
    obs["pt"] = [remap[int(p)] for p in obs["pt"]]
    T, X, _, info, _, _ = pkg.bundle_adjustment(sc["kfs"], sc["pts"][seen], obs, iterations=20, robust=True)
    assert info["rounds"] == 1 and info["free_poses"] == [1, 0] and len(seen) < world.P
    assert got_kf[0][2].tobytes() == sc["kfs"]["Tcw"][0].tobytes() and got_kf[1][2].tobytes() == T[1].tobytes()
    for p in range(world.P):
        want = X[remap[p]] if p in remap else np.array([sc["pts"][p][f] for f in ("x", "y", "z")], f32)
        assert got_pt[p][0].tobytes() == want.tobytes(), p
        assert (got_pt[p][5] > 0) == (p in remap)      # UpdateNormalAndDepth ran for the points of the problem only
