"""Seeded pose-optimisation scenes: map points in front of a KITTI-00 stereo camera, their noisy observations, gross outliers,
monocular and invalid entries, and a motion-model guess next to the true pose."""
import numpy as np

import pose_ref as R

FX, FY, CX, CY, BF = 718.856, 718.856, 607.19, 185.2, 386.1448      # KITTI-00, as tests/tracking_chain.py
W, H = 1241, 376
NLEVELS, SCALE = 8, 1.2
SF = (np.float32(SCALE) ** np.arange(NLEVELS)).astype(np.float32)
INV_SIGMA2 = (np.float32(1.0) / (SF * SF)).astype(np.float32)
CAM = (FX, FY, CX, CY, BF, BF / FX)


def pose(rvec, t):
    """float64 4x4 from a rotation vector and a translation (Rodrigues)"""
    rvec = np.asarray(rvec, np.float64)
    th = np.linalg.norm(rvec)
    K = np.array([[0, -rvec[2], rvec[1]], [rvec[2], 0, -rvec[0]], [-rvec[1], rvec[0], 0]])
    Rm = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


def make(seed, n, mono=0.0, outliers=0.0, invalid=0.0, noise=0.7, rot=0.01, trans=0.15, rvec=None):
    """-> dict(obs [n] OBS_DTYPE, cam, Tcw_true float64 4x4, Tcw0 float32 4x4 (the guess), octave [n], gross [n] bool)
    rvec: the true rotation vector, instead of a small drawn one (the same numbers are drawn either way)"""
    rng = np.random.default_rng(seed)
    r0, t0 = rng.normal(0, 0.05, 3), rng.normal(0, 1.0, 3)
    Ttrue = pose(r0 if rvec is None else rvec, t0)
    z = rng.uniform(4.0, 60.0, n)
    u = rng.uniform(130, W - 30, n)                                # ur = u - bf / z stays positive down to z = 4
    v = rng.uniform(20, H - 20, n)
    Xc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], 1)
    Xw = (Xc - Ttrue[:3, 3]) @ Ttrue[:3, :3]                     # R^T (Xc - t)
    Xw = Xw.astype(np.float32)
    Xc = Xw.astype(np.float64) @ Ttrue[:3, :3].T + Ttrue[:3, 3]  # what the float map point projects to
    octave = rng.integers(0, NLEVELS, n)
    s = SF[octave].astype(np.float64) * noise
    pu = Xc[:, 0] / Xc[:, 2] * FX + CX + rng.normal(0, 1, n) * s
    pv = Xc[:, 1] / Xc[:, 2] * FY + CY + rng.normal(0, 1, n) * s
    pr = pu - BF / Xc[:, 2] + rng.normal(0, 1, n) * s
    gross = rng.random(n) < outliers
    pu = np.where(gross, pu + rng.choice([-1, 1], n) * rng.uniform(15, 80, n), pu)
    pv = np.where(gross, pv + rng.choice([-1, 1], n) * rng.uniform(15, 80, n), pv)
    obs = np.zeros(n, R.OBS_DTYPE)
    obs["valid"] = (rng.random(n) >= invalid).astype(np.int32)
    obs["u"], obs["v"] = pu, pv
    obs["ur"] = np.where(rng.random(n) < mono, -1.0, pr)
    obs["inv_sigma2"] = INV_SIGMA2[octave]
    obs["wx"], obs["wy"], obs["wz"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    d = pose(rng.normal(0, 1, 3) * rot / np.sqrt(3), rng.normal(0, 1, 3) * trans / np.sqrt(3))
    return dict(obs=obs, cam=CAM, Tcw_true=Ttrue, Tcw0=(d @ Ttrue).astype(np.float32), octave=octave, gross=gross)


# The shapes the GPU tests run (tests/test_poseopt_gpu.py), smallest where the kernel can go wrong: name -> make() arguments.
# 0 / 2: fewer than 3 correspondences; 3: the minimum; 9 / 10: the `< 10` break; 63-65: a wave's edge; 255-257: the workgroup's edge and
# the strided loop; then the mixes, each edge kind alone, invalid entries in between, and a start far enough off for a rejected trial;
# 1536 / 1537: the last edge the kernel stages in LDS (PO_LDS_EDGES) and the first it reads from memory; 2000: well past the stage.
# rot3x / y / z: a true pose turned 3 rad about one axis - the rotation's trace is negative and its largest diagonal entry is that
# axis's, the three branches of quat_from_R every other scene (a rotation of ~0.05 rad) leaves alone; both edge kinds.
CASES = {
    "n0": dict(seed=100, n=0), "n2": dict(seed=102, n=2), "n3": dict(seed=103, n=3), "n9": dict(seed=109, n=9), "n10": dict(seed=110, n=10),
    "n63": dict(seed=163, n=63, mono=0.3, outliers=0.2), "n64": dict(seed=164, n=64, mono=0.3, outliers=0.2),
    "n65": dict(seed=165, n=65, mono=0.3, outliers=0.2), "n255": dict(seed=255, n=255, mono=0.3, outliers=0.2),
    "n256": dict(seed=256, n=256, mono=0.3, outliers=0.2), "n257": dict(seed=257, n=257, mono=0.3, outliers=0.2),
    "mixed300": dict(seed=300, n=300, mono=0.3, outliers=0.25), "outliers600": dict(seed=600, n=600, outliers=0.4),
    "all_mono": dict(seed=120, n=120, mono=1.0, outliers=0.1), "all_stereo": dict(seed=121, n=120, mono=0.0, outliers=0.1),
    "invalid": dict(seed=150, n=150, mono=0.3, outliers=0.2, invalid=0.3),
    "far": dict(seed=200, n=200, mono=0.3, outliers=0.2, rot=0.2, trans=2.0),
    "n1536": dict(seed=1536, n=1536, mono=0.3, outliers=0.2, invalid=0.05), "n1537": dict(seed=1537, n=1537, mono=0.3, outliers=0.2, invalid=0.05),
    "n2000": dict(seed=2000, n=2000, mono=0.3, outliers=0.2, invalid=0.05),
    "rot3x": dict(seed=3002, n=12, mono=0.4, rvec=(3.0, 0.0, 0.0)), "rot3y": dict(seed=3103, n=12, mono=0.4, rvec=(0.0, 3.0, 0.0)),
    "rot3z": dict(seed=3202, n=12, mono=0.4, rvec=(0.0, 0.0, 3.0)),
}


def case(name):
    return make(**CASES[name])
