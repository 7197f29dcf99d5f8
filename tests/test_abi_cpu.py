"""CPU: the C-ABI library loads, exports every symbol include/orbx.h declares, and fails
LOUDLY (never falls back to a CPU path) when no GPU is usable."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header="orbx.h"):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(orb[xmv]_[a-z0-9_]+)\s*\(", txt)))


# the developer build's hooks: the stage hooks of the extractor / area query, then the matchers' path hooks (which resolver, LDS plan,
# fall-back or stereo form a call took), the extractor's launch plan and what an image size decides (tests/test_size_plan_cpu.py)
STAGE_HOOKS = ["orbm_debug_features_in_area", "orbx_debug_blur_patches", "orbx_debug_blurred_level", "orbx_debug_level_points",
               "orbx_debug_octree_fallbacks", "orbx_debug_sincosf"]
PATH_HOOKS = ["orbm_debug_match_path", "orbm_debug_resolve_plan", "orbm_debug_stereo_path", "orbx_debug_plan_chunk", "orbx_debug_last_plan",
              "orbx_debug_size_plan"]
# the calling thread's matcher scratch (tests/test_thread_scratch_cpu.py, tests/test_match_threads_gpu.py)
SCRATCH_HOOKS = ["orbm_debug_thread_scratch"]
# fill every fresh scratch block with a word (tests/test_scratch_fill_gpu.py)
FILL_HOOKS = ["orbx_debug_set_alloc_fill", "orbx_debug_alloc_fill_stats"]
# hold one stream back, name the streams a call uses (tests/stream_stall.py, tests/test_stream_order_gpu.py)
STALL_HOOKS = ["orbx_debug_stall_stream", "orbx_debug_streams"]


def test_library_exports_every_declared_symbol_and_hook(pkg):
    b = __import__("importlib").import_module("orb_slam2v2-1_amd.build")
    b.build()
    L = pkg.lib()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), "missing export %s" % n
    assert sorted(pkg.EXPORTS) == names, "EXPORTS list and include/orbx.h disagree"
    # the test hooks are NOT product surface: no *_debug_* symbol in the product library (nm -D), all of them - and everything else - in
    # the developer build, declared in include/orbx_dev.h
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "debug" not in nm, [l for l in nm.splitlines() if "debug" in l]
    D = pkg.lib(developer=True)
    dev = sorted(set(_declared("orbx_dev.h")) - set(names))
    assert dev == sorted(pkg.DEV_EXPORTS) == sorted(STAGE_HOOKS + PATH_HOOKS + SCRATCH_HOOKS + FILL_HOOKS + STALL_HOOKS) and len(dev) == 17
    for n in names + dev:
        assert hasattr(D, n), "developer build: missing export %s" % n


def test_keypoint_struct_is_28_bytes(pkg):
    assert pkg.KP_DTYPE.itemsize == 28 and pkg.MP_DTYPE.itemsize == 28 and pkg.LASTPT_DTYPE.itemsize == 28


def test_hamming_is_host_side(pkg):
    z = np.zeros(32, np.uint8)
    assert pkg.ORBmatcher.DescriptorDistance(z, ~z) == 256
    assert pkg.lib().orbm_hamming(None, None) == pkg.ORBX_ERR_ARG
    assert pkg.ORBmatcher.TH_LOW == 50 and pkg.ORBmatcher.TH_HIGH == 100 and pkg.ORBmatcher.HISTO_LENGTH == 30


def test_no_gpu_fails_loudly(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(pkg.OrbxError) as e:
        pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
    m = pkg.ORBmatcher(0.9, True)
    k = np.zeros(4, pkg.KP_DTYPE)
    with pytest.raises(pkg.OrbxError):
        m.SearchForInitialization(k, np.zeros((4, 32), np.uint8), k, np.zeros((4, 32), np.uint8),
                                  pkg.grid_geom(640, 480), np.zeros((4, 2), np.float32), 100)


def test_argument_errors(pkg):
    L = pkg.lib()
    h = C.c_void_p()
    assert L.orbx_create(0, 1.2, 8, 20, 7, 0, C.byref(h)) == pkg.ORBX_ERR_ARG
    assert L.orbx_create(1000, 1.0, 8, 20, 7, 0, C.byref(h)) == pkg.ORBX_ERR_ARG
    assert L.orbx_create(1000, 1.2, 99, 20, 7, 0, C.byref(h)) == pkg.ORBX_ERR_ARG
    assert L.orbx_create(1000, 1.2, 8, 20, 7, 0, None) == pkg.ORBX_ERR_ARG
    assert b"bad" in L.orbx_last_error() or b"NULL" in L.orbx_last_error()
    assert L.orbx_destroy(None) == 0


def test_product_never_imports_oracle():
    """The product path must not route through the oracle (or any CPU fallback)."""
    pk = os.path.join(ROOT, "orb_slam2v2-1_amd")
    for dirpath, _, files in os.walk(pk):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cc", ".cpp", ".hpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                code = "\n".join(l for l in txt.splitlines() if not l.strip().startswith(("#", "//", "*", "/*", '"""')))
                assert "import oracle" not in code and "from oracle" not in code and "orb_oracle" not in code, \
                    "%s references the oracle" % f


def test_predict_scale_threshold_table(oracle):
    """orbm_predict_scale_thresholds (host code of the library): level = #thresholds <= ratio reproduces
    MapPoint::PredictScale (src/MapPoint.cc:414-429, ceil(logf(ratio)/logf(sf))) for random ratios and for
    every float within a few ulps of each level boundary."""
    import importlib
    pkg = importlib.import_module("orb_slam2v2-1_amd")
    L = oracle.lib()
    for sf, nl in ((1.2, 8), (1.1, 12), (1.5, 4), (2.0, 3)):
        log_sf = np.float32(np.log(np.float32(sf)))
        thr = pkg.predict_scale_thresholds(log_sf, nl)
        assert len(thr) == nl - 1 and (np.diff(thr) > 0).all()
        rng = np.random.default_rng(7)
        ratios = list(np.exp(rng.uniform(-2, 5, 20000)).astype(np.float32))
        for t in thr:
            b = int(np.float32(t).view(np.uint32))
            ratios += [np.array([b + d], np.uint32).view(np.float32)[0] for d in range(-6, 7)]
        ratios += [np.float32(0.0), np.float32(1.0), np.float32(1e-30), np.float32(3e38)]
        for r in ratios:
            expect = L.oracle_predict_scale_ratio(float(r), float(log_sf), nl)
            got = int((np.float32(r) >= thr).sum())
            assert got == expect, (sf, float(r))


def test_default_build_has_no_process_global_switch(pkg):
    """no global mutable state.  The library exports no orbx_debug_* setter; kernel selection is per handle
    (orbx_set_option), the matchers' one option per thread (orbm_set_thread_option), and phase-stop keys need -DORBX_DEVELOPER."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    syms = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert "orbx_set_option" in syms and "orbm_set_thread_option" in syms
    assert not [s for s in syms if s.startswith("orbx_debug_set") or s == "g_debug"], syms
    assert "ORBX_BENCH_KNOBS" not in open(os.path.join(ROOT, "bench.py")).read()
