"""CPU: the launch rule of an extraction call (plan_chunk, csrc/orbx_plan.h) through the developer build's orbx_debug_plan_chunk - no
HIP call, no GPU - against its independent restatement tests/launch_rule_ref.py, over every option key the rule reads, the pairs of
keys that interact, batch sizes, profiling / prefetch / sparse-hint state and synthetic geometries; and the invariants the kernels
rely on, checked again here from their statements ("The launch plan")."""
import itertools

import numpy as np
import pytest

import launch_rule_ref as ref

# legal values per option key (orbx_set_option).  Keys 0, 1 and 7 (developer build: phase stops) take any value >= 0; the rule tells
# 0 from non-zero and, for key 7, the time-stamp values 8 and 9 from the stops.
VALUES = {0: (0, 1, 2), 1: (0, 1, 2), 4: range(4), 6: range(4), 7: (0, 1, 2, 8, 9), 8: range(5), 10: range(4), 11: range(3), 12: range(2),
          15: range(17), 16: range(3), 18: range(2), 19: range(17), 20: range(3), 21: (0, 1, 40), 23: range(2), 26: range(2)}
PAIRS = [(4, 23), (4, 18), (6, 23), (6, 19), (15, 19), (16, 20), (26, 23)]
# in a pair the level keys 15 and 19 take the values the rule can tell apart with at most 8 levels: off, below 2, the smallest, nl - 1, nl, the maximum
PAIR_VALUES = {**VALUES, 15: (0, 1, 2, 7, 8, 16), 19: (0, 1, 2, 7, 8, 16)}
BATCHES = (1, 2, 4, 5, 8, 32, 64, 128)
# ncells per level: both sides of 600 and of 1600 in one geometry
NCELLS = (2000, 1600, 1599, 700, 600, 599, 100, 20)


def _option_settings():
    out = [{}]
    for k, vals in VALUES.items():
        out += [{k: v} for v in vals if v]
    for a, b in PAIRS:
        out += [{a: va, b: vb} for va in PAIR_VALUES[a] for vb in PAIR_VALUES[b] if va and vb]
    return out


def _geometries():
    for nl, bigmask in itertools.product((2, 3, 8), (0, 0b11)):
        full = (1 << nl) - 1
        yield dict(nl=nl, totalStrips=0, stripLevels=0, octBigMask=bigmask)
        for ts, sl in itertools.product((31, 64, 2000), (full, full >> 2)):      # (31 x 128 = 3968, 64 x 64 = 4096)
            yield dict(nl=nl, totalStrips=ts, stripLevels=sl, octBigMask=bigmask)


def _extra(opt):
    """State that only some keys look at, on top of the usual values: crossed with batch size and geometry for the settings that touch it."""
    usual = dict(pfUsed=0, evPyrDone=0, dbgBlur=0, sliceScratch=1, fastTileStride=48, fastScoreStride=40)
    ex = []
    if 10 in opt:
        ex += [dict(usual, pfUsed=1, evPyrDone=e) for e in (0, 1)]
    if 15 in opt or 19 in opt:
        ex.append(dict(usual, dbgBlur=1))
    if 26 in opt:
        ex.append(dict(usual, sliceScratch=0))
    if 6 in opt or not opt:
        ex += [dict(usual, fastTileStride=t, fastScoreStride=s) for t, s in ((44, 36), (52, 44), (60, 52), (48, 48))]
    return usual, ex


def _check_invariants(p, i, opt):
    """Section 2 of the launch plan's contract, from its statements (not from orbx_plan.h)."""
    B, nl = i["B"], i["nl"]
    assert p["gather"] == (not p["fused"])
    if p["multiWg"]:
        assert not p["fused"] and p["gather"]
    if p["bigMask"]:
        assert p["multiWg"]
    if p["histOct"]:
        assert p["fused"] and not p["strips"] and B <= 4 and i["lastChunks"] == 1 and not p["multiWg"]
    if p["earlyLv"] > 0:
        m = (1 << p["earlyLv"]) - 1
        assert p["fused"] and p["strips"] and not p["compact"] and p["aSplit"] == 0 and not i["prof"] and p["stripLevels"] & m == m
    if p["aSplit"] > 0:
        assert p["usePyr"] and not p["multiWg"] and nl >= 3 and 0 < p["aSplit"] < nl
    if p["sweepShared"] or p["sweepSlices"]:
        assert p["fused"] and not p["histOct"] and i["sliceScratch"]
    assert p["octForm"] in (ref.OCT_EXACT, ref.OCT_BIG, ref.OCT_EARLY, ref.OCT_SPLIT, ref.OCT_SINGLE)     # exactly one form
    if p["octForm"] == ref.OCT_BIG:
        assert opt.get(1, 0) == 0 and opt.get(7, 0) == 0 and p["multiWg"] and p["gather"]
    assert (p["octForm"] == ref.OCT_EXACT) == (not p["usePyr"])
    assert (p["octForm"] == ref.OCT_EARLY) == (p["earlyLv"] > 0)
    assert (p["octForm"] == ref.OCT_SPLIT) == (p["aSplit"] > 0)
    if not p["fused"]:
        assert p["sparseHint"] != ref.HINT_OCT_SRC
    else:
        assert p["sparseHint"] != ref.HINT_GATHER


@pytest.fixture(scope="module")
def rule(pkg):
    """(PlanInput fields by name, {option: value}) -> (status, ChunkPlan as a flat tuple) through orbx_debug_plan_chunk."""
    __import__("importlib").import_module("orb_slam2v2-1_amd.build").build()
    assert ref.FIELDS == pkg.CHUNK_PLAN_FIELDS and NAMES == pkg.PLAN_INPUT_FIELDS
    a, out = np.zeros(NS + 16 + 32, np.int32), np.zeros(len(ref.FIELDS) + 16, np.int32)
    fn, pa, po = pkg.lib(True).orbx_debug_plan_chunk, a.ctypes.data, out.ctypes.data

    def run(fields, opt):
        a[:] = [fields.get(n, 0) for n in NAMES] + CELLS[fields["nl"]] + (opt if isinstance(opt, list) else ref.option_list(opt))
        rc = fn(pa, len(a), po, len(out))
        return rc, tuple(out.tolist())
    return run


NAMES = ["B", "nl", "totalStrips", "stripLevels", "octBigMask", "lastChunks", "prof", "profFast", "skipPyr", "pfUsed", "evPyrDone", "dbgBlur",
         "sliceScratch", "fastTileStride", "fastScoreStride", "sparseRecent"]
NS = len(NAMES)
CELLS = {nl: list(NCELLS[:nl]) + [0] * (16 - nl) for nl in (2, 3, 8)}


def test_plan_equals_the_restatement_and_keeps_the_invariants(pkg, rule):
    plans, forms, fast, checked, ncase = set(), set(), set(), set(), 0
    geoms = list(_geometries())
    for opt in _option_settings():
        usual, extra = _extra(opt)
        o = ref.option_list(opt)
        cases = itertools.chain(itertools.product([usual], geoms, BATCHES, (0, 1), (0, 1), (0, 1)),
                                itertools.product(extra, geoms, BATCHES, (0,), (0,), (0,)))
        for ex, g, B, prof, skip, recent in cases:
            nch = ref.chunk_count(B, prof, skip, opt)
            i = dict(ex, **g, B=B // nch, lastChunks=nch, prof=prof, profFast=prof, skipPyr=skip, sparseRecent=recent)
            rc, got = rule(i, o)
            want = ref.plan(ncells=NCELLS, opt=o, **i)
            assert rc == pkg.ORBX_OK, (i, opt, pkg.lib(True).orbx_last_error())
            assert got == want, (i, opt, {k: (v, ref.as_dict(want)[k]) for k, v in ref.as_dict(got).items() if v != ref.as_dict(want)[k]})
            key = (got, i["B"], i["nl"], nch, prof, i["sliceScratch"], o[1], o[7])     # everything the invariants read
            if key not in checked:
                checked.add(key)
                _check_invariants(ref.as_dict(got), i, opt)
            ncase += 1
    for t in checked:
        p = ref.as_dict(t[0])
        plans.add(t[0])
        forms.add(p["octForm"])
        fast.add((p["strips"], p["fastCells"]))
    print("launch plan sweep: %d cases, %d distinct plans" % (ncase, len(plans)))
    assert forms == {ref.OCT_EXACT, ref.OCT_BIG, ref.OCT_EARLY, ref.OCT_SPLIT, ref.OCT_SINGLE}
    assert {(1, 0), (0, 1), (1, 1)} <= fast          # strips alone, cells alone, both
    assert len(plans) > 100


def test_profiling_of_the_fast_stage_alone(pkg, rule):
    """orbx_set_profiling 2 / 3: events around the FAST stage only (profFast without prof) - the ordering kernel's condition."""
    for skip, o12 in itertools.product((0, 1), (0, 1)):
        i = dict(B=8, nl=8, totalStrips=2000, stripLevels=255, octBigMask=0, lastChunks=1, prof=0, profFast=1, skipPyr=skip, sliceScratch=1,
                 fastTileStride=48, fastScoreStride=40)
        rc, got = rule(i, {12: o12})
        assert rc == pkg.ORBX_OK and got == ref.plan(ncells=NCELLS, opt={12: o12}, **i)
        assert ref.as_dict(got)["orderKernel"] == (skip and not o12)


def test_single_image_with_large_levels_takes_the_histogram_form(pkg, rule):
    """The configuration of the one GPU memory fault this project has had (HISTORY.md): B = 1, an image with large levels
    (octBigMask != 0), every option at its default.  The FAST stage histograms for the quad-tree, no k_gather runs, so nothing may
    choose the multi-workgroup form, which sweeps the compacted keys k_gather writes."""
    i = dict(B=1, nl=8, totalStrips=2000, stripLevels=255, octBigMask=0b1111, lastChunks=1, sliceScratch=1, fastTileStride=48, fastScoreStride=40)
    rc, p = rule(i, {})
    assert rc == pkg.ORBX_OK
    p = ref.as_dict(p)
    assert p["histOct"] and p["fused"] and not p["multiWg"] and p["bigMask"] == 0 and not p["gather"] and p["octForm"] == ref.OCT_SINGLE


def test_hook_refuses_bad_arguments(pkg, rule):
    L = pkg.lib(True)
    a, out = np.zeros(64, np.int32), np.zeros(43, np.int32)
    assert L.orbx_debug_plan_chunk(a.ctypes.data, 63, out.ctypes.data, 43) == pkg.ORBX_ERR_ARG
    assert L.orbx_debug_plan_chunk(a.ctypes.data, 64, out.ctypes.data, 43) == pkg.ORBX_ERR_ARG      # B = 0, nl = 0
    rc, p = pkg.debug_plan_chunk(B=1, nl=8, lastChunks=1, ncells=NCELLS)
    assert rc == pkg.ORBX_OK and p["histOct"] and p == ref.as_dict(ref.plan(B=1, nl=8, totalStrips=0, stripLevels=0, octBigMask=0, lastChunks=1, ncells=NCELLS))
