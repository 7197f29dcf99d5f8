"""GPU: the bundle adjustment's results do not depend on what fresh scratch memory held, with the fill hook of
tests/test_scratch_fill_gpu.py: every new scratch block - the staging pair's device block and its pinned mirror - filled with two
different words gives the bytes of the run without a fill.  The cases: both rounds with flagged edges and a free pose that leaves
the problem (`dead_pose`), the factorisation in device memory (`nfL+1`), the points-only limit (`nf0`), a stopped call."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_ref as R        # noqa: E402
import lba_scene as S      # noqa: E402
from test_lba_cpu import StopAt      # noqa: E402
from test_lba_gpu import as_bytes, compare      # noqa: E402
from test_scratch_fill_gpu import PAIR_BLOCKS, fill      # noqa: E402,F401   the fixture that fills every fresh scratch block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["dead_pose", "nfL+1", "nf0"])
def test_results_do_not_depend_on_fresh_scratch(pkg, fill, name):      # noqa: F811
    sc, ref, _, dev = S.reference(name)

    def run():
        res = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
        return {"bytes": dict(enumerate(as_bytes(res))), "res": res}
    fill.three(run, PAIR_BLOCKS, lambda raw: compare(name, raw["res"], ref, dev), "bundle adjustment " + name)


def test_stopped_call_does_not_depend_on_fresh_scratch(pkg, fill):      # noqa: F811
    sc, _, _, dev = S.reference("outliers")
    ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"], stop=StopAt(1))

    def run():
        res = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], stop=StopAt(1))
        return {"bytes": dict(enumerate(as_bytes(res))), "res": res}
    fill.three(run, PAIR_BLOCKS, lambda raw: compare("outliers stopped at :655", raw["res"], ref, dev), "bundle adjustment, stopped")
