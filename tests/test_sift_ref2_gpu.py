"""Context.sift_extract (sift.hip) held directly to the independent float64 restatement tests/ref2/sift_ref2.py, on the
images and with the limits of tests/test_sift_ref2_cpu.py (tests/ref2/sift_deviation_budget.json, measured with the
CPU reference as the candidate, never with this output).  test_sift_gpu.py holds the kernels to sift_ref.cc bit for
bit; this file keeps them pinned to SIFT even if sift_ref.cc and sift.hip are edited together."""
import pytest

from ref2 import sift_compare as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", sc.FAST)
def test_gpu_within_the_budget(amc_ctx, tag):
    name, opts = sc.CASES[tag]
    got, _ = amc_ctx.sift_extract(sc.image(name), **opts)
    sc.check_against_budget(tag, got)
