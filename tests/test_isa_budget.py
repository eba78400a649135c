"""CPU-side check of the fused conditional block's instruction budget (scripts/isa_budget.py): the benchmarked instantiation
cond_gf_split_kernel<2, false, false, 2> cross-compiled with the library's own flags.  Pins its registers (168: three workgroups per CU), no
scratch, and the weighted issue cycles of its flow phase, so that a later change cannot drift back unnoticed.  No kernel is launched."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_budget  # noqa: E402

# flow-phase weighted issue cycles (static, every branch once): 8444 before the rescale / log2(e) folds, the batched reflection norms and
# the dead log1p of the Pade tail were cut; 6716 after, pinned with 2 % room for scheduling noise
FLOW_CYCLES_MAX = 6850


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    if not os.path.exists(isa_budget.HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "cs.s")
    isa_budget.compile_asm(out)
    return isa_budget.report(open(out).read(), (2, False, False, 2))


def test_headline_kernel_registers_and_occupancy(budget):
    assert budget["vgpr"] + budget["agpr"] <= 168, budget
    assert budget["scratch"] == 0 and budget["vgpr_spill"] == 0, budget
    assert budget["waves_per_simd"] == 3, budget


def test_headline_kernel_flow_budget(budget):
    r = budget["regions"]
    assert r["matrix"]["mfma"] == 216, r                    # 3 chunks x 4 k-steps x 3 piece products x 3 tiles x 2 row groups
    assert r["flow"]["mfma"] == 0, r
    assert r["flow"]["cycles"] <= FLOW_CYCLES_MAX, r
