"""CPU-side pin of the row reductions in the layer loop of the fused conditional block (scripts/isa_budget.py, regions "matrix" + "flow") for
the benchmarked instantiation cond_gf_split_kernel<2, false, false, 2>, cross-compiled with the library's own flags.  No kernel is launched.

A row's four coordinate lanes are reduced with v_permlane16_swap / v_permlane32_swap (csrc/jf_cond_split.h).  With one cs_rsum per row group
and value the layer loop held 18 + 14 of them: two batched norm reductions (cs_rsum4: 4 + 2 each) and 2 x (4 reflections + 1 log-det sum)
single sums (1 + 1 each).  Paired across the wave's two row groups (cs_rsum2: 2 + 1 for two sums) the ten single sums become five pairs:
2 x (4 + 2) + 5 x (2 + 1) = 18 + 9."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_budget  # noqa: E402

SWAP16_MAX, SWAP32_MAX = 18, 9
# flow-phase weighted issue cycles (static, every branch once): 6716 with one reduction per row group, 6680 on the listing with the paired
# ones.  (The matrix region went from 2136 to 1916 beside it: the chunk DMA's LDS addresses became scalar.)
FLOW_CYCLES_PARENT = 6716
FLOW_CYCLES_MAX = 6680


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    if not os.path.exists(isa_budget.HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "cs.s")
    isa_budget.compile_asm(out)
    return isa_budget.report(open(out).read(), (2, False, False, 2))


def test_layer_loop_swaps(budget):
    r = budget["regions"]
    assert r["matrix"]["swap32"] + r["flow"]["swap32"] <= SWAP32_MAX, r
    assert r["matrix"]["swap16"] + r["flow"]["swap16"] <= SWAP16_MAX, r


def test_flow_cycles_below_the_unpaired_listing(budget):
    assert FLOW_CYCLES_MAX < FLOW_CYCLES_PARENT
    assert budget["regions"]["flow"]["cycles"] <= FLOW_CYCLES_MAX, budget["regions"]
