"""CPU-side pin of phase 1 of the fused conditional block (scripts/isa_budget.py, region "phase1": everything in front of the layer loop --
input staging, the K1 -> 128 layer, tanh, the f16 split) for the benchmarked instantiation cond_gf_split_kernel<2, false, false, 2>,
cross-compiled with the library's own flags.  No kernel is launched."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_budget  # noqa: E402

# weighted issue cycles of phase 1 (static: both sides of every branch, loop bodies once).  8248 with element-wise staging (an index division
# and a segment search per element, sine and cosine of both angles for every column), zeroed accumulators with the bias added behind them, a
# rolled k-step loop and 8 vector instructions per tanh + split.  Row-wise staging, bias-started accumulators, unrolled k-steps and 4
# instructions per tanh + split reach PHASE1_CYCLES; pinned with 2 % room for scheduling noise, as the flow pin is.
# The gate is 60 % of 8248: the floor is ~3100-3500 (64 values x (2 transcendentals x 8 + 4 x 4), ~270 of staging, the f32 MFMAs, address
# set-up).
PHASE1_PARENT = 8248
PHASE1_GATE = 4950
PHASE1_CYCLES = 3604
PHASE1_CYCLES_MAX = int(PHASE1_CYCLES * 1.02)
# the compiler lays k-steps 2 .. 6 of the unrolled K1 -> 128 product (not run at K1 <= 8) out BEHIND the layer loop, where the script's
# text-order regions count them as "tail": phase 1 and tail together are held as well, so that work cannot leave the pin by moving there
# (parent: 8248 + 604 = 8852)
PHASE1_AND_TAIL_MAX = int((3604 + 1228) * 1.02)


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    if not os.path.exists(isa_budget.HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "cs.s")
    isa_budget.compile_asm(out)
    return isa_budget.report(open(out).read(), (2, False, False, 2))


def test_phase1_budget(budget):
    r = budget["regions"]
    assert PHASE1_CYCLES_MAX <= PHASE1_GATE
    assert r["phase1"]["cycles"] <= PHASE1_CYCLES_MAX, r
    assert r["phase1"]["cycles"] + r["tail"]["cycles"] <= PHASE1_AND_TAIL_MAX, r
    assert PHASE1_AND_TAIL_MAX - 604 <= PHASE1_GATE                # the parent's tail (epilogue only) taken off: still inside the gate


def test_phase1_tanh_and_split_take_four_vector_instructions_per_value(budget):
    # 64 hidden values per lane (2 row groups x 32): v_exp + v_rcp each, and add, fma, half a v_cvt_pk twice, v_fma_mix.  The staging and
    # the embedding add 16 transcendentals (v_sin / v_cos of two angles for each of at most four segments)
    r = budget["regions"]["phase1"]
    assert r["trans"] <= 2 * 64 + 16, r
