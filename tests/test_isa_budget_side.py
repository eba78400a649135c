"""CPU-side pin of the conditional manifold block (scripts/isa_budget_side.py) for cond_mchain_kernel<float, FFam, 256, false> -- the s2 block of
the benchmarked step, `jf_cond_f_chain_inv_f32` -- cross-compiled with the library's own flags.  No kernel is launched.
profiles/r09_side_budget.md has the parent's listing and this tree's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_budget  # noqa: E402
import isa_budget_side  # noqa: E402

# the parent: 108 VGPRs, no scratch, 4 waves per SIMD by registers (profiles/r09_side_budget.md)
PARENT_VGPRS, PARENT_WAVES = 108, 4
VALUES = isa_budget_side.HIDDEN_VALUES                 # 32 hidden values per lane and row tile (the row-tile loop is not unrolled)
# what the hidden layer holds besides tanh and the split, taken from the PARENT's listing, whose form DESIGN section 3.1 counts as 8 vector + 2
# transcendental instructions per value: region `act` (between the two products) 291 non-transcendental vector instructions = 8 x 32 + 35 of
# address arithmetic and bias reads; the whole hidden layer (staging of W1 / b1 / W2 / x included) 809 = 8 x 32 + 553; no transcendental
# outside tanh (the staging's ilogb / ldexp are integer work)
ACT_OTHER, HIDDEN_OTHER, STAGE_TRANS = 291 - 8 * 32, 809 - 8 * 32, 0
# weighted issue cycles of everything behind the second product (static: every option of the `f` layer once).  Parent 31212; FFam::apply_inv_f32
# reaches LAYERS_CYCLES; pinned with the 2 % scheduling room of the other two pins
LAYERS_PARENT = 31212
LAYERS_CYCLES = 25188
LAYERS_CYCLES_MAX = int(LAYERS_CYCLES * 1.02)


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    if not os.path.exists(isa_budget.HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "cm.s")
    isa_budget_side.compile_asm(out)
    return isa_budget_side.report(open(out).read(), ocml=False)


def test_registers_scratch_and_waves_are_not_worse_than_the_parents(budget):
    assert budget["scratch"] == 0 and budget["vgpr_spill"] == 0, budget
    assert budget["vgpr"] + budget["agpr"] <= PARENT_VGPRS, budget
    assert budget["waves_per_simd"] >= PARENT_WAVES, budget


def test_hidden_layer_takes_four_vector_and_two_transcendental_instructions_per_value(budget):
    r = budget["regions"]
    assert r["hidden"]["mfma"] == 8 + 12, r                              # one k-step of the f32 product, 4 k-steps x 3 f16 passes: loops rolled
    assert r["hidden"]["trans"] <= 2 * VALUES + STAGE_TRANS, r
    assert r["act"]["valu"] <= 4 * VALUES + ACT_OTHER, r
    assert r["hidden"]["valu"] <= 4 * VALUES + HIDDEN_OTHER, r


def test_layer_part_budget(budget):
    assert LAYERS_CYCLES_MAX < LAYERS_PARENT
    assert budget["regions"]["layers"]["cycles"] <= LAYERS_CYCLES_MAX, budget["regions"]
