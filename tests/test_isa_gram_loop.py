"""tools/isa_point_census.py on the assembly the library in this tree was built from: the Gram's observation-tile loop of the
production instantiation of the wave kernel, letkf_wave_kernel<50, 11, false, 1, 0>, must not grow back what r13 took out of it
(csrc/letkf_wave_dev.h TRIM, DESIGN.md 4.1, profiles/r13_README.md) -- the selects on the staged weights of a step past the end,
the per-lane clamp of the chunk index, the per-step mask of the narrow member block and the 64-bit address add per row load.
Before r13 the loop's span held 95 vector instructions and 23 v_cndmask_b32 per 12 matrix instructions; r13 reached 52 and none.
(The span is the census's: hipcc lays the third step of the three in flight out behind the loop's backward branch, in both
builds, so the span holds two steps' matrix instructions.  With that block the iteration went from 122 vector instructions per
18 matrix instructions to 73.)"""
import glob
import os
import sys

import pytest

from __graft_entry__ import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_point_census

VALU_PER_12_BEFORE = 95
VALU_PER_12_REACHED = 52


@pytest.fixture(scope="module")
def loop():
    units = glob.glob(os.path.join(ROOT, "scale-letkf_amd", "lib", "obj", "letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not units:                                                       # (the GPU box receives the library, not its objects)
        pytest.skip("no device assembly beside the objects (built elsewhere)")
    c = isa_point_census.census(units[0])
    assert c["gram_tile_loop"] is not None and c["gram_tile_loop"]["mfma"] > 0, c["spans"]
    return c["gram_tile_loop"]


def test_no_lane_reads_in_the_tile_loop(loop):
    assert loop["v_readlane_b32"] == 0, loop


def test_no_selects_in_the_tile_loop(loop):
    assert loop["v_cndmask_b32"] == 0, loop


def test_vector_instructions_per_matrix_instruction(loop):
    valu, mfma = loop["valu"], loop["mfma"]
    print(f"gram_tile_loop: {valu} vector instructions per {mfma} matrix instructions = {12.0 * valu / mfma:.1f} per 12")
    assert 12 * valu <= 64 * mfma, loop                                  # the bar: two thirds of what it was
    assert 12 * valu <= VALU_PER_12_REACHED * mfma, loop                 # what r13 reached
