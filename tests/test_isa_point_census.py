"""tools/isa_point_census.py on the assembly the library in this tree was built from: the production instantiation of the wave
kernel, letkf_wave_kernel<50, 11, false, 1, 0>, must not grow back the lane traffic of parked scalars that r12 took out of its
point loop (profiles/r12_README.md).  Before r12 the function held 2 926 v_readlane_b32 -- whole 8- and 16-dword
argument tuples fetched from a spill register for one field, and a 64-bit lane mask per row of every masked per-row loop -- and
ten spill registers written by v_writelane_b32; the bounds below are the figures r12 reached."""
import glob
import os
import sys

import pytest

from __graft_entry__ import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_point_census

READLANES_BEFORE = 2926


@pytest.fixture(scope="module")
def census():
    units = glob.glob(os.path.join(ROOT, "scale-letkf_amd", "lib", "obj", "letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not units:                                                       # (the GPU box receives the library, not its objects)
        pytest.skip("no device assembly beside the objects (built elsewhere)")
    c = isa_point_census.census(units[0])
    assert c["step_pair"] is not None and c["gram_tile_loop"] is not None and c["point_loop"] is not None, c["spans"]
    return c


def test_lane_reads_of_the_production_kernel(census):
    n = census["function"]["v_readlane_b32"]
    assert n <= READLANES_BEFORE // 2, n                                # the bar: at most half of what it was
    assert n <= 978, n                                                  # what r12 reached


def test_no_lane_reads_in_the_two_hot_loops(census):
    assert census["gram_tile_loop"] is not None and census["gram_tile_loop"]["mfma"] > 0
    assert census["gram_tile_loop"]["v_readlane_b32"] == 0, census["gram_tile_loop"]
    assert census["step_pair"]["v_readlane_b32"] == 0, census["step_pair"]


def test_step_pair_length(census):
    assert census["step_pair"]["all"] == 379, census["step_pair"]


def test_spill_registers(census):
    regs = census["writelane_registers"]
    assert len(regs) <= 4, regs                                         # ten before r12
    assert census["function"]["v_writelane_b32"] <= 212, census["function"]
