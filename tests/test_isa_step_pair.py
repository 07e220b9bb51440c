"""tools/isa_step_pair.py on the assembly the library in this tree was built from: the tool must find the production instantiation
of the wave kernel (its last template argument is the integer FUSED mode), and the Jacobi step pair -- the loop the kernel spends
most of its FP64 issue slots in -- must not grow back past the count the ends of the line were trimmed to; nor the
kernel's matrix instructions past 18 (Gram step) + 117 (warm-start product, nine full tiles x 13 steps) + 104 (apply)."""
import glob
import os
import sys

import pytest

from __graft_entry__ import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_step_pair


def test_step_pair_of_the_production_kernel():
    units = glob.glob(os.path.join(ROOT, "scale-letkf_amd", "lib", "obj", "letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not units:                                                       # (the GPU box receives the library, not its objects)
        pytest.skip("no device assembly beside the objects (built elsewhere)")
    n, mix, body = isa_step_pair.steppair(units[0])
    assert mix["v_mov_b32_dpp"] == 114, mix                             # the loop the tool picked is the step pair
    assert n <= 383, (n, mix.most_common(20))
    # the selects that are left are the two `rot ? tt : 0.0` of the even and the odd step
    assert sum(c for op, c in mix.items() if op.startswith("v_cndmask")) <= 4, mix


def test_matrix_instructions_of_the_production_kernel():
    units = glob.glob(os.path.join(ROOT, "scale-letkf_amd", "lib", "obj", "letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not units:
        pytest.skip("no device assembly beside the objects (built elsewhere)")
    kern = "_ZN5letkf17letkf_wave_kernelILi50ELi11ELb0ELi1ELi0EEEvNS_9PointArgsE:"
    n, inside = 0, False
    with open(units[0]) as f:
        for line in f:
            if line.startswith(kern):
                inside = True
            elif inside and line.strip().startswith("s_endpgm"):
                break
            elif inside and line.strip().startswith("v_mfma_f64_16x16x4"):
                n += 1
    assert inside and 0 < n <= 18 + 117 + 104, n
