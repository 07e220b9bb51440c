"""The rotation scalars of the Jacobi step pair in the assembly the library in this tree was built from (tools/isa_step_pair.py on
the production instantiation of the wave kernel): with the three magnitude tests of a rotation decided on the upper dwords
(csrc/letkf_rot_rule.h) and one vote per step pair, the step pair holds 379 instructions, was 383; 32 v_mul_f64, was 38 (the three
threshold products of either rotation are gone); and of FP64 compares only the two |t| > 1e-6 of the early-stop rule, was 8.  The
integer tests that replace them are, per rotation, one add, one max, one saturating subtract and the compare of `rot`, and per
step pair one max and two compares: 11 32-bit instructions.  None of this may grow back."""
import glob
import os
import sys

import pytest

from __graft_entry__ import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_step_pair


def test_rotation_scalars_of_the_production_step_pair():
    units = glob.glob(os.path.join(ROOT, "scale-letkf_amd", "lib", "obj", "letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not units:                                                       # (the GPU box receives the library, not its objects)
        pytest.skip("no device assembly beside the objects (built elsewhere)")
    n, mix, body = isa_step_pair.steppair(units[0])
    assert mix["v_mov_b32_dpp"] == 114, mix                             # the loop the tool picked is the step pair
    assert n <= 379, (n, mix.most_common(20))
    count = lambda pred: sum(c for op, c in mix.items() if pred(op))
    assert count(lambda op: op.startswith("v_mul_f64")) <= 32, mix
    assert count(lambda op: op.startswith("v_cmp") and "_f64" in op) <= 2, mix
    # the integer tests: no more than they were written as, and the saturating subtract is there (the guard on g2 hangs on it)
    assert count(lambda op: op.startswith(("v_add_u32", "v_sub_i32", "v_max_i32", "v_cmp_lt_i32", "v_cmp_gt_i32", "v_cmp_ge_i32",
                                           "v_cmp_le_i32"))) <= 11, mix
    assert sum(1 for line in body if line.strip().startswith("v_sub_i32") and line.rstrip().endswith("clamp")) == 2, mix
    # scalar bookkeeping of the votes: three ORs and the `hasR &&` of the odd rotation
    assert count(lambda op: op in ("s_or_b64", "s_and_b64")) <= 4, mix
