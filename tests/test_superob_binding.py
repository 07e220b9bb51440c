"""What only the seventh companion header include/letkf_amd_superob.h has (the checks every companion shares are in
test_companion_bindings.py): the one select kernel for both stages, the Fortran routine and the driver's call order, and the
two host-only helpers against the statement."""
import os
import re

import numpy as np
import pytest

import _superob as S
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
CSRC = os.path.join(PKG_DIR, "csrc")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_one_select_kernel_serves_both_stages():
    kernels = open(os.path.join(CSRC, "letkf_superob.hip")).read()
    assert len(re.findall(r"__global__[^;{]*\bsuperob_select_kernel\(", kernels)) == 1      # one select kernel for both stages
    assert "superob_select_kernel<true>" in kernels and "superob_select_kernel<false>" in kernels


def test_the_fortran_routine_and_the_drivers_call_order(pkg):
    src = open(os.path.join(FDIR, "letkf_superob_amd.f90")).read()
    assert callable(pkg.Context.superob)
    assert re.search(r"SUBROUTINE superob_amd\(", src)
    drv = open(os.path.join(FDIR, "superob_driver.f90")).read()
    assert drv.rindex("CALL superob_amd") < drv.rindex("letkf_ctx_synchronize") < drv.rindex("WRITE (uo)")
    assert "access='sequential'" in drv


def test_the_host_helpers_are_the_statements(pkg):
    for nslots, nbslot in ((7, 4), (1, 1), (4, 1), (64, 33), (5, 5), (6, 3)):
        assert [int(s) for s in pkg.superob_slot_priority(nslots, nbslot)] == S.slot_priority(nslots, nbslot)
    assert [int(s) for s in pkg.superob_slot_priority(7, 4)] == [4, 3, 5, 2, 6, 1, 7]
    for nobtype, nid in ((24, 16), (4, 4), (32, 32), (1, 1)):
        for a, b in zip(pkg.superob_default_methods(nobtype, nid), S.default_methods(nobtype, nid)):
            assert a.shape == (nid, nobtype) and np.array_equal(a, b)
    for bad in ((0, 1), (65, 1), (3, 0), (3, 4)):
        with pytest.raises(pkg.LetkfError):
            pkg.superob_slot_priority(*bad)
    for bad in ((0, 4), (33, 4), (4, 0), (4, 33)):
        with pytest.raises(pkg.LetkfError):
            pkg.superob_default_methods(*bad)
    assert pkg.SUPEROB_SURFACE_TYPES == S.SURFACE_TYPES == sum(1 << (t - 1) for t in (8, 9, 10, 11, 15))
