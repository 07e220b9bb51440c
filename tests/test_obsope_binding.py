"""What only the third companion header include/letkf_amd_obsope.h has (the checks every companion shares are in
test_companion_bindings.py): the Fortran routine's signature and the driver's call order."""
import os
import re

import pytest

from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_the_fortran_routine_and_the_drivers_call_order(pkg):
    src = open(os.path.join(FDIR, "letkf_obsope_amd.f90")).read()
    assert callable(pkg.Context.obsope)
    assert re.search(r"SUBROUTINE obsope_amd\(ctx, prm, nfile, off, elm, typ, lev, ri, rj, fields, n1, n2, set, idx, qc, ensval", src)
    drv = open(os.path.join(FDIR, "obsope_driver.f90")).read()
    assert drv.index("CALL obsope_amd") < drv.index("CALL set_letkf_obs_amd(ctx")     # the operator reads the files first
