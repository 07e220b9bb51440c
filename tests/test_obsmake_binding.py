"""What only the fifth companion header include/letkf_amd_obsmake.h has (the checks every companion shares are in
test_companion_bindings.py): the SFMT recurrence as a host-only unit, the Fortran routines and the driver's call order."""
import os
import re

import pytest

from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
CSRC = os.path.join(PKG_DIR, "csrc")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_the_sfmt_recurrence_is_host_only():
    sfmt = open(os.path.join(CSRC, "letkf_sfmt.cpp")).read()
    assert "#include <hip" not in sfmt and "__global__" not in sfmt and "__device__" not in sfmt


def test_the_fortran_routines_and_the_drivers_call_order(pkg):
    src = open(os.path.join(FDIR, "letkf_obsmake_amd.f90")).read()
    assert callable(pkg.Context.randn) and callable(pkg.Context.obsmake_slot) and callable(pkg.Context.obsmake_noise) and callable(pkg.Rand)
    assert re.search(r"SUBROUTINE obsmake_slot_amd\(", src) and re.search(r"SUBROUTINE obsmake_noise_amd\(", src)
    drv = open(os.path.join(FDIR, "obsmake_driver.f90")).read()
    assert drv.rindex("CALL obsmake_slot_amd") < drv.rindex("CALL rand_create_amd") < drv.rindex("CALL obsmake_noise_amd")
