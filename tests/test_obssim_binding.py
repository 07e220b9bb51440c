"""What only the sixth companion header include/letkf_amd_obssim.h has (the checks every companion shares are in
test_companion_bindings.py): the one header that holds the point physics both kernels use, the Fortran routine and the driver's
call order."""
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


def test_the_point_physics_lives_in_one_header_both_kernels_include():
    for unit in ("letkf_obsope.hip", "letkf_obssim.hip"):
        assert '#include "letkf_obsope_point_dev.h"' in open(os.path.join(CSRC, unit)).read(), unit
    hdr = open(os.path.join(CSRC, "letkf_obsope_point_dev.h")).read()
    for name in ("calc_ref_vr", "ceil_split", "term2", "term3", "radar_azimuth", "radar_distance", "radar_elevation"):
        assert re.search(r"__device__ inline \w+ " + name + r"\(", hdr), name
        for f in os.listdir(CSRC):
            if f.endswith(".hip"):
                assert not re.search(r"__device__[^;{]*\b" + name + r"\(", open(os.path.join(CSRC, f)).read()), (name, f)
    for f in os.listdir(CSRC):
        if f.endswith(".hip"):
            assert not re.search(r'#include\s+"[^"]*\.hip"', open(os.path.join(CSRC, f)).read()), f


def test_the_fortran_routine_and_the_drivers_call_order(pkg):
    src = open(os.path.join(FDIR, "letkf_obssim_amd.f90")).read()
    assert callable(pkg.Context.obssim)
    assert re.search(r"SUBROUTINE obssim_cal_amd\(", src)
    drv = open(os.path.join(FDIR, "obssim_driver.f90")).read()
    assert drv.rindex("CALL state_to_history_amd") < drv.rindex("CALL obssim_cal_amd") < drv.rindex("WRITE (uo, rec=irec)")
    assert "access='direct'" in drv
