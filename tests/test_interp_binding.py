"""What only the companion header include/letkf_amd_interp.h has (the checks every companion shares are in
test_companion_bindings.py): the coarse set of an axis against its definition, and the Fortran routine's signature."""
import ctypes as C
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


@pytest.mark.parametrize("n", [1, 2, 5, 7, 8])
@pytest.mark.parametrize("stride", [1, 2, 3, 4, 8])
def test_coarse_axis_is_the_strided_set_with_the_end(pkg, n, stride):
    want = sorted(set(range(0, n, stride)) | {n - 1})
    assert list(pkg.interp_coarse_axis(n, stride)) == want
    cnt = C.c_int32(-1)
    assert pkg.lib().letkf_interp_coarse_axis(n, stride, None, C.byref(cnt)) == 0 and cnt.value == len(want)


def test_coarse_axis_refuses_bad_arguments(pkg):
    cnt = C.c_int32(-1)
    for n, s in ((0, 1), (5, 0), (-1, 2)):
        assert pkg.lib().letkf_interp_coarse_axis(n, s, None, C.byref(cnt)) == -1


def test_the_fortran_routine_and_no_option_of_its_own(pkg):
    src = open(os.path.join(FDIR, "letkf_interp_amd.f90")).read()
    assert not [a for a in dir(pkg.Context) if a.startswith("OPT_") and "INTERP" in a]
    assert re.search(r"SUBROUTINE das_letkf_interp_amd\(ctx, args, tables, nx, ny, nlev, stride_x, stride_y", src)
