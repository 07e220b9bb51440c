"""What only the fourth companion header include/letkf_amd_monit.h has (the checks every companion shares are in
test_companion_bindings.py): the Fortran routines with their element lists, the driver's call order, and letkf_monit_type
against the reference's list."""
import os
import re

import numpy as np
import pytest

import _monit as M
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_the_fortran_routines_their_element_lists_and_the_drivers_call_order(pkg):
    src = open(os.path.join(FDIR, "letkf_monit_amd.f90")).read()
    assert callable(pkg.Context.state_to_history) and callable(pkg.Context.monit_obs) and callable(pkg.monit_type)
    assert re.search(r"SUBROUTINE state_to_history_amd\(ctx, st, layout, v3d, v2d, ierr\)", src)
    assert re.search(r"SUBROUTINE monit_obs_amd\(ctx, mprm, prm, nfile, off, elm, typ, lev, ri, rj, dat, fields, nn, key, set, idx, rec, &\n"
                     r"\s+nobs, bias, rmse, monit_type, ierr\)", src)
    assert re.search(r"SUBROUTINE monit_print_amd\(nobs, bias, rmse, monit_type\)", src)
    assert [int(x) for x in re.search(r"elem_uid_monit\(nid_obs_monit\) = &\n\s+\(/([^/]*)/\)", src).group(1).split(",")] == M.ELEM_UID.tolist()
    assert re.findall(r"'([ \w]{3})'", re.search(r"obelmlist\(nid_obs_monit\) = &\n\s+\(/([^/]*)/\)", src).group(1)) == M.OBELMLIST
    drv = open(os.path.join(FDIR, "monit_driver.f90")).read()
    assert drv.index("CALL state_to_history_amd") < drv.index("CALL monit_obs_amd") < drv.index("CALL monit_print_amd")


@pytest.mark.parametrize("radar,h08", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_monit_type_is_the_references_list(pkg, radar, h08):
    """common_obs_scale.f90:1821-1837, the names spelled out here: U V T Tv Q PS; + REF RE0 Vr; + H08; RH and PRH never"""
    on = ["  U", "  V", "  T", " Tv", "  Q", " PS"] + (["REF", "RE0", " Vr"] if radar else []) + (["H08"] if h08 else [])
    want = np.array([1 if n in on else 0 for n in M.OBELMLIST], dtype=np.int32)
    got = pkg.monit_type(M.ELEM_UID, radar, h08)
    assert np.array_equal(got, want) and np.array_equal(M.monit_type(M.ELEM_UID, radar, h08), want)
    assert got[M.OBELMLIST.index(" RH")] == 0 and got[M.OBELMLIST.index("PRH")] == 0
    assert np.array_equal(pkg.monit_type(M.ELEM_UID[::-1].copy(), radar, h08), want[::-1])      # by id, not by position
    with pytest.raises(pkg.LetkfError):
        pkg.monit_type(np.zeros(33, dtype=np.int32), radar, h08)
