"""CPU checks of set_letkf_obs behind one call (include/letkf_amd.h section 9): the restatements of tests/native/setobs_oracle.c
against a plain numpy statement of the cited lines of scale/letkf/letkf_obs.f90, the library's host mesh-size helper
against the oracle, and the new C structs against their BIND(C) mirrors."""
import math
import os

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from _setobs import ELEM_UID, NID_OBS, NOBTYPE, UID, UNDEF, make_world, namelist, oracle_local, oracle_mesh_dims

DZF = float(np.float32(3.651483717))          # letkf_obs.f90:27, a single-precision literal


def np_preprocess(f, nml):
    """letkf_obs.f90:268-305, element by element (libm log10 through math.log10)"""
    elm, dat, err = f["elm"].copy(), f["dat"].copy(), f["err"].copy()
    mref = 10.0 ** (nml["min_radar_ref_dbz"] / 10.0)
    low = nml["min_radar_ref_dbz"] + nml["low_ref_shift"]
    use = np.zeros((NOBTYPE, NID_OBS), bool)
    for n in range(len(elm)):
        if elm[n] == 4001:
            if 0.0 <= dat[n] < 1.0e10:
                if dat[n] < mref:
                    elm[n], dat[n] = 4004, low
                else:
                    dat[n] = 10.0 * math.log10(dat[n])
            else:
                dat[n] = UNDEF
            if nml["use_obserr_radar_ref"]:
                err[n] = nml["obserr_radar_ref"]
        elif elm[n] == 4004:
            dat[n] = low
            if nml["use_obserr_radar_ref"]:
                err[n] = nml["obserr_radar_ref"]
        elif elm[n] == 4002 and nml["use_obserr_radar_vr"]:
            err[n] = nml["obserr_radar_vr"]
        use[f["typ"][n] - 1, UID[int(elm[n])] - 1] = True
    return elm, dat, err, use


def np_ctype_tables(use, nml):
    """letkf_obs.f90:307-342"""
    out = dict(elm=[], elm_u=[], typ=[], hl=[], vl=[])
    for ityp in range(1, NOBTYPE + 1):
        for u in range(1, NID_OBS + 1):
            if use[ityp - 1, u - 1]:
                e = ELEM_UID[u - 1]
                out["elm"].append(e)
                out["elm_u"].append(u)
                out["typ"].append(ityp)
                out["hl"].append(nml["hori_local_radar_obsnoref"] if e == 4004 else nml["hori_local_radar_vr"] if e == 4002
                                 else nml["hori_local"][ityp - 1])
                out["vl"].append(nml["vert_local_radar_vr"] if e == 4002 else nml["vert_local"][ityp - 1])
    return out


def np_mesh_dims(typ, hl, nml, nlon, nlat):
    """letkf_obs.f90:657-677"""
    rows = []
    for t, h in zip(typ, hl):
        if nml["obs_sort_grid_spacing"][t - 1] > 0:
            tg = nml["obs_sort_grid_spacing"][t - 1]
        elif nml["max_nobs_per_grid"][t - 1] > 0:
            tg = 0.1 * math.sqrt(float(nml["max_nobs_per_grid"][t - 1])) * nml["obs_min_spacing"][t - 1]
        else:
            tg = h * DZF / 6.0
        gi = min(math.ceil(nml["dx"] * nlon / tg), nlon)
        gj = min(math.ceil(nml["dy"] * nlat / tg), nlat)
        si, sj = nml["dx"] * nlon / gi, nml["dy"] * nlat / gj
        ni, nj = math.ceil(h * DZF / si), math.ceil(h * DZF / sj)
        rows.append((gi, gj, si, sj, ni, nj, gi + 2 * ni, gj + 2 * nj))
    return rows


@pytest.mark.parametrize("h08", [False, True])
def test_preprocess_and_ctype_tables_match_numpy(h08):
    nml = namelist()
    w = make_world(3, nfile_rows=(1500, 800), h08=h08)
    o = oracle_local(w, w["ranks"][0], nml)
    elm, dat, err, use = np_preprocess(w["files"], nml)
    assert np.array_equal(o["files"]["elm"], elm)
    assert np.array_equal(o["files"]["dat"], dat)
    assert np.array_equal(o["files"]["err"], err)
    e0, d0 = w["files"]["elm"], w["files"]["dat"]
    ref = e0 == 4001
    # every branch of :273-297 is taken
    assert ((elm == 4004) & ref).sum() > 10 and (dat[ref] == UNDEF).sum() > 10 and (ref & (d0 < 0)).sum() > 10
    assert (ref & (d0 >= 1e10)).sum() > 10 and ((elm == 4001) & (dat != UNDEF)).sum() > 100 and (e0 == 4004).sum() > 10
    t = np_ctype_tables(use, nml)
    assert np.array_equal(o["tables"]["elm_ctype"], t["elm"])
    assert np.array_equal(o["tables"]["elm_u_ctype"], t["elm_u"])
    assert np.array_equal(o["tables"]["typ_ctype"], t["typ"])
    assert np.array_equal(o["tables"]["hori_loc_ctype"], t["hl"])
    assert np.array_equal(o["tables"]["vert_loc_ctype"], t["vl"])
    # T (3073, type 1) has no obsda row but a ctype -- before PS (type 8), so it shifts PS's ctype number
    assert (3073 in t["elm"]) and t["elm"].index(3073) < t["elm"].index(14593)
    assert 3073 not in set(o["rows"]["elm"].tolist())
    # count tables: per ctype before / after QC
    for ic in range(o["nctype"]):
        sel = o["rows"]["ctype"] == ic
        assert o["tot"][ic, 0] == sel.sum() and o["tot"][ic, 1] == (sel & (o["qc"] == 0)).sum()


@pytest.mark.parametrize("nlon,nlat", [(12, 12), (40, 30), (5, 3)])
def test_mesh_dims_every_branch(nlon, nlat):
    nml = namelist()
    nml["obs_sort_grid_spacing"][2] = 250.0            # a spacing finer than DX: the min(., nlon) clamp
    typ = np.array([1, 3, 8, 22, 22, 23], np.int32)
    hl = np.array([4000.0, 3000.0, 5000.0, 2000.0, 2200.0, 400.0])
    o = oracle_mesh_dims(typ, hl, nml, nlon, nlat)
    exp = np_mesh_dims(typ, hl, nml, nlon, nlat)
    got = list(zip(*[o[k] for k in ("ngrd_i", "ngrd_j", "grdspc_i", "grdspc_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i",
                                     "ngrdext_j")]))
    assert [tuple(float(x) for x in g) for g in got] == [tuple(float(x) for x in e) for e in exp]
    assert o["ngrd_i"][1] == nlon and o["ngrd_j"][1] == nlat            # clamped
    pkg = load_package()
    pkg.build()
    h = pkg.obs_mesh_dims(typ, hl, nml["obs_sort_grid_spacing"], nml["max_nobs_per_grid"], nml["obs_min_spacing"],
                          nml["dx"], nml["dy"], nlon, nlat)
    for k in o:
        assert np.array_equal(h[k], o[k]), k


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/amdflang"), reason="amdflang not present")
def test_setobs_structs_mirror_bind_c():
    from _header import c_structs, fortran_types
    src = open(os.path.join(ROOT, "scale-letkf_amd", "fortran", "letkf_amd_api.f90")).read()
    cs, fs = c_structs(), fortran_types(src)
    for name in ("letkf_setobs_params", "letkf_obs_file_rows", "letkf_obs_table_info"):
        assert fs[name] == cs[name], name
    for entry in ("letkf_set_obs_local_dev", "letkf_set_obs_finish_dev", "letkf_set_obs_dev", "letkf_obs_mesh_dims",
                  "letkf_obs_table_search", "letkf_obs_table_destroy"):
        assert f"BIND(C, name='{entry}')" in src


def test_setobs_ctypes_mirror_sizes():
    import ctypes as C
    from _header import sizeof
    pkg = load_package()
    assert (sizeof("letkf_setobs_params"), sizeof("letkf_obs_file_rows"), sizeof("letkf_obs_table_info")) == (
        C.sizeof(pkg.SetObsParams), C.sizeof(pkg.ObsFileRows), C.sizeof(pkg.ObsTableInfo))
