"""The record codec from a Fortran host (scale-letkf_amd/fortran/letkf_obsfile_amd.f90): obsfile_driver writes conventional, radar
and obsda files with Fortran's own sequential unformatted WRITE, reads their bytes with stream access, decodes and assembles
them on the device and compares with what it wrote; then it encodes on the device, writes the bytes with stream access and reads
them back with sequential READ.  Every line it prints must say PASS.  Without a device: the module compiles under amdflang."""
import os
import subprocess

import pytest

from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "obsfile_driver")
FC = "/opt/rocm/bin/amdflang"
HAVE_FC = os.path.exists(FC)
CHECKS = {"conv_count", "conv_decode", "conv_denormal_kept", "conv_encode", "radar_count", "radar_decode", "radar_encode_without_undefined",
          "obsda_count", "obsda_assemble", "obsda_encode"}


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_the_module_and_the_driver_compile_with_amdflang(tmp_path):
    for f in ("letkf_amd_api", "letkf_mapproj_amd", "letkf_obsfile_amd"):
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / "letkf_obsfile_amd.mod").exists()
    subprocess.check_call([FC, "-O2", "-c", os.path.join(FDIR, "obsfile_driver.f90"), "-o", str(tmp_path / "obsfile_driver.o")], cwd=tmp_path)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_checks_the_framing_against_fortrans_own_io(tmp_path):
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "obsfile"], stdout=subprocess.DEVNULL)
    r = subprocess.run([DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=120)
    lines = [l.split() for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert all(l[0] == "PASS" for l in lines), r.stdout
    assert {l[1] for l in lines} == CHECKS, r.stdout
    # the files Fortran wrote and the files the device wrote lie side by side: same sizes where every row is kept
    for a, b in (("conv.dat", "conv_dev.dat"), ("obsda2.dat", "obsda_dev.dat")):
        assert os.path.getsize(tmp_path / a) == os.path.getsize(tmp_path / b) > 0
    assert os.path.getsize(tmp_path / "radar.dat") == 36 + 36 * 300 and os.path.getsize(tmp_path / "radar_dev.dat") == 36 + 36 * (300 - 300 // 7)
