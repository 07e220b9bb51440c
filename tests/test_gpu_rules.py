"""letkf_rules_dev.h (the per-point update rules every solver kernel calls) on the device against a plain host restatement
written from the reference's lines: every helper over a few hundred tuples that hold the corners the guards exist for.
Integers and booleans equal, floating results within 8 x 2^-53 of the tuple's largest intermediate."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.gpu
def test_rules_match_the_host_restatement(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = tmp_path / "rules_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "scale-letkf_amd", "csrc"),
                    os.path.join(HERE, "hip", "rules_check.hip"), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "mismatches 0"
