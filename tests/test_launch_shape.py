"""The launch shape of the register kernels (scale-letkf_amd/csrc/letkf_launch_shape.h: run length, grids, plan inputs, plan and
workspace bytes of letkf_wave_kernel and letkf_trio_kernel) without a GPU and without the library: a stand-alone program
(tests/native/launch_shape_cases.cpp, host code only) prints the shape of every case of tests/golden/launch_shape/parent_shapes.npz,
which holds what the four code sites computed that decided the shape before there was one function
(profiles/launch_shape_README.md says from which commit and lines).  Which points start cold is a function of the shape, so a
field that moves here moves results: a change of a rule is made in that header, judged here, and re-records the fixture."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "launch_shape_cases.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_shape", "parent_shapes.npz")
INPUTS = ["trio", "k", "mode", "npts", "stride", "run_req", "num_cu", "resident", "dynamic", "grid_per_cu"]
SCALARS = ["run_len", "grid", "grid_ws", "warm_bytes", "ppw", "resident_per_xcd", "ub_of", "reset_counters"]
PLAN = ["base", "whole", "f", "t", "nstat", "magic"]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    d = tmp_path_factory.mktemp("launch_shape")
    exe = str(d / "launch_shape_cases")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "scale-letkf_amd", "csrc"), SRC, "-o", exe], check=True)

    def run(inputs):
        """inputs: {name: [ncase]} -> every output column of the program, by name"""
        path = str(d / "cases.txt")
        np.savetxt(path, np.stack([inputs[n] for n in INPUTS], axis=1), fmt="%d")
        rows = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
        assert len(rows) == len(inputs["k"])
        cols = np.array([[int(v) for v in r.split()] for r in rows], dtype=object)
        assert cols.shape[1] == 60
        out = {n: cols[:, i].astype(np.int64) for i, n in enumerate(SCALARS)}
        for j, n in enumerate(PLAN):
            out["plan_" + n] = cols[:, 8 + 8 * j:16 + 8 * j].astype(np.uint64 if n == "magic" else np.int32)
        for i, n in enumerate(["plan_ub", "plan_nruns", "plan_same", "walk"]):
            out[n] = cols[:, 56 + i].astype(np.int64)
        return out
    return run


@pytest.fixture(scope="module")
def shapes(golden, program):
    return program({n: golden["in_" + n] for n in INPUTS})


def assert_recorded(got, golden):
    for n in SCALARS + ["plan_" + p for p in PLAN] + ["plan_ub", "plan_nruns"]:
        bad = np.flatnonzero((got[n] != golden[n]).reshape(len(got[n]), -1).any(axis=1))
        assert bad.size == 0, (n, [(dict((i, int(golden["in_" + i][c])) for i in INPUTS), got[n][c], golden[n][c]) for c in bad[:3]])


def test_the_case_list_is_what_the_checks_assume(golden):
    n = len(golden["in_k"])
    assert 3000 <= n <= 4096
    assert set(golden["in_k"]) == {2, 16, 17, 20, 21, 32, 48, 50, 62, 63, 64, 80, 100}
    assert set(golden["in_k"][golden["in_trio"] == 1]) == {2, 16, 17, 20} and set(golden["in_mode"][golden["in_trio"] == 1]) == {0}
    assert set(golden["in_mode"][golden["in_k"] <= 62]) == {0, 1, 2, 3} and set(golden["in_mode"][golden["in_k"] >= 63]) == {0, 1}
    assert set(golden["in_run_req"]) == {0, 1, 2, 3, 5, 16, 128, 4096, 5000}
    assert set(golden["in_num_cu"]) == {1, 8, 256, 304} and set(golden["in_resident"]) == {0, 1, 2, 3}
    assert set(golden["in_dynamic"]) == {0, 1} and {0, 1, 3, 4, 63, 64, 65} <= set(golden["in_npts"])
    assert np.all(golden["in_npts"] % golden["in_stride"] == 0)      # (prepare_wave refuses anything else)


def test_every_field_is_the_recorded_one(shapes, golden):
    assert_recorded(shapes, golden)


def test_a_launcher_gets_the_shape_from_the_run_length_prepare_wave_stored(program, golden):
    """prepare_wave asks with the call's run request and no occupancy and stores run_len; the launcher asks again with that
    run_len as the request and its kernel's occupancy.  The recorded shapes are those of that chain."""
    inp = {n: golden["in_" + n].copy() for n in INPUTS}
    first = dict(inp, resident=np.zeros_like(inp["resident"]))
    inp["run_req"] = program(first)["run_len"]
    assert np.any(inp["run_req"] != golden["in_run_req"])
    got = program(inp)
    assert_recorded(got, golden)


def test_every_plan_hands_out_every_run_once(shapes, golden):
    """Each case with dynamic dealing and a known occupancy: the plan that sched_plan_check's statements make from the shape's own
    run length, grid, ppw, resident_per_xcd and ub_of is the shape's plan, and its walk hands out every run exactly once, whole
    or as four quarters."""
    planned = (golden["in_dynamic"] == 1) & (golden["in_resident"] > 0)
    assert planned.sum() > 2000
    assert shapes["plan_nruns"].max() <= 1 << 27                     # (the walk's cap: the case list stays under it)
    assert np.all(shapes["plan_same"][planned] == 1)
    bad = np.flatnonzero(planned & (shapes["walk"] != 0))
    assert bad.size == 0, [(dict((i, int(golden["in_" + i][c])) for i in INPUTS), int(shapes["walk"][c])) for c in bad[:3]]
    # without a plan (static dealing, or prepare_wave's call before a launcher is chosen) the plan is all zero
    for p in PLAN:
        assert not shapes["plan_" + p][~planned].any()
    assert np.all(shapes["grid"][~planned] == shapes["grid_ws"][~planned])
