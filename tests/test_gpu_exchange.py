"""The exchange entry of the library (C ABI section 8, letkf_obs_allgatherv_dev = MPI_ALLGATHERV of
scale/letkf/letkf_obs.f90:1036-1046 as grouped ncclSend / ncclRecv) on a real RCCL communicator.  One GPU is all a test
box has, so the communicator has one rank (send-to-self inside the group): that exercises the run-time binding of
RCCL, the communicator hand-over from the host, stream ordering and the byte arithmetic.  More than one rank: what every
rank of an N-rank job posts is checked on the CPU against a recording stand-in for RCCL (tests/test_exchange_plan.py), the
entries' own nranks > 1 code runs on this one GPU with 2 .. 9 simulated ranks behind a loop-back stand-in that really moves
the bytes (tests/test_gpu_exchange_ranks.py -- not RCCL: it proves the arithmetic, not that RCCL comes up on N devices), the
Python twin is checked by tests/test_sharding_gloo.py.

The communicator is created the way a host of the library creates it -- ncclGetUniqueId + ncclCommInitRank, as bench.py
--exchange lib does -- in a fresh child process with RCCL's own log switched on.  History: in round 2 ncclCommInitAll,
called inside the pytest process (HIP initialised through torch, ~250 tests run, the library's non-blocking stream
alive), once never returned on a pool box; nothing of that run was kept.  What that call does that this one does not:
ncclCommInitAll spawns one bootstrap thread per device and rendezvouses them over a socket on the first interface RCCL
finds (the container's host name does not resolve on the pool; NCCL_SOCKET_IFNAME is pinned to the loopback below).
A communicator that does not come up within the limit is a FAILURE here, with RCCL's log in the message -- not a skip."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def rccl():
    return C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"))


def _one_rank_exchange():
    from _gpu import ctx
    lib = rccl()

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]
    uid = UniqueId()
    assert lib.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    lib.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert lib.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        c = ctx()
        for rows, cols, dt in [(1000, 51, torch.float64), (0, 51, torch.float64), (777, 1, torch.int32)]:
            send = (torch.randn(rows, cols, device="cuda") * 100).to(dt)
            recv = torch.full((max(rows, 1), cols), -1, dtype=dt, device="cuda")
            c.obs_allgatherv(comm.value, 0, [rows], send, recv)
            torch.cuda.synchronize()
            assert torch.equal(recv[:rows], send)
        # ---- the other exchanges on the same communicator (C ABI 8b), one rank: everything is the own block
        import numpy as np
        send = torch.randn(40, 51, dtype=torch.float64, device="cuda")
        recv = torch.full((64, 51), -1.0, dtype=torch.float64, device="cuda")
        c.alltoallv(comm.value, 0, [33], [5], [33], [20], 51 * 8, send, recv)      # rows 5 .. 38 of send -> rows 20 .. 53 of recv
        torch.cuda.synchronize()
        assert torch.equal(recv[20:53], send[5:38]) and bool((recv[:20] == -1).all()) and bool((recv[53:] == -1).all())
        cnt = torch.arange(1000, dtype=torch.int32, device="cuda")
        c.allreduce_sum_i32(comm.value, 1, cnt)
        torch.cuda.synchronize()
        assert torch.equal(cnt.cpu(), torch.arange(1000, dtype=torch.int32))
        # scatter / gather_grd_mpi_alltoall through the library: member fields -> slots of the point-major state and back
        nlev, nlon, nlat, nv3d, nens = 9, 13, 7, 3, 5
        nij1 = nlon * nlat
        x = torch.full((nv3d * nens * nlev * nij1,), float("nan"), dtype=torch.float64, device="cuda")
        fields = [torch.from_numpy(np.random.default_rng(50 + m).standard_normal(nv3d * nlat * nlon * nlev)).cuda() for m in range(3)]
        for m in range(3):
            c.members_alltoall(comm.value, 1, 0, 0, nlev, nlon, nlat, nv3d, m + 1, 1, fields[m], x, 1, nlev * nij1, nens * nlev * nij1)
        torch.cuda.synchronize()
        xv = x.view(nv3d, nens, nlev, nij1)
        for m in range(3):
            f = fields[m].view(nv3d, nlat * nlon, nlev)                              # v3dg(nlev,nlon,nlat,nv3d): level-fastest
            assert torch.equal(xv[:, m + 1], f.permute(0, 2, 1))
        assert bool(torch.isnan(xv[:, 0]).all()) and bool(torch.isnan(xv[:, 4]).all())
        back = torch.full_like(fields[0], float("nan"))
        c.members_alltoall(comm.value, 1, 0, 1, nlev, nlon, nlat, nv3d, 2, 1, back, x, 1, nlev * nij1, nens * nlev * nij1)
        torch.cuda.synchronize()
        assert torch.equal(back, fields[1])
        c.members_alltoall(0, 1, 0, 1, nlev, nlon, nlat, nv3d, 3, 1, back, x, 1, nlev * nij1, nens * nlev * nij1)   # one rank needs no communicator
        torch.cuda.synchronize()
        assert torch.equal(back, fields[2])
        # argument errors are reported, not executed
        from _gpu import pkg
        try:
            c.obs_allgatherv(comm.value, 1, [5], send, recv)          # myrank out of range
        except pkg.LetkfError:
            pass
        else:
            raise AssertionError("myrank out of range was accepted")
    finally:
        lib.ncclCommDestroy(comm)


def test_allgatherv_on_a_one_rank_communicator():
    """In a child process under a time limit, RCCL's log captured: a communicator that does not come up FAILS the test
    with that log (round 2 turned the one hang seen into a skip, which would have hidden a recurrence)."""
    import subprocess
    import sys
    env = dict(os.environ, NCCL_DEBUG="INFO", NCCL_DEBUG_SUBSYS="INIT,BOOTSTRAP,NET,ENV", NCCL_SOCKET_IFNAME="lo",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=240, env=env)
    except subprocess.TimeoutExpired as e:
        tail = lambda b: (b.decode(errors="replace") if isinstance(b, bytes) else (b or ""))[-6000:]
        pytest.fail("RCCL communicator creation / the one-rank exchange did not return within 240 s; RCCL log:\n"
                    + tail(e.stdout) + "\n" + tail(e.stderr))
    assert r.returncode == 0 and "one-rank exchange ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the repo root: __graft_entry__
    _one_rank_exchange()
    print("one-rank exchange ok")
