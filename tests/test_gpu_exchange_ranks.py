"""The exchange entries of the library (C ABI section 8: letkf_members_alltoall_dev, letkf_alltoallv_dev,
letkf_obs_allgatherv_dev, letkf_allreduce_sum_i32_dev) with 2 .. 9 ranks on one GPU, and set_letkf_obs composed across ranks
on them.  RCCL refuses two ranks on one device, so the transport is the loop-back stand-in of tests/_loopback.py /
tests/native/rccl_loopback.c behind the library's run-time binding: the ranks are contexts in ONE fresh child process,
called one after the other; the library's own nranks > 1 code runs end to end -- pack kernels, grouped sends and receives,
unpack kernels, in their real order on real buffers.  Every comparison is exact: this is data movement and integer sums.

One child runs all the cases under one time limit and prints one JSON line; the tests below read their cases out of it.
A child that fails or does not return fails every test once, with its output.  The pytest process itself never hands a
stand-in handle to the library (it may have bound the real RCCL): that happens in the child alone, after the child has
checked that the ncclSend in its global scope is the stand-in's.  What the stand-in does not prove -- RCCL itself, several
devices, concurrency -- is said in tests/_loopback.py; the one-rank test on the real RCCL is tests/test_gpu_exchange.py."""
import functools
import json
import os
import subprocess
import sys

import pytest

import _loopback as L

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def child():
    """(results, None) or (None, why): the child is started once per session"""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(L.__file__)], capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        tail = lambda b: (b.decode(errors="replace") if isinstance(b, bytes) else (b or ""))[-6000:]
        return None, "the loop-back child did not return within 240 s:\n" + tail(e.stdout) + "\n" + tail(e.stderr)
    lines = [l for l in r.stdout.splitlines() if l.startswith(L.RESULT_MARK)]
    if r.returncode != 0 or len(lines) != 1:
        return None, f"the loop-back child ended with {r.returncode}:\n" + r.stdout[-3000:] + r.stderr[-6000:]
    return json.loads(lines[0][len(L.RESULT_MARK):]), None


def check(ids):
    out, why = child()
    if out is None:
        pytest.fail(why)
    assert out["bound"] is True                     # the address comparison ran before the first multi-rank call
    res = out["results"]
    failed, total = [], dict(sends=0, recvs=0, send_bytes=0, groups=0, allreduces=0)
    for cid in ids:
        r = res.get(cid)
        if r is None:
            failed.append(f"{cid}: not run (the child stopped at an earlier case)")
            continue
        c = r["counters"]
        print(f"{cid}: sends {c['sends']} receives {c['recvs']} bytes {c['send_bytes']} groups {c['groups']} "
              f"all-reduces {c['allreduces']}" + ("" if r["ok"] else "  FAILED"))
        for k in total:
            total[k] += c[k]
        if not r["ok"]:
            failed.append(f"{cid}: {r['error']}")
    print(f"total of {len(ids)} cases: {total}")
    assert not failed, "\n".join(failed)
    return total


MEMBERS = L.members_cases()


@pytest.mark.parametrize("nranks", [2, 3, 4, 8])
def test_members_alltoall(nranks):
    """dir 0 then dir 1 on 13x7 (91 points: not divisible by 2, 3, 4, 8) and 16x8; a full batch, a short last batch, one
    member; nlev 1 / 9, nv3d 1 / 3; mstart 0 and > 0 with spare slots that stay NaN; two stride triples.  The state equals
    the definition and the oracle's orc_member_points bit for bit, dir 1 returns every holder's field and writes no
    non-holder's, and every rank posted exactly the messages of the definition inside one group."""
    ids = [c["id"] for c in MEMBERS if c["nranks"] == nranks and (c["nlon"], c["nlat"]) != (3, 2) and c["mcount"] > 0]
    assert len(ids) == 2 * 2 * 4 * (2 if nranks == 2 else 3)
    total = check(ids)
    assert total["sends"] > 0


def test_members_alltoall_more_ranks_than_points_in_a_row():
    """3x2 on 4 ranks: ranks 2 and 3 own one point, ranks 0 and 1 two"""
    check([c["id"] for c in MEMBERS if c["nranks"] == 4 and c["nlon"] == 3 and c["mcount"] > 0])


def test_members_alltoall_rank_without_points_takes_part():
    """3x2 on 8 ranks: ranks 6 and 7 own no point.  The contract of include/letkf_amd.h: such a rank makes the call with
    an empty state (x NULL), sends / receives the field of a member it holds, and every message of its peers is matched.
    (Before this was decided the library refused x == NULL: in a real job that rank would have left the group while its
    peers waited.)"""
    ids = [c["id"] for c in MEMBERS if c["nranks"] == 8 and c["nlon"] == 3 and c["mcount"] > 0]
    assert any("-mc8-" in i for i in ids)           # ranks 6 and 7 hold members 6 and 7 there
    check(ids)


def test_members_alltoall_empty_batch_posts_nothing():
    """mcount = 0: the call succeeds on every rank, moves nothing and the stand-in records nothing"""
    ids = [c["id"] for c in MEMBERS if c["mcount"] == 0]
    assert len(ids) == 10 * 2 * 4
    total = check(ids)
    assert total == dict(sends=0, recvs=0, send_bytes=0, groups=0, allreduces=0)


def test_alltoallv():
    """seeded send matrices for 2 .. 6 ranks (zero rows and columns, an all-zero rank, own blocks of zero and non-zero
    size), offsets with gaps and out of rank order, row_bytes 4 / 8 / 408; the halo exchange of a 3x3 world; the
    transpose's equal blocks.  Every receive buffer is the numpy scatter of the senders' rows, the sentinel elsewhere."""
    ids = [c["id"] for c in L.alltoallv_cases()]
    assert len(ids) == 5 * 3 + 2
    check(ids)


def test_alltoallv_refuses_an_own_block_of_two_sizes():
    total = check(["alltoallv-own-block-refused"])
    assert total == dict(sends=0, recvs=0, send_bytes=0, groups=0, allreduces=0)


def test_allgatherv():
    """every rank ends with the rank-major concatenation, rows beyond the total untouched; the send to oneself goes
    through ncclSend / ncclRecv and is served within the group"""
    check([c["id"] for c in L.allgatherv_cases()])


def test_allreduce_sum_i32():
    check([c["id"] for c in L.allreduce_cases()])


@pytest.mark.parametrize("world", ["2x2", "3x2"])
def test_set_obs_across_ranks_on_the_library_exchanges(world):
    """letkf_set_obs_local_dev, tot_sub through letkf_allreduce_sum_i32_dev, n_cell and the sorted send buffers through
    letkf_obs_allgatherv_dev, letkf_set_obs_finish_dev: the composition a host on N GPUs runs, the finished tables checked
    against the oracle as in tests/test_gpu_setobs.py test_two_by_two_world (which stands a concatenation in for the
    exchange)."""
    total = check([f"setobs-{world}"])
    assert total["allreduces"] > 0 and total["sends"] > 0


def test_every_case_has_a_test():
    out, why = child()
    if out is None:
        pytest.fail(why)
    assert sorted(out["results"]) == sorted(L.all_case_ids())
