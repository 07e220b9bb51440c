"""The loop-back stand-in for RCCL (tests/_loopback.py, tests/native/rccl_loopback.c) without a GPU: it compiles with gcc,
its mailbox / two-pass / counter semantics hold on host memory (a child process gives it a host-memory twin of the four
HIP calls it resolves from the loaded runtime), the plan check flags every kind of broken plan on fabricated logs, and the
expected-result builders agree with the oracle and with hand-made examples.  The stand-in is loaded in child processes
only: in the pytest process its ncclSend would be what the library binds."""
import collections
import ctypes as C
import json
import subprocess
import sys

import numpy as np

import _loopback as L
import _oracle

OK_COUNTERS = dict.fromkeys(L.COUNTERS, 0)


def counters(**kw):
    return dict(OK_COUNTERS, **kw)


def test_plan_check_accepts_a_matched_plan_and_flags_every_defect():
    S, R = 0, 1
    good = [(S, 0, 1, 80, 1, 7, 1), (R, 1, 0, 40, 1, 7, 1), (S, 1, 0, 40, 1, 8, 2), (R, 0, 1, 80, 1, 8, 2)]
    cnt = counters(sends=2, recvs=2, send_bytes=120, recv_bytes=120, groups=2)
    plan = collections.Counter({(0, 1, 80): 1, (1, 0, 40): 1})
    assert L.plan_violations(good, cnt, 2, plan) == []
    # a send nobody receives (a hang on the real thing)
    assert any("sent but not received: [(1, 0, 40)]" in b for b in L.plan_violations(good[:1] + good[2:], counters(sends=2, recvs=1, groups=2), 2))
    # a receive nobody sends
    assert any("received but not sent: [(0, 1, 80)]" in b for b in L.plan_violations(good[1:], counters(sends=1, recvs=2, groups=2), 2))
    # matched among themselves, but not what the definition implies (a dropped pair)
    assert any("missing from the plan: [(1, 0, 40)]" in b for b in L.plan_violations([good[0], good[3]], counters(sends=1, recvs=1, groups=2), 2, plan))
    # the counters
    for k in L.MUST_BE_ZERO:
        assert L.plan_violations(good, dict(cnt, **{k: 1}), 2, plan) == [f"{k} = 1"]
    assert "the log and the counters disagree" in L.plan_violations(good, dict(cnt, sends=3), 2, plan)
    # grouping: outside a group, nested, two groups in one call, one group over two calls, more groups than calls
    assert any("depth 0" in b for b in L.plan_violations([(S, 0, 1, 80, 0, 7, 1)] + good[1:], cnt, 2, plan))
    assert any("depth 2" in b for b in L.plan_violations([(S, 0, 1, 80, 2, 7, 1)] + good[1:], cnt, 2, plan))
    assert any("more than one group" in b for b in L.plan_violations([(S, 0, 1, 80, 1, 6, 1)] + good[1:], dict(cnt, groups=3), 3, plan))
    assert any("spans more than one" in b for b in L.plan_violations([(S, 0, 1, 80, 1, 8, 1)] + good[2:] + [(R, 1, 0, 40, 1, 8, 1)], cnt, 2, plan))
    assert any("3 groups in 2" in b for b in L.plan_violations(good, dict(cnt, groups=3), 2, plan))


def test_expected_state_is_the_oracles_member_points():
    o = _oracle.oracle()
    for (nlon, nlat), nranks, nlev, nv3d, kind in [((13, 7), 3, 9, 3, "point"), ((13, 7), 8, 1, 3, "member"), ((16, 8), 4, 9, 1, "member"),
                                                   ((3, 2), 4, 9, 3, "point"), ((3, 2), 8, 1, 1, "member")]:
        nens, nxy = 7, nlon * nlat
        fields = {m: L.member_field(3, m, nlev, nlon, nlat, nv3d) for m in (2, 3, 5)}
        assert sum(L.share(nxy, p, nranks) for p in range(nranks)) == nxy
        for p in range(nranks):
            nij1 = L.share(nxy, p, nranks)
            assert nij1 == (nxy - p + nranks - 1) // nranks
            st = L.strides(kind, nij1, nlev, nens)
            e = L.expected_state(fields, nlev, nlon, nlat, nv3d, nens, nranks, p, *st)
            assert e.size == nv3d * nens * nlev * nij1
            xo = np.full_like(e, np.nan)
            if nij1:
                for m, f in fields.items():
                    o.orc_member_points(C.c_int(0), C.c_int(nlev), C.c_int(nlon), C.c_int(nlat), C.c_int(nv3d), C.c_int(nranks),
                                        C.c_int(p), C.c_int(m), _oracle._dp(f), _oracle._dp(xo), C.c_int64(nij1),
                                        *[C.c_int64(v) for v in st])
            assert np.array_equal(e, xo, equal_nan=True)
            assert np.isnan(e).sum() == nv3d * (nens - 3) * nlev * nij1          # the slots nobody sent
    assert L.share(6, 6, 8) == 0 and L.share(6, 7, 8) == 0 and L.share(6, 5, 8) == 1


def test_members_plan():
    # 6 points on 8 ranks, two holders: each sends to the five other ranks that own a point, none to ranks 6 and 7
    p = L.members_plan(0, 8, 6, 9, 3, 2)
    assert sorted(p) == [(0, d, 8 * 27) for d in (1, 2, 3, 4, 5)] + [(1, d, 8 * 27) for d in (0, 2, 3, 4, 5)]
    assert L.members_plan(1, 8, 6, 9, 3, 2) == collections.Counter({(d, s, n): 1 for (s, d, n) in p})
    # 91 points on 4 ranks: 23, 23, 23, 22
    assert L.members_plan(0, 4, 91, 1, 1, 1) == collections.Counter({(0, 1, 8 * 23): 1, (0, 2, 8 * 23): 1, (0, 3, 8 * 22): 1})
    assert not L.members_plan(0, 4, 91, 1, 1, 0)


def test_case_lists_cover_what_they_must():
    mc = L.members_cases()
    assert len({c["id"] for c in mc}) == len(mc)
    for g, r in [((13, 7), 2), ((13, 7), 3), ((13, 7), 4), ((13, 7), 8), ((16, 8), 2), ((16, 8), 8), ((3, 2), 4), ((3, 2), 8)]:
        sub = [c for c in mc if (c["nlon"], c["nlat"]) == g and c["nranks"] == r]
        assert {c["mcount"] for c in sub} == {r, r - 1, 1, 0}
        assert {c["stride"] for c in sub} == {"point", "member"}
        assert {c["nlev"] for c in sub} == {1, 9} and {c["nv3d"] for c in sub} == {1, 3}
        assert {c["mstart"] > 0 for c in sub} == {True, False}
        assert all(c["nens"] > c["mstart"] + c["mcount"] for c in sub)
    for c in L.alltoallv_cases():
        M, n = c["M"], len(c["M"])
        if "random" in c["id"] and n >= 3:
            off = lambda s, d: M[s][d] if s != d else 0
            zero = [z for z in range(n) if not any(M[z]) and not any(M[s][z] for s in range(n))]
            assert len(zero) >= 1                                                          # an all-zero rank
            assert any(not any(off(s, d) for d in range(n)) for s in range(n) if s not in zero)   # another zero row
            assert any(not any(off(s, d) for s in range(n)) for d in range(n) if d not in zero)   # another zero column
    diag = [c["M"][q][q] for c in L.alltoallv_cases() if "random" in c["id"] for q in range(len(c["M"]))]
    assert 0 in diag and 3 in diag                                                         # own blocks of both kinds
    H = L.halo_matrix()
    assert sum(1 for s in range(9) if s != 4 and H[s][4] > 0) == 8 and H[0][8] == 0 and H[0][2] == 0 and H[0][4] > 0
    assert {c["row_bytes"] for c in L.alltoallv_cases() if "random" in c["id"]} == {4, 8, 408}
    assert any(v == 1 for c in L.alltoallv_cases() for s, row in enumerate(c["M"]) for d, v in enumerate(row) if s != d)
    assert any((a < 0).any() for c in L.allreduce_cases() for a in L.allreduce_inputs(c["nranks"], c["count"]))


def test_alltoallv_expected_by_hand():
    M = [[1, 2], [3, 0]]
    lay = L.alltoallv_layout(M, 1)
    for me in range(2):                              # blocks do not overlap, in either buffer
        for key, cnt in (("soff", M[me]), ("roff", [M[0][me], M[1][me]])):
            a, b = lay[me][key]
            assert a + cnt[0] <= b or b + cnt[1] <= a
    rb = 4
    sends = [np.arange(lay[r]["nsend"] * rb, dtype=np.uint8) + 100 * r for r in range(2)]
    e = L.alltoallv_expected(M, lay, rb, sends, 0)
    own, other = lay[0]["roff"][0] * rb, lay[0]["roff"][1] * rb
    assert np.array_equal(e[own:own + 4], sends[0][lay[0]["soff"][0] * rb:][:4])
    assert np.array_equal(e[other:other + 12], sends[1][lay[1]["soff"][0] * rb:][:12])
    untouched = np.ones(e.size, bool)
    untouched[own:own + 4] = untouched[other:other + 12] = False
    assert (e[untouched] == L.SENTINEL).all()
    assert L.alltoallv_plan(M, rb) == collections.Counter({(0, 1, 8): 1, (1, 0, 12): 1})
    assert L.allgatherv_plan([5, 0, 7], 4) == collections.Counter({(s, d, n): 1 for s, n in ((0, 20), (2, 28)) for d in range(3)})


FAKE_HIP = r"""
#include <stdlib.h>
#include <string.h>
int hipMalloc(void **p, size_t n) { *p = malloc(n ? n : 1); return *p ? 0 : 2; }
int hipFree(void *p) { free(p); return 0; }
int hipMemcpyAsync(void *d, const void *s, size_t n, int kind, void *st) { (void)kind; (void)st; memcpy(d, s, n); return 0; }
int hipStreamSynchronize(void *st) { (void)st; return 0; }
"""

CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import _loopback as L
out = {}
lb = L.Loopback()
out["unbound"] = lb.lib.lb_bind_hip()                       # no HIP runtime in the process yet: refused, loudly
out["unbound_msg"] = lb.lib.lb_last_error().decode()
comms = lb.world(2)
a = np.arange(10, dtype=np.uint8)
out["send_without_hip"] = lb.lib.ncclSend(a.ctypes.data_as(C.c_void_p), C.c_size_t(10), 0, 1, C.c_void_p(comms[0]), None)
out["global"] = lb.bound_in_global_scope()
"""

CHILD2 = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import _loopback as L
fake = C.CDLL(sys.argv[1])                                  # the host-memory twin, loaded as a HIP runtime would be
lb = L.Loopback()
l = lb.lib
assert l.lb_bind_hip() == 0, l.lb_last_error()
assert lb.bound_in_global_scope()
p = lambda a: a.ctypes.data_as(C.c_void_p)
send = lambda a, n, peer, comm: l.ncclSend(p(a), C.c_size_t(n), 0, peer, C.c_void_p(comm), None)
recv = lambda a, n, peer, comm: l.ncclRecv(p(a), C.c_size_t(n), 0, peer, C.c_void_p(comm), None)
out = {}
# ---- two ranks swap 10 and 6 bytes and each sends to itself, two passes
c = lb.world(2)
src = [np.arange(10, dtype=np.uint8), np.arange(6, dtype=np.uint8) + 50]
dst = [np.full(32, 255, np.uint8), np.full(32, 255, np.uint8)]
def rank(r):
    lb.call_begin()
    n_me, n_peer = (10, 6) if r == 0 else (6, 10)
    assert l.ncclGroupStart() == 0
    assert recv(dst[r][16:], n_me, r, c[r]) == 0           # posted before the send to oneself: served at the group's end
    assert send(src[r], n_me, r, c[r]) == 0
    assert send(src[r], n_me, 1 - r, c[r]) == 0
    assert recv(dst[r], n_peer, 1 - r, c[r]) == 0
    assert l.ncclGroupEnd() == 0
rank(0)
out["after_rank0_deposit"] = [lb.counters()["unmatched"], dst[0][:6].tolist(), dst[0][16:18].tolist()]
rank(1)
out["deposit"] = lb.counters()
lb.deliver()
for d in dst:
    d[:] = 255
rank(0); rank(1)
out["deliver"] = lb.counters()
out["violations"] = L.plan_violations(lb.log(), lb.counters(), 2)
out["dst0"], out["dst1"] = dst[0].tolist(), dst[1].tolist()
# ---- a receive of the wrong size: a non-zero result, counted, nothing written; an ungrouped receive from nobody
c = lb.world(3)
lb.deliver()
lb.call_begin()
l.ncclGroupStart(); send(src[0], 10, 1, c[0]); l.ncclGroupEnd()
d = np.full(16, 255, np.uint8)
lb.call_begin()
l.ncclGroupStart(); rc = recv(d, 8, 0, c[1]); l.ncclGroupEnd()
out["mismatch"] = [rc, lb.counters()["mismatches"], d.tolist() == [255] * 16]
out["ungrouped"] = [recv(d, 8, 2, c[1]), lb.counters()["ungrouped"], lb.counters()["unmatched"], d.tolist() == [255] * 16]
out["mismatch_violations"] = L.plan_violations(lb.log(), lb.counters(), 3)
# ---- a handle that is not the stand-in's, a handle of an earlier world, a peer out of range
old = c[0]
c = lb.world(2)
junk = (C.c_char * 64)()
out["bad_comm"] = [l.ncclSend(p(src[0]), C.c_size_t(4), 0, 0, C.cast(junk, C.c_void_p), None),
                   l.ncclSend(p(src[0]), C.c_size_t(4), 0, 0, None, None), send(src[0], 4, 2, c[0]), lb.counters()["bad_comm"]]
# ---- all-reduce: deposit leaves the buffers alone, deliver writes the sum
c = lb.world(3)
ins = [np.array([1, -5, 2 ** 30], np.int32), np.array([10, 5, 2 ** 30], np.int32), np.array([100, -7, 3], np.int32)]
buf = [a.copy() for a in ins]
ar = lambda r: l.ncclAllReduce(p(buf[r]), p(buf[r]), C.c_size_t(3), 2, 0, C.c_void_p(c[r]), None)
out["ar_deposit"] = [ar(r) for r in range(3)] + [all((buf[r] == ins[r]).all() for r in range(3))]
lb.deliver()
out["ar_deliver"] = [ar(r) for r in range(3)] + [b.tolist() for b in buf]
out["ar_float_refused"] = l.ncclAllReduce(p(buf[0]), p(buf[0]), C.c_size_t(3), 7, 0, C.c_void_p(c[0]), None)
# ---- a rank that never deposited: the deliver pass of the others reports it instead of waiting for it
c = lb.world(2)
lb.deliver()
out["ar_missing"] = [l.ncclAllReduce(p(buf[0]), p(buf[0]), C.c_size_t(3), 2, 0, C.c_void_p(c[0]), None), lb.counters()["unmatched"]]
print(json.dumps(out))
"""


def _run(tmp_path, script, *args):
    r = subprocess.run([sys.executable, "-c", script, *args, L.HERE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_stand_in_compiles_and_refuses_to_work_without_the_process_hip_runtime(tmp_path):
    r = _run(tmp_path, CHILD + "print(json.dumps(out))", "-")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["unbound"] == -1 and "no HIP runtime" in out["unbound_msg"]
    assert out["send_without_hip"] != 0 and out["global"] is True


def test_stand_in_semantics_on_host_memory(tmp_path):
    src, so = tmp_path / "fake_hip.c", tmp_path / "libamdhip64_hostmem.so"
    src.write_text(FAKE_HIP)
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", str(src), "-o", str(so)])
    r = _run(tmp_path, CHILD2, str(so))
    out = json.loads(r.stdout.strip().splitlines()[-1])
    # deposit: rank 0 met an empty slot from rank 1 (counted, nothing written) and was served its own message
    assert out["after_rank0_deposit"] == [1, [255] * 6, [0, 1]]
    assert out["deposit"]["unmatched"] == 1 and out["deposit"]["sends"] == 4
    d = out["deliver"]
    assert (d["sends"], d["recvs"], d["send_bytes"], d["recv_bytes"], d["groups"], d["unmatched"]) == (4, 4, 32, 32, 2, 0)
    assert out["violations"] == []
    assert out["dst0"] == [50, 51, 52, 53, 54, 55] + [255] * 10 + list(range(10)) + [255] * 6
    assert out["dst1"] == list(range(10)) + [255] * 6 + [50, 51, 52, 53, 54, 55] + [255] * 10
    assert out["mismatch"] == [4, 1, True]
    assert out["ungrouped"] == [0, 1, 1, True]
    assert any(b.startswith("unmatched") for b in out["mismatch_violations"]) and any(b.startswith("mismatches") for b in out["mismatch_violations"])
    assert out["bad_comm"] == [4, 4, 4, 2]
    assert out["ar_deposit"] == [0, 0, 0, True]
    s = [111, -7, (2 ** 31 + 3) - 2 ** 32]                  # int32 wraps, as on the device
    assert out["ar_deliver"] == [0, 0, 0, s, s, s]
    assert out["ar_float_refused"] == 4
    assert out["ar_missing"][0] != 0 and out["ar_missing"][1] == 1
