"""The multi-rank exchange entries (C ABI section 8) run with more than one rank on ONE GPU: a loop-back stand-in for RCCL
(tests/native/rccl_loopback.c) behind the library's run-time binding.  R simulated ranks are R contexts in one fresh
child process, called one after the other in two passes (deposit, then deliver: see the C file); what the deliver pass
wrote is compared bit for bit with the definition, and what every rank posted is compared with the plan the definition
implies -- a send nobody receives would be a hang on the real thing, here it is a counter.

What this is not: no RCCL, no xGMI, no concurrency.  It proves index arithmetic and ordering on one stream; that RCCL
comes up on N devices is proved by tests/test_gpu_exchange.py (one rank) and by a real multi-device run only.

This module holds (a) the build of the stand-in, (b) the pure-Python side -- cases, expected results, plan checks (CPU
tested by tests/test_loopback_plan.py) -- and (c) the child's driver, run as `python tests/_loopback.py`, which prints one
JSON line of results (tests/test_gpu_exchange_ranks.py reads it)."""
import collections
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rccl_loopback.c")
SO = os.path.join(HERE, "native", "librccl_loopback.so")
COUNTERS = ("sends", "recvs", "send_bytes", "recv_bytes", "groups", "unmatched", "mismatches", "ungrouped", "overwrites",
            "allreduces", "bad_comm", "hip_errors", "log_dropped")
MUST_BE_ZERO = ("unmatched", "mismatches", "ungrouped", "overwrites", "bad_comm", "hip_errors", "log_dropped")
SENTINEL = 0xA5
RESULT_MARK = "LOOPBACK-RESULTS "


def build_so():
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < os.path.getmtime(SRC):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-Wall", "-o", SO, SRC, "-ldl"])
    return SO


class Loopback:
    """The stand-in, loaded RTLD_GLOBAL: do this in a fresh process BEFORE the library's first exchange call."""

    def __init__(self):
        self.lib = l = C.CDLL(build_so(), mode=C.RTLD_GLOBAL)
        l.lb_comm_of.restype = C.c_void_p
        l.lb_call_begin.restype = C.c_long
        l.lb_log_size.restype = C.c_long
        l.lb_last_error.restype = C.c_char_p
        l.lb_hip_path.restype = C.c_char_p
        assert l.lb_ncounters() == len(COUNTERS)

    def world(self, nranks):
        """a new world in the deposit pass; returns one communicator handle (an integer) per rank"""
        w = self.lib.lb_world_begin(C.c_int(nranks))
        assert w > 0, nranks
        comms = [self.lib.lb_comm_of(C.c_int(w), C.c_int(r)) for r in range(nranks)]
        assert all(comms)
        return comms

    def deliver(self):
        self.lib.lb_deliver()

    def call_begin(self):
        return self.lib.lb_call_begin()

    def counters(self):
        a = (C.c_int64 * len(COUNTERS))()
        self.lib.lb_counters(a)
        return dict(zip(COUNTERS, [int(v) for v in a]))

    def log(self):
        """[(kind, src, dst, bytes, depth, group, call)], kind 0 = send, 1 = receive"""
        out = []
        e = (C.c_int64 * 7)()
        for i in range(self.lib.lb_log_size()):
            self.lib.lb_log_get(C.c_long(i), e)
            out.append(tuple(int(v) for v in e))
        return out

    def bound_in_global_scope(self):
        """the ncclSend (and the rest) that a dlsym on the process image finds is the stand-in's own"""
        g = C.CDLL(None)
        for name in ("ncclSend", "ncclRecv", "ncclGroupStart", "ncclGroupEnd", "ncclAllReduce", "ncclGetErrorString"):
            mine = C.cast(getattr(self.lib, name), C.c_void_p).value
            seen = C.cast(getattr(g, name), C.c_void_p).value
            if mine is None or mine != seen:
                return False
        return True


# ----------------------------------------------------------------------------------------------------------------------
# the pure-Python side: plan checks

def plan_violations(log, counters, ncalls, expect=None):
    """What is wrong with the deliver pass of one entry, as a list of sentences (empty = a plan that would neither hang
    nor corrupt).  log / counters: Loopback.log() / .counters() after the pass; ncalls: entry calls made in it;
    expect: the multiset (collections.Counter) of (src, dst, bytes) the definition implies, or None."""
    bad = [f"{k} = {counters[k]}" for k in MUST_BE_ZERO if counters.get(k, 0) != 0]
    sends = collections.Counter((s, d, n) for kind, s, d, n, *_ in log if kind == 0)
    recvs = collections.Counter((s, d, n) for kind, s, d, n, *_ in log if kind == 1)
    if sum(sends.values()) != counters["sends"] or sum(recvs.values()) != counters["recvs"]:
        bad.append("the log and the counters disagree")
    if sends != recvs:
        bad.append(f"sent but not received: {sorted((sends - recvs).elements())}; received but not sent: "
                   f"{sorted((recvs - sends).elements())}")
    if expect is not None and sends != expect:
        bad.append(f"sends missing from the plan: {sorted((expect - sends).elements())}; sends beyond it: "
                   f"{sorted((sends - expect).elements())}")
    by_call, by_group = collections.defaultdict(set), collections.defaultdict(set)
    for kind, s, d, n, depth, group, call in log:
        if depth != 1:
            bad.append(f"{'send' if kind == 0 else 'receive'} {s} -> {d} posted at group depth {depth}")
        by_call[call].add(group)
        by_group[group].add(call)
    if any(len(g) != 1 for g in by_call.values()):
        bad.append("an entry call spread its operations over more than one group")
    if any(len(c) != 1 for c in by_group.values()):
        bad.append("one group spans more than one entry call")
    if counters["groups"] > ncalls:
        bad.append(f"{counters['groups']} groups in {ncalls} entry calls")
    return bad


# ----------------------------------------------------------------------------------------------------------------------
# letkf_members_alltoall_dev

def share(nxy, r, nranks):
    """number of subdomain points r, r + nranks, ... < nxy (nij1node of common_mpi_scale.f90:264-283)"""
    return len(range(r, nxy, nranks))


def strides(kind, nij1, nlev, nens):
    """(sp, sm, sv) of the state; element (i, lev, m, v) at (i + nij1*lev)*sp + m*sm + v*sv"""
    if kind == "point":
        return 1, nlev * nij1, nens * nlev * nij1
    assert kind == "member"
    return nens, 1, nens * nlev * nij1


def member_field(seed, m, nlev, nlon, nlat, nv3d):
    """v3dg(nlev,nlon,nlat,nv3d) of member m, level-fastest, flat"""
    return np.random.default_rng([seed, m]).standard_normal(nv3d * nlat * nlon * nlev)


def expected_state(fields, nlev, nlon, nlat, nv3d, nens, nranks, p, sp, sm, sv):
    """rank p's state by the definition: point i of rank p is subdomain point p + nranks*i, member m in its slot; NaN
    wherever nobody wrote.  fields: {member: flat field}."""
    nxy = nlon * nlat
    pts = np.arange(p, nxy, nranks)
    nij1 = len(pts)
    x = np.full(nv3d * nens * nlev * nij1, np.nan)
    i, lev, v = np.meshgrid(np.arange(nij1), np.arange(nlev), np.arange(nv3d), indexing="ij")
    for m, f in fields.items():
        f = f.reshape(nv3d, nxy, nlev)
        x[(i + nij1 * lev) * sp + m * sm + v * sv] = f[v, pts[i], lev]
    return x


def members_plan(direction, nranks, nxy, nlev, nv3d, mcount):
    """the messages of one scatter (dir 0) / gather (dir 1): holder s <-> every other rank d that owns points"""
    plan = collections.Counter()
    for s in range(mcount):
        for d in range(nranks):
            n = 8 * nv3d * nlev * share(nxy, d, nranks)
            if d != s and n > 0:
                plan[(s, d, n) if direction == 0 else (d, s, n)] += 1
    return plan


def members_cases():
    """grids 13x7 (91 points: not divisible by 2, 3, 4, 8) and 16x8 on 2, 3, 4, 8 ranks, 3x2 on 4 and on 8 ranks (8: ranks
    6 and 7 own no point); a full batch, a short last batch, one member and none; nlev 1 / 9, nv3d 1 / 3, mstart 0 and > 0
    with more slots than are filled; the point-fastest and the member-fastest stride triple."""
    out = []
    shapes = [(1, 1, 0), (9, 3, 2), (9, 1, 0), (1, 3, 1)]               # (nlev, nv3d, mstart)
    worlds = [(g, r) for g in ((13, 7), (16, 8)) for r in (2, 3, 4, 8)] + [((3, 2), 4), ((3, 2), 8)]
    for (nlon, nlat), nranks in worlds:
        for mcount in sorted({nranks, nranks - 1, 1, 0}):
            for kind in ("point", "member"):
                for nlev, nv3d, mstart in shapes:
                    out.append(dict(nlon=nlon, nlat=nlat, nranks=nranks, mcount=mcount, stride=kind, nlev=nlev, nv3d=nv3d,
                                    mstart=mstart, nens=mstart + nranks + 2))
    for c in out:
        c["id"] = "members-{nlon}x{nlat}-r{nranks}-mc{mcount}-{stride}-lev{nlev}-v{nv3d}-ms{mstart}".format(**c)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# letkf_alltoallv_dev

def alltoallv_layout(M, seed):
    """Offsets (in rows) for the send matrix M[s][d]: blocks in a shuffled rank order with gaps between them.
    Returns per rank dict(soff, roff, nsend, nrecv): offsets per peer and the buffer sizes in rows."""
    rng = np.random.default_rng(seed)
    n = len(M)
    out = []
    for me in range(n):
        lay = {}
        for key, cnt in (("s", [M[me][d] for d in range(n)]), ("r", [M[s][me] for s in range(n)])):
            off, at = [0] * n, int(rng.integers(0, 3))
            for q in rng.permutation(n):
                off[q] = at
                at += cnt[q] + int(rng.integers(0, 4))
            lay[key + "off"], lay["n" + ("send" if key == "s" else "recv")] = off, at + 1
        out.append(lay)
    return out


def alltoallv_expected(M, lay, row_bytes, sends, me):
    """rank me's receive buffer (uint8): the senders' rows at its receive offsets, the sentinel everywhere else"""
    exp = np.full(lay[me]["nrecv"] * row_bytes, SENTINEL, np.uint8)
    for s in range(len(M)):
        a, b = lay[me]["roff"][s] * row_bytes, lay[s]["soff"][me] * row_bytes
        exp[a:a + M[s][me] * row_bytes] = sends[s][b:b + M[s][me] * row_bytes]
    return exp


def alltoallv_plan(M, row_bytes):
    n = len(M)
    return collections.Counter((s, d, M[s][d] * row_bytes) for s in range(n) for d in range(n) if s != d and M[s][d] > 0)


def random_matrix(n, seed):
    """zero rows, zero columns, an all-zero rank (n >= 3), own blocks of zero and non-zero size"""
    rng = np.random.default_rng(seed)
    M = rng.integers(0, 7, (n, n))
    M[rng.random((n, n)) < 0.2] = 1                                       # single rows: the smallest message
    for q in range(n):
        M[q, q] = 0 if q % 2 == 0 else 3
    if n >= 3:
        z, r1, c1 = rng.permutation(n)[:3]
        M[z, :] = 0                                                       # rank z neither sends nor receives, itself included
        M[:, z] = 0
        M[r1, np.arange(n) != r1] = 0                                     # r1 sends to nobody else, c1 receives from nobody else
        M[np.arange(n) != c1, c1] = 0
    return [[int(v) for v in row] for row in M]


def halo_matrix(px=3, py=3, seed=5):
    """each rank receives from its (up to 8) neighbours of a px x py world and keeps its own rows"""
    rng = np.random.default_rng(seed)
    n = px * py
    M = [[0] * n for _ in range(n)]
    for s in range(n):
        for d in range(n):
            if max(abs(s % px - d % px), abs(s // px - d // px)) <= 1:
                M[s][d] = int(rng.integers(1, 9))
    return M


def alltoallv_cases():
    out = []
    for n, rb in itertools.product(range(2, 7), (4, 8, 408)):
        out.append(dict(id=f"alltoallv-random-r{n}-rb{rb}", M=random_matrix(n, 100 * n + rb), row_bytes=rb, seed=n + rb))
    out.append(dict(id="alltoallv-halo-3x3", M=halo_matrix(), row_bytes=408, seed=9))
    out.append(dict(id="alltoallv-equal-blocks-r4", M=[[11] * 4 for _ in range(4)], row_bytes=8 * 30, seed=4))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# letkf_obs_allgatherv_dev, letkf_allreduce_sum_i32_dev

def allgatherv_cases():
    return [dict(id=f"allgatherv-{'_'.join(map(str, c))}-rb{rb}", counts=c, row_bytes=rb)
            for c in ([5, 0, 7, 3], [0, 0, 0, 9], [1, 1]) for rb in (408, 4)]


def allgatherv_plan(counts, row_bytes):
    """every rank that has rows sends them to every rank, itself included"""
    n = len(counts)
    return collections.Counter((s, d, counts[s] * row_bytes) for s in range(n) for d in range(n) if counts[s] > 0)


def allreduce_cases():
    return [dict(id=f"allreduce-r{n}-n{cnt}", nranks=n, count=cnt) for n in (2, 4) for cnt in (0, 1, 1000)]


def allreduce_inputs(nranks, count, seed=77):
    rng = np.random.default_rng([seed, nranks, count])
    return [rng.integers(-10 ** 6, 10 ** 6, count).astype(np.int32) for _ in range(nranks)]


def all_case_ids():
    return ([c["id"] for c in members_cases() + alltoallv_cases()] + ["alltoallv-own-block-refused"] +
            [c["id"] for c in allgatherv_cases() + allreduce_cases()] + ["setobs-2x2", "setobs-3x2"])


# ----------------------------------------------------------------------------------------------------------------------
# the child's driver (GPU)

class Driver:
    def __init__(self, lb):
        import torch
        from _gpu import pkg
        self.torch, self.pkg, self.lb = torch, pkg, lb
        pkg.build()
        self._ctx = []

    def ctxs(self, n):
        """one library context per simulated rank, all on the process's current stream"""
        while len(self._ctx) < n:
            self._ctx.append(self.pkg.Context(0, self.torch.cuda.current_stream().cuda_stream))
        return self._ctx[:n]

    def two_pass(self, nranks, call, refill, expect, moves=True):
        """`call(rank, comm)` for every rank (deposit), switch, `refill()`, every rank again (deliver).  Returns the
        counters of the deliver pass after the plan checks."""
        torch, lb = self.torch, self.lb
        comms = lb.world(nranks)
        for phase in (0, 1):
            for r in range(nranks):
                lb.call_begin()
                call(r, comms[r])
                torch.cuda.synchronize()
            if phase == 0:
                lb.deliver()
                refill()
                torch.cuda.synchronize()
        cnt = lb.counters()
        bad = plan_violations(lb.log(), cnt, nranks, expect)
        assert not bad, "; ".join(bad)
        if moves:
            assert cnt["sends"] > 0, "data had to move between two ranks, yet the stand-in saw no send"
        else:
            assert cnt["sends"] == cnt["recvs"] == cnt["groups"] == cnt["allreduces"] == 0 and not lb.log(), cnt
        return cnt

    # ---- letkf_members_alltoall_dev
    def members(self, c):
        import _oracle
        torch = self.torch
        R, nlev, nlon, nlat, nv3d, ms, mc, nens = (c[k] for k in ("nranks", "nlev", "nlon", "nlat", "nv3d", "mstart", "mcount", "nens"))
        nxy = nlon * nlat
        ctxs = self.ctxs(R)
        nij1 = [share(nxy, p, R) for p in range(R)]
        st = [strides(c["stride"], nij1[p], nlev, nens) for p in range(R)]
        fields = {ms + s: member_field(31, ms + s, nlev, nlon, nlat, nv3d) for s in range(mc)}
        fd = [torch.from_numpy(fields[ms + p]).cuda() if p < mc else None for p in range(R)]
        nan = float("nan")
        x = [torch.full((nv3d * nens * nlev * nij1[p],), nan, dtype=torch.float64, device="cuda") for p in range(R)]
        assert all((t.data_ptr() == 0) == (nij1[p] == 0) for p, t in enumerate(x))      # a rank without points: x is NULL
        totals = collections.Counter()

        def run(direction, v3dg, refill):
            cnt = self.two_pass(R, lambda p, comm: ctxs[p].members_alltoall(comm, R, p, direction, nlev, nlon, nlat, nv3d, ms, mc,
                                                                           v3dg[p], x[p], *st[p]),
                                refill, members_plan(direction, R, nxy, nlev, nv3d, mc), moves=mc > 0)
            totals.update(cnt)

        run(0, fd, lambda: [t.fill_(nan) for t in x])
        o = _oracle.oracle()
        exp = []
        for p in range(R):
            e = expected_state(fields, nlev, nlon, nlat, nv3d, nens, R, p, *st[p])
            got = x[p].cpu().numpy()
            assert np.array_equal(got, e, equal_nan=True), f"dir 0, rank {p}: the state differs from the definition"
            xo = np.full_like(e, np.nan)
            if nij1[p]:
                for m, f in fields.items():
                    o.orc_member_points(C.c_int(0), C.c_int(nlev), C.c_int(nlon), C.c_int(nlat), C.c_int(nv3d), C.c_int(R),
                                        C.c_int(p), C.c_int(m), _oracle._dp(f), _oracle._dp(xo), C.c_int64(nij1[p]),
                                        *[C.c_int64(v) for v in st[p]])
            assert np.array_equal(got, xo, equal_nan=True), f"dir 0, rank {p}: the state differs from orc_member_points"
            exp.append(e)
        # dir 1 on that state: every holder gets its field back, a non-holder's v3dg is not written
        back = [torch.full((nv3d * nxy * nlev,), nan, dtype=torch.float64, device="cuda") for _ in range(R)]
        run(1, back, lambda: [t.fill_(nan) for t in back])
        for p in range(R):
            b = back[p].cpu().numpy()
            if p < mc:
                assert np.array_equal(b, fields[ms + p]), f"dir 1, rank {p}: the field did not come back"
            else:
                assert np.isnan(b).all(), f"dir 1, rank {p} holds no member, yet its v3dg was written"
            assert np.array_equal(x[p].cpu().numpy(), exp[p], equal_nan=True), f"dir 1 changed the state of rank {p}"
        return dict(totals)

    # ---- letkf_alltoallv_dev
    def alltoallv(self, c):
        torch = self.torch
        M, rb = c["M"], c["row_bytes"]
        n = len(M)
        ctxs = self.ctxs(n)
        lay = alltoallv_layout(M, c["seed"])
        rng = np.random.default_rng(c["seed"] + 1000)
        sends = [rng.integers(0, 256, lay[r]["nsend"] * rb).astype(np.uint8) for r in range(n)]
        sd = [torch.from_numpy(s).cuda() for s in sends]
        rd = [torch.full((lay[r]["nrecv"] * rb,), SENTINEL, dtype=torch.uint8, device="cuda") for r in range(n)]
        moves = any(M[s][d] for s in range(n) for d in range(n) if s != d)
        cnt = self.two_pass(n, lambda r, comm: ctxs[r].alltoallv(comm, r, M[r], lay[r]["soff"], [M[s][r] for s in range(n)],
                                                                 lay[r]["roff"], rb, sd[r], rd[r]),
                            lambda: [t.fill_(SENTINEL) for t in rd], alltoallv_plan(M, rb), moves=moves)
        for r in range(n):
            assert np.array_equal(rd[r].cpu().numpy(), alltoallv_expected(M, lay, rb, sends, r)), f"rank {r}: receive buffer"
            assert np.array_equal(sd[r].cpu().numpy(), sends[r]), f"rank {r}: the send buffer was written"
        return cnt

    def alltoallv_refused(self):
        """send and receive counts of the own block differ: an error code and a message, nothing posted"""
        torch, lb = self.torch, self.lb
        ctxs = self.ctxs(2)
        comms = lb.world(2)
        lb.deliver()
        send = torch.zeros(64, dtype=torch.uint8, device="cuda")
        recv = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
        try:
            ctxs[0].alltoallv(comms[0], 0, [2, 1], [0, 2], [3, 1], [0, 3], 8, send, recv)
        except self.pkg.LetkfError as e:
            assert str(e).startswith("letkf_amd error -1:") and "own block" in str(e), str(e)   # LETKF_E_INVALID
        else:
            raise AssertionError("send_counts[myrank] != recv_counts[myrank] was accepted")
        torch.cuda.synchronize()
        cnt = lb.counters()
        assert not any(cnt.values()) and not lb.log(), cnt
        assert bool((recv == SENTINEL).all())
        return cnt

    # ---- letkf_obs_allgatherv_dev
    def allgatherv_raw(self, ctx, comm, me, counts, row_bytes, send_ptr, recv_ptr):
        n = len(counts)
        ctx._check(ctx._l.letkf_obs_allgatherv_dev(ctx._c, C.c_void_p(comm), C.c_int32(n), C.c_int32(me), (C.c_int64 * n)(*counts),
                                                   C.c_int64(row_bytes), C.c_void_p(send_ptr), C.c_void_p(recv_ptr)))

    def allgatherv(self, c):
        torch = self.torch
        counts, rb = c["counts"], c["row_bytes"]
        n, total = len(counts), sum(counts)
        ctxs = self.ctxs(n)
        rng = np.random.default_rng(sum(counts) + rb)
        sends = [rng.integers(0, 256, counts[r] * rb).astype(np.uint8) for r in range(n)]
        sd = [torch.from_numpy(s).cuda() if len(s) else None for s in sends]
        rd = [torch.full(((total + 3) * rb,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(n)]
        cnt = self.two_pass(n, lambda r, comm: self.allgatherv_raw(ctxs[r], comm, r, counts, rb,
                                                                   sd[r].data_ptr() if sd[r] is not None else None, rd[r].data_ptr()),
                            lambda: [t.fill_(SENTINEL) for t in rd], allgatherv_plan(counts, rb), moves=total > 0)
        exp = np.concatenate(sends + [np.full(3 * rb, SENTINEL, np.uint8)])
        for r in range(n):
            assert np.array_equal(rd[r].cpu().numpy(), exp), f"rank {r}: not the rank-major concatenation"
        return cnt

    # ---- letkf_allreduce_sum_i32_dev
    def allreduce(self, c):
        torch, lb = self.torch, self.lb
        n, count = c["nranks"], c["count"]
        ctxs = self.ctxs(n)
        ins = allreduce_inputs(n, count)
        bufs = [torch.from_numpy(a.copy()).cuda() for a in ins]

        def refill():                                   # in place: the deposit pass must have left the inputs alone
            for r in range(n):
                assert np.array_equal(bufs[r].cpu().numpy(), ins[r]), f"rank {r}: the deposit pass changed the buffer"
        comms = lb.world(n)
        for phase in (0, 1):
            for r in range(n):
                lb.call_begin()
                ctxs[r].allreduce_sum_i32(comms[r], n, bufs[r])
                torch.cuda.synchronize()
            if phase == 0:
                lb.deliver()
                refill()
        cnt = lb.counters()
        bad = [f"{k} = {cnt[k]}" for k in MUST_BE_ZERO if cnt[k]]
        assert not bad, bad
        assert cnt["allreduces"] == (n if count else 0) and cnt["sends"] == cnt["recvs"] == 0, cnt
        want = sum(a.astype(np.int64) for a in ins).astype(np.int32)
        for r in range(n):
            assert np.array_equal(bufs[r].cpu().numpy(), want), f"rank {r}: not the sum"
        return cnt

    # ---- set_letkf_obs across ranks on the library's own exchanges
    def setobs(self, px, py, seed):
        """local half, all-reduce of tot_sub, all-gather of n_cell and of the sorted send buffers, finish half: the
        composition a host on px*py GPUs runs, checked like tests/test_gpu_setobs.py test_two_by_two_world"""
        import test_gpu_setobs as T
        from _gpu import dev
        from _setobs import make_world, namelist, oracle_local
        torch = self.torch
        nml = namelist()
        w = make_world(seed, px=px, py=py, k=12, det_run=True, nfile_rows=(6000, 3000))
        n = px * py
        ctxs = self.ctxs(n)
        locs = [oracle_local(w, rk, nml) for rk in w["ranks"]]
        gs = []
        for me, rk in enumerate(w["ranks"]):
            g = T.run_local(w, rk, nml, me=me)
            g["_set"], g["_idx"] = rk["set"], rk["idx"]
            conv_file, _, _ = T.check_local(w, g, locs[me])
            gs.append(g)
        infos = [g["tab"].info() for g in gs]
        totals = collections.Counter()
        # (2) tot_sub through the all-reduce
        tot_in = [g["tab"].host()["tot_sub"].astype(np.int32).ravel() for g in gs]
        tot = [dev(a.copy()) for a in tot_in]
        comms = self.lb.world(n)
        for phase in (0, 1):
            for r in range(n):
                self.lb.call_begin()
                ctxs[r].allreduce_sum_i32(comms[r], n, tot[r])
                torch.cuda.synchronize()
            if phase == 0:
                self.lb.deliver()
        cnt = self.lb.counters()
        assert cnt["allreduces"] == n and not any(cnt[k] for k in MUST_BE_ZERO), cnt
        totals.update(cnt)
        # (3) every rank's n_cell row and sorted send buffer through the all-gather, straight from the table's device arrays
        ncell, ld = infos[0].ncell, infos[0].ld_send
        assert all(i.ncell == ncell and i.ld_send == ld for i in infos)
        n_all = [torch.full((n, ncell), -1, dtype=torch.int32, device="cuda") for _ in range(n)]
        totals.update(self.two_pass(n, lambda r, comm: self.allgatherv_raw(ctxs[r], comm, r, [ncell] * n, 4, infos[r].n_cell,
                                                                           n_all[r].data_ptr()),
                                    lambda: [t.fill_(-1) for t in n_all], allgatherv_plan([ncell] * n, 4)))
        ns = [int(i.nsorted) for i in infos]
        recv = [torch.full((sum(ns), ld), float("nan"), dtype=torch.float64, device="cuda") for _ in range(n)]
        totals.update(self.two_pass(n, lambda r, comm: self.allgatherv_raw(ctxs[r], comm, r, ns, ld * 8,
                                                                           infos[r].sendbuf if ns[r] else None, recv[r].data_ptr()),
                                    lambda: [t.fill_(float("nan")) for t in recv], allgatherv_plan(ns, ld * 8)))
        # (4) the finish half, checked against the oracle
        for me, g in enumerate(gs):
            ctxs[me].set_obs_finish(g["tab"], n_all[me], recv[me], tot_g=tot[me])
            torch.cuda.synchronize()
            of = T.finish_conv(w, locs, me, conv_file)
            T.check_finish(w, g["tab"], of, conv_file)
            assert of["nobstotal"] > 0
        for g in gs:
            g["tab"].close()
        return dict(totals)


def main():
    lb = Loopback()                                 # in the process image before torch and before the library
    import torch
    sys.path.insert(0, os.path.dirname(HERE))       # the repo root: __graft_entry__
    assert torch.cuda.is_available()
    # proof of binding, before the first nranks > 1 call: a dlsym on the process image finds the stand-in's own symbols
    assert lb.bound_in_global_scope(), "ncclSend in the global scope is not the loop-back stand-in's"
    drv = Driver(lb)
    torch.zeros(1, device="cuda")
    assert lb.lib.lb_bind_hip() == 0, lb.lib.lb_last_error().decode()
    hip_path = lb.lib.lb_hip_path().decode()
    jobs = ([(c["id"], lambda c=c: drv.members(c)) for c in members_cases()] +
            [(c["id"], lambda c=c: drv.alltoallv(c)) for c in alltoallv_cases()] +
            [("alltoallv-own-block-refused", drv.alltoallv_refused)] +
            [(c["id"], lambda c=c: drv.allgatherv(c)) for c in allgatherv_cases()] +
            [(c["id"], lambda c=c: drv.allreduce(c)) for c in allreduce_cases()] +
            [("setobs-2x2", lambda: drv.setobs(2, 2, 21)), ("setobs-3x2", lambda: drv.setobs(3, 2, 22))])
    assert [j[0] for j in jobs] == all_case_ids()
    results = {}
    for cid, job in jobs:
        try:
            results[cid] = dict(ok=True, counters=job())
        except AssertionError as e:                  # a wrong result: the next case can still run
            results[cid] = dict(ok=False, error=f"{e}"[:2000] or traceback.format_exc()[-2000:], counters=lb.counters())
        except Exception:                            # anything else (an error of the runtime among them): nothing more runs
            results[cid] = dict(ok=False, error=traceback.format_exc()[-3000:], counters=lb.counters())
            break
    print(RESULT_MARK + json.dumps(dict(bound=True, hip=hip_path, results=results)))


if __name__ == "__main__":
    main()
