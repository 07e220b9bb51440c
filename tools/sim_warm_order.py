"""What the hand-over order of the eigenvectors is worth to a warm-started one-sided Jacobi: a numpy model of the wave kernel's
iteration (letkf_jacobi_dev.h: odd-even transposition on a line, rotate and swap, the kernel's tangent formula, both stop rules
checked once per step pair) run up the columns of a bench workload, every level warm-started from the level below.

Q is handed over in the order its columns sit on the line when the iteration stops ("sit": what the kernel did before
LETKF_WARM_SORT), sorted by eigenvalue, descending, columns without an eigenvector (the inert zero column of an odd k) last
("sorted": letkf_wave_dev.h warm_rank), or sorted with rank r at position r ^ 1 ("pair": LETKF_WARM_ORDER -- a column that
starts at an even position travels right and one at an odd position left, so ranks (2m, 2m+1) meet in step 1 either way, but
(2m+1, 2m+2) meet at the end of the cycle when sorted and in step 2 when paired; valid columns only, an unpaired last valid
rank keeps its position).  Printed: the mean of ceil(step pairs / S) over the warm-started points -- the kernel's
nsweep -- and the mean of step pairs / S, for every order and both stop rules (early: a quiet cycle at |cos| <= 1e-8 and
|t| <= 1e-6 ends the iteration as well; strict: only the 1e-12 rule).  CPU only; the absolute counts are the model's, the
difference between the orders is what it is for.

Usage: tools/sim_warm_order.py [WORKLOAD=C2-mini] [NCOL=5] [SEED=1] [--json]
  WORKLOAD  a name of bench_workload.CONFIGS, or C2-sim / C2-k20-sim: C2's / C2-k20's lattice and 60 levels on a 20 x 20 grid"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench_workload as bw

ROT_TOL2, STOP_TOL2, EARLY_TOL2, EARLY_T = 1e-30, 1e-24, 1e-16, 1e-6


def jacobi(G, early, max_sweep=60):
    """G: [k, ncol] columns in line order (ncol even).  Returns (step pairs done, G in final line order)."""
    ncol = G.shape[1]
    S = ncol // 2
    quiet = quiet2 = pairs = 0
    for _ in range(max_sweep * S):
        nc = nc2 = False
        for start in (0, 1):
            lo = np.arange(start, ncol - 1, 2)
            x, y = G[:, lo], G[:, lo + 1]
            a, b, ga = (x * x).sum(0), (y * y).sum(0), (x * y).sum(0)
            g2, ab = ga * ga, a * b
            rot = g2 > ROT_TOL2 * ab
            h = 0.5 * (b - a)
            den = np.abs(h) + np.sqrt(h * h + g2)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(rot, ga / np.copysign(den, h), 0.0)
            c = 1.0 / np.sqrt(1.0 + t * t)
            nc |= bool((g2 > STOP_TOL2 * ab).any())
            nc2 |= bool((g2 > EARLY_TOL2 * ab).any() or (np.abs(t) > EARLY_T).any())
            # rotate and swap: the lower position takes c (y + t x), the upper one c (x - t y)
            G[:, lo], G[:, lo + 1] = c * (y + t * x), c * (x - t * y)
        pairs += 1
        quiet = 0 if nc else quiet + 1
        quiet2 = 0 if nc2 else quiet2 + 1
        if quiet >= S or (early and quiet2 >= S):
            break
    return pairs, G


MODES = ("sit", "sorted", "pair")


def hand_over_order(lam, valid, mode):
    """order[p]: the column (line position when the iteration stopped) that the next point finds at position p."""
    ncol = len(lam)
    if mode == "sit":
        return np.arange(ncol)
    order = np.lexsort((np.arange(ncol), -lam, ~valid))   # valid first, eigenvalue descending, ties by position
    if mode == "pair":
        nvalid = int(valid.sum())
        pos = np.arange(ncol)
        pos = np.where((pos | 1) < nvalid, pos ^ 1, pos)      # position of rank r; ranks >= nvalid and an unpaired last one stay
        out = np.empty(ncol, dtype=order.dtype)
        out[pos] = order
        order = out
    return order


def hand_over(G, mode):
    """Normalised columns of G in the order the next point starts from."""
    lam = np.sqrt((G * G).sum(0))
    valid = lam > 0.0
    Q = G * np.where(valid, 1.0 / np.where(valid, lam, 1.0), 0.0)
    return Q[:, hand_over_order(lam, valid, mode)]


def simulate(name, ncols, seed=1, modes=MODES):
    if name.endswith("-sim"):     # the full-size workload's lattice and levels on a small horizontal grid
        bw.CONFIGS[name] = dict(bw.CONFIGS[name[:-4]], nx=20, ny=20)
    w = bw.build(name, torch.device("cpu"))
    k, cfg = w["k"], w["cfg"]
    nij, nz = cfg["nx"] * cfg["ny"], cfg["nz"]
    ncol = (k + 1) & ~1
    S = ncol // 2
    ens = w["ensval"][:, :k].numpy()
    off, idx, rdiag = w["obs_off"].numpy(), w["obs_idx"].numpy(), w["rdiag"].numpy()

    def amat(p):
        o0, o1 = int(off[p]), int(off[p + 1])
        Y = ens[idx[o0:o1]]
        A = (Y / rdiag[o0:o1, None]).T @ Y
        A[np.diag_indices(k)] += k - 1.0
        return A, o1 - o0

    cols = np.random.default_rng(seed).choice(nij, ncols, replace=False)
    res = {}
    for early in (True, False):
        for mode in modes:
            sweeps, frac = [], []
            for col in cols:
                Q = None
                for lev in range(nz):
                    A, n = amat(col + nij * lev)
                    if n == 0:            # a point without observations hands nothing on: the next one starts cold
                        Q = None
                        continue
                    G0 = np.zeros((k, ncol))
                    G0[:, :k] = A
                    if Q is not None:
                        G0 = A @ Q
                    pairs, G = jacobi(G0, early)
                    if Q is not None:
                        sweeps.append(math.ceil(pairs / S))
                        frac.append(pairs / S)
                    Q = hand_over(G, mode)
            res[("early" if early else "strict", mode)] = (float(np.mean(sweeps)), float(np.mean(frac)), len(sweeps))
    return dict(workload=name, k=k, columns=int(ncols), levels=nz, n_mean=w["n_mean"],
                **{f"{rule}_{mode}": dict(nsweep_mean=v[0], cycles_mean=v[1], points=v[2]) for (rule, mode), v in res.items()})


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    r = simulate(args[0] if args else "C2-mini", int(args[1]) if len(args) > 1 else 5, int(args[2]) if len(args) > 2 else 1)
    if "--json" in sys.argv:
        print(json.dumps(r))
    else:
        print(f"{r['workload']}: k = {r['k']}, {r['columns']} columns x {r['levels']} levels, mean n = {r['n_mean']:.1f}")
        for rule in ("early", "strict"):
            a, b, c = r[f"{rule}_sit"], r[f"{rule}_sorted"], r[f"{rule}_pair"]
            print(f"  {rule:6s} stop rule, {a['points']} warm points: nsweep as they sit {a['nsweep_mean']:.3f}, sorted {b['nsweep_mean']:.3f} "
                  f"({100 * (b['nsweep_mean'] / a['nsweep_mean'] - 1):+.1f} %), rank ^ 1 {c['nsweep_mean']:.3f}; "
                  f"cycles {a['cycles_mean']:.3f} -> {b['cycles_mean']:.3f} -> {c['cycles_mean']:.3f}")
