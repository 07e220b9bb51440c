"""Numpy restatement of das_efso's localisation advection (loc_advection, scale/letkf/efso_tools.f90:158-195, used at
scale/letkf/letkf_tools.f90:1225-1229) in SCALE's grid frame, and synthetic shear winds for the tests.

    c_i = locadv_rate * eft * 3600 / dx,   c_j = locadv_rate * eft * 3600 / dy
    ri[p] = rig[ij] - (0.5 * (u0[p] + u1[p])) * c_i,   rj[p] = rjg[ij] - (0.5 * (v0[p] + v1[p])) * c_j,   p = ij + nij1*lev

Positions are SCALE's fractional global grid indices: no 1/cos(lat), pole reflection or longitude wrap (the reference's
lon/lat grid).  numpy evaluates each operation once in IEEE double, as the device kernel does without fused multiply-adds,
so the two agree bit for bit."""
import numpy as np

MAX_CELLS = 2.0 ** 20


def coefs(locadv_rate, eft, dx, dy):
    """(c_i, c_j) in the order the library computes them: ((rate * eft) * 3600) / dx"""
    return locadv_rate * eft * 3600.0 / dx, locadv_rate * eft * 3600.0 / dy


def advect(rig, rjg, u0, v0, u1, v1, locadv_rate, eft, dx, dy):
    """(ri, rj) [nij1*nlev] for winds [nij1*nlev] (p = ij + nij1*lev)"""
    nij1 = len(rig)
    nlev = len(u0) // nij1
    ci, cj = coefs(locadv_rate, eft, dx, dy)
    ri = np.tile(np.asarray(rig, np.float64), nlev) - (0.5 * (np.asarray(u0) + np.asarray(u1))) * ci
    rj = np.tile(np.asarray(rjg, np.float64), nlev) - (0.5 * (np.asarray(v0) + np.asarray(v1))) * cj
    return ri, rj


def bad_points(rig, rjg, ri, rj):
    """points the library rejects: not finite, or moved by more than 2^20 cells in i or j"""
    nlev = len(ri) // len(rig)
    di = np.abs(ri - np.tile(rig, nlev))
    dj = np.abs(rj - np.tile(rjg, nlev))
    with np.errstate(invalid="ignore"):
        return ~((di <= MAX_CELLS) & (dj <= MAX_CELLS))


def shear_winds(rng, nij1, nlev, u_bot=10.0, u_top=30.0, v=5.0, noise=3.0):
    """(u0, v0, u1, v1) [nij1*nlev] in m/s: a westerly that grows with height (u_bot .. u_top over the levels, the
    profile bench_efso.py --locadv uses), a steady southerly, and two times that differ by noise"""
    lev = np.repeat(np.arange(nlev), nij1)
    u = u_bot + (u_top - u_bot) * lev / max(nlev - 1, 1)
    u0 = u + noise * rng.standard_normal(nij1 * nlev)
    u1 = u + noise * rng.standard_normal(nij1 * nlev)
    v0 = v + noise * rng.standard_normal(nij1 * nlev)
    v1 = v + noise * rng.standard_normal(nij1 * nlev)
    return u0, v0, u1, v1
