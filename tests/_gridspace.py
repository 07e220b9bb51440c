"""The argument space of the grid-side streaming entries (letkf_api_grid.hip; include/letkf_amd.h sections 4 and 7 and row f4):
a plain numpy statement of each operation, written from the reference's lines, the state layouts the strides allow, and the
cases that tests/test_gridspace_helpers.py (statement against the oracle, no GPU) and tests/test_gpu_grid_argspace.py (device
against the statement) share.  No GPU and no oracle is touched here.

Arithmetic is stated in np.longdouble; pure data movement is integer indexing.  Two operations also have a float64 form because
the comparison with the device is bit for bit: the mean (the kernel promises member-order summation) and the set-up passes
relax_beta / infl_init (every operation in them is a single correctly rounded one, so float64 IS the statement)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                                # unit roundoff of binary64
CANARY = 0x7FF4DEADBEEF0001                   # a signalling-NaN bit pattern (tests/_argspace.py): still there = never written
ICANARY = -0x21524111                         # the same idea for int32 outputs
UNDEF = -9.99e33                              # common/common.f90:38
CUT2 = float(np.float32(13.33333333))         # dist_zero_fac_square, a single-precision literal (letkf_obs.f90:28)
ZFAC = float(np.float32(3.651483717))         # dist_zero_fac (letkf_obs.f90:27)
E_INVALID = -1                                # LETKF_E_INVALID


# ------------------------------------------------------------------------------------------------------------------ layouts
LAYOUTS = ("point", "member", "var_mid", "padded", "view")
TAIL = 11                                     # canaries behind the last addressed element of every layout


def layout(name, nv, nens, npts):
    """(sp, sm, sv, offset, size) of a logical [nv, nens, npts] state; element (v, m, p) sits at offset + p*sp + m*sm + v*sv"""
    if name == "point":                       # gues3d(nij1*nlev, nens, nv3d), the reference's
        sp, sm, sv, off = 1, npts, npts * nens, 0
    elif name == "member":                    # member-fastest, then variable, then point
        sp, sm, sv, off = nens * nv, nv, 1, 0
    elif name == "var_mid":                   # point, variable, member
        sp, sm, sv, off = 1, npts * nv, npts, 0
    elif name == "padded":                    # point-fastest with gaps behind every member and every variable
        sm = npts + 3
        sp, sv, off = 1, sm * nens + 5, 0
    elif name == "view":                      # the reference's layout, 17 elements into a larger buffer
        sp, sm, sv, off = 1, npts, npts * nens, 17
    else:
        raise ValueError(name)
    last = (npts - 1) * sp + (nens - 1) * sm + (nv - 1) * sv if npts > 0 else -1
    return sp, sm, sv, off, off + last + 1 + TAIL


def state_index(nv, nens, npts, sp, sm, sv, off):
    v = np.arange(nv)[:, None, None]
    m = np.arange(nens)[None, :, None]
    p = np.arange(npts)[None, None, :]
    return off + p * sp + m * sm + v * sv


def canary_buffer(size, dtype=np.float64):
    if dtype == np.float64:
        return np.full(size, CANARY, dtype=np.int64).view(np.float64)
    return np.full(size, ICANARY, dtype=np.int32)


def place(x3, name):
    """logical x3 [nv, nens, npts] under layout `name` inside a canary buffer: (buffer, offset, sp, sm, sv, mask of the
    addressed elements).  The library gets buffer[offset:]."""
    nv, nens, npts = x3.shape
    sp, sm, sv, off, size = layout(name, nv, nens, npts)
    buf = canary_buffer(size)
    idx = state_index(nv, nens, npts, sp, sm, sv, off)
    buf[idx] = x3
    mask = np.zeros(size, bool)
    mask[idx] = True
    return buf, off, sp, sm, sv, mask


def lift(buf, shape, name):
    """the logical [nv, nens, npts] array back out of a buffer laid out by place()"""
    sp, sm, sv, off, _ = layout(name, *shape)
    return buf[state_index(*shape, sp, sm, sv, off)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def untouched(buf, mask):
    """every element outside the mask still holds the canary's bits"""
    return bool(np.all(bits(buf)[~mask] == CANARY))


# ---------------------------------------------------------------------------------------- mean, perturbations, spread
# common_scale.f90:1513-1552 (ensmean_grd), letkf_tools.f90:209-230, common_scale.f90:1570-1607 (enssprd_grd)
def mean_ld(x3, k):
    return x3[:, :k].astype(LD).sum(axis=1) / LD(k)


def mean_f64(x3, k):
    """member order, as :1529-1533: s = x(1); s = s + x(m); s / mem"""
    s = x3[:, 0].copy()
    for m in range(1, k):
        s += x3[:, m]
    return s / float(k)


def perturbations(x3, k):
    """x(m) - x(mmean): one correctly rounded subtraction each, so float64 is the statement"""
    out = x3.copy()
    out[:, :k] = x3[:, :k] - x3[:, k:k + 1]
    return out


def spread_ld(x3, k):
    """:1588-1592, from the mean the array HOLDS in slot k"""
    d = x3[:, :k].astype(LD) - x3[:, k:k + 1].astype(LD)
    return np.sqrt((d * d).sum(axis=1) / LD(k - 1))


def ens_case(k, nv, npts, seed=0, filled_mean=True):
    """[nv, k+1, npts]: members with a mean 10^3 times their spread (so the spread's subtraction cancels three digits), slot k
    the float64 member-order mean, or -7 where the test is about writing it"""
    rng = np.random.default_rng(1000 * k + 10 * nv + npts + seed)
    s = (1.0 + np.arange(nv))[:, None, None]
    x = np.empty((nv, k + 1, npts))
    x[:, :k] = s * (1000.0 + rng.standard_normal((nv, k, npts)))
    x[:, k] = mean_f64(x, k) if filled_mean else -7.0
    return x


# (k, nv, npts, layout): every value of every axis, every layout with k = 1 and with k = 50
ENS_CASES = [(1, 1, 1, "point"), (1, 11, 255, "member"), (1, 1, 256, "var_mid"), (1, 11, 257, "padded"),
             (1, 1, 1000, "view"), (50, 11, 257, "point"), (50, 1, 1000, "member"), (50, 11, 1, "var_mid"),
             (50, 1, 255, "padded"), (50, 11, 256, "view"), (2, 11, 256, "member"), (2, 1, 1, "padded"),
             (3, 1, 257, "var_mid"), (3, 11, 255, "view"), (100, 1, 1000, "point"), (100, 11, 255, "member")]


def spread_bound(ref, k):
    """(k + 4) u ref: the k squares and k - 1 additions of positive terms lose at most k u of the sum (contracted or not),
    the subtractions are exact or one rounding each, then the division and the root"""
    return (k + 4) * U * np.abs(ref).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- member_points
# grd_to_buf / buf_to_grd, common_mpi_scale.f90:1428-1480: local point i of rank r is subdomain point j = r + np*i
def nij1_of(nxy, np_, rank):
    return (nxy - rank + np_ - 1) // np_


def member_points_fwd(field, nlev, nxy, nv3d, np_, rank):
    """field v3dg(nlev, nlon*nlat, nv3d) flat, level-fastest -> [nv3d, npts], p = i + nij1*k"""
    f = field.reshape(nv3d, nxy, nlev)
    j = np.arange(rank, nxy, np_)
    return np.ascontiguousarray(f[:, j, :].transpose(0, 2, 1)).reshape(nv3d, -1)


def member_points_back(field, xs, nlev, nxy, nv3d, np_, rank):
    """the field after buf_to_grd of xs [nv3d, npts]: the rank's own columns replaced, every other left as it was"""
    out = field.copy().reshape(nv3d, nxy, nlev)
    j = np.arange(rank, nxy, np_)
    out[:, j, :] = xs.reshape(nv3d, nlev, len(j)).transpose(0, 2, 1)
    return out.reshape(-1)


# (nlev, nlon, nlat, np, rank, nv3d, m is the mean slot, layout); nij1 in the comment
MP_CASES = [(1, 1, 1, 1, 0, 1, False, "point"),          # 1
            (31, 3, 1, 5, 1, 4, True, "member"),         # 1, np > nxy
            (32, 19, 5, 3, 0, 1, True, "padded"),        # 32, the long share of 95 = 32 + 32 + 31
            (33, 19, 5, 3, 2, 4, False, "point"),        # 31, the short share
            (65, 14, 7, 3, 1, 4, False, "member"),       # 33
            (33, 14, 7, 3, 2, 1, True, "point"),         # 32, short share of 98 = 33 + 33 + 32
            (65, 20, 15, 3, 0, 1, False, "padded"),      # 100
            (1, 31, 3, 3, 0, 4, True, "point"),          # 31, one level
            (32, 20, 15, 3, 2, 4, False, "member"),      # 100
            (31, 8, 4, 1, 0, 4, True, "padded")]         # 32, one rank
MP_K = 2                                                 # members beside the mean slot in the state these cases use


# --------------------------------------------------------------------------------------------------------- state_trans
# common_scale.f90:1181-1224 (forward), :1229-1280 (inverse)
SLOTS = ("iv_rho", "iv_rhou", "iv_rhov", "iv_rhow", "iv_rhot", "iv_u", "iv_v", "iv_w", "iv_t", "iv_p")
TRACER_CV = [1407.0, 4218.0, 4218.0, 2006.0, 2006.0, 2006.0, 2106.0, 1952.0]     # QV QC QR QI QS QG and two more


def state_consts(assign, nq, clamp_q=0, clamp_qhyd=0):
    """SCALE-RM's constants as a dict; `assign`: 'scale' (common_scale.f90:36-51, the analysis variables overwrite the
    prognostic ones slot for slot), 'shift' (analysis variable i sits in the slot of prognostic variable i + 2, cyclically:
    every write lands on a slot another quantity is read from) or 'disjoint' (analysis 5..9, moisture moved up to 10)"""
    c = dict(rdry=287.04, rvap=461.46, cvdry=1004.64 - 287.04, pre00=1.0e5, tracer_cv=TRACER_CV[:nq],
             iv_rho=0, iv_rhou=1, iv_rhov=2, iv_rhow=3, iv_rhot=4, positive_definite_q=clamp_q,
             positive_definite_qhyd=clamp_qhyd)
    ana = {"scale": [0, 1, 2, 3, 4], "shift": [2, 3, 4, 0, 1], "disjoint": [5, 6, 7, 8, 9]}[assign]
    c.update(zip(SLOTS[5:], ana))
    c["iv_q"] = 10 if assign == "disjoint" else 5
    c["nv3d"] = c["iv_q"] + nq
    return c


def clamped_species(c):
    """the slots state_trans_inv clamps: iv_q under POSITIVE_DEFINITE_Q; qc qr qi qs qg -- the five after it, and no
    further species -- under POSITIVE_DEFINITE_QHYD (:1244-1248)"""
    out = [c["iv_q"]] if c["positive_definite_q"] else []
    if c["positive_definite_qhyd"]:
        out += [n for n in range(c["iv_q"] + 1, min(c["nv3d"], c["iv_q"] + 6))]
    return out


def state_trans_ld(c, v, inverse):
    """v [nv3d, n] float64 -> the transformed state in longdouble (untouched variables carry their float64 value)"""
    a = v.astype(LD)
    iq, nv3d = c["iv_q"], c["nv3d"]
    if inverse:
        for n in clamped_species(c):
            a[n] = np.maximum(a[n], LD(0))
    qdry, cvtot = LD(1), LD(0)
    for n in range(iq, nv3d):
        qdry = qdry - a[n]
        cvtot = cvtot + a[n] * LD(c["tracer_cv"][n - iq])
    cvtot = LD(c["cvdry"]) * qdry + cvtot
    rtot = LD(c["rdry"]) * qdry + LD(c["rvap"]) * a[iq]
    pre00 = LD(c["pre00"])
    out = a.copy()
    if not inverse:
        rho = a[c["iv_rho"]]
        pres = pre00 * (a[c["iv_rhot"]] * rtot / pre00) ** ((cvtot + rtot) / cvtot)
        out[c["iv_u"]], out[c["iv_v"]], out[c["iv_w"]] = a[c["iv_rhou"]] / rho, a[c["iv_rhov"]] / rho, a[c["iv_rhow"]] / rho
        out[c["iv_t"]], out[c["iv_p"]] = pres / (rho * rtot), pres
    else:
        pr = a[c["iv_p"]]
        rho = pr / (rtot * a[c["iv_t"]])
        out[c["iv_rhot"]] = pre00 / rtot * (pr / pre00) ** (cvtot / (cvtot + rtot))
        out[c["iv_rhow"]], out[c["iv_rhov"]], out[c["iv_rhou"]] = a[c["iv_w"]] * rho, a[c["iv_v"]] * rho, a[c["iv_u"]] * rho
        out[c["iv_rho"]] = rho
    return out


def state_written(c, inverse):
    w = [c[s] for s in (SLOTS[:5] if inverse else SLOTS[5:])]
    return sorted(set(w + (clamped_species(c) if inverse else [])))


def state_field(c, n, seed, negative=True):
    """a plausible SCALE restart state [nv3d, n] under c's slots; some hydrometeors slightly negative when asked"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(1.0, 2.0, (c["nv3d"], n))               # slots no variable owns (the disjoint assignment's 5..9)
    rho = rng.uniform(0.3, 1.2, n)
    v[c["iv_rho"]] = rho
    v[c["iv_rhou"]] = rho * rng.normal(5, 10, n)
    v[c["iv_rhov"]] = rho * rng.normal(0, 10, n)
    v[c["iv_rhow"]] = rho * rng.normal(0, 1, n)
    v[c["iv_rhot"]] = rho * rng.uniform(290, 450, n)
    v[c["iv_q"]] = rng.uniform(-2e-3 if negative else 0.0, 0.02, n)
    for s in range(c["iv_q"] + 1, c["nv3d"]):
        v[s] = rng.uniform(-1e-4 if negative else 0.0, 1e-3, n)
    return v


def state_inverse_input(c, v):
    """what state_trans_inv is handed: the forward statement rounded to float64, the moisture as it was"""
    return state_trans_ld(dict(c, positive_definite_q=0, positive_definite_qhyd=0), v, False).astype(np.float64)


STATE_GRIDS = [(1, 1, 1), (5, 3, 17), (36, 7, 5)]           # 1, 255 and 1260 points
STATE_NQ = [1, 6, 8]
STATE_ASSIGN = ["scale", "shift", "disjoint"]
CLAMPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


# ------------------------------------------------------------------------------------------------ relax_beta, infl_init
def beta_params(radar_only, bw, nlong=37, nlatg=29, ihalo=2, jhalo=2, dx=1000.0, dy=1250.0, radar_zmax=10000.0,
                vert_local_radar=2000.0):
    return dict(radar_only=radar_only, ihalo=ihalo, jhalo=jhalo, nlong=nlong, nlatg=nlatg, radar_zmax=radar_zmax,
                vert_local_radar=vert_local_radar, boundary_buffer_width=bw, dx=dx, dy=dy)


def zcut_of(p):
    return p["radar_zmax"] + p["vert_local_radar"] * ZFAC


def relax_beta(p, rig, rjg, hgt):
    """letkf_tools.f90:1911-1948 for hgt [nlev, nij1]; float64 throughout, as the reference"""
    nlev, nij1 = hgt.shape
    beta = np.ones((nlev, nij1))
    if p["boundary_buffer_width"] > 0.0:
        di = np.minimum(rig - p["ihalo"], (p["nlong"] + p["ihalo"] + 1) - rig) * p["dx"]
        dj = np.minimum(rjg - p["jhalo"], (p["nlatg"] + p["jhalo"] + 1) - rjg) * p["dy"]
        dist = np.minimum(di, dj) / p["boundary_buffer_width"]
        b2 = np.where(dist < 1.0, np.maximum(dist, 0.0), 1.0)
        beta = np.broadcast_to(b2, (nlev, nij1)).copy()
    if p["radar_only"]:
        beta[hgt > zcut_of(p)] = 0.0
    return beta


def beta_points(p):
    """(rig, rjg) placed by hand for a buffer of 5 cells in i: dist_bdy exactly 0 (on either edge), exactly 1 (where beta
    stays 1), one ulp inside 1, just inside and outside the domain (negative distance: 0), the middle, and the j side"""
    bw = p["boundary_buffer_width"] if p["boundary_buffer_width"] > 0 else 5000.0
    lo_i, hi_i = float(p["ihalo"]), float(p["nlong"] + p["ihalo"] + 1)
    lo_j, hi_j = float(p["jhalo"]), float(p["nlatg"] + p["jhalo"] + 1)
    wi, wj = bw / p["dx"], bw / p["dy"]
    mid_i, mid_j = 0.5 * (lo_i + hi_i), 0.5 * (lo_j + hi_j)
    ri = [lo_i, hi_i, lo_i + wi, hi_i - wi, np.nextafter(lo_i + wi, 0.0), np.nextafter(lo_i, np.inf), lo_i - 0.5, hi_i + 0.5,
          mid_i, mid_i, mid_i, mid_i, mid_i, lo_i + 0.25 * wi, lo_i + 0.25 * wi, 0.0]
    rj = [mid_j, mid_j, mid_j, mid_j, mid_j, mid_j, mid_j, mid_j,
          mid_j, lo_j, hi_j - wj, np.nextafter(lo_j, -np.inf), lo_j + 0.5 * wj, lo_j + 0.5 * wj, lo_j + 0.125 * wj, mid_j]
    return np.array(ri), np.array(rj)


def beta_heights(p, nlev, nij1, seed):
    """hgt [nlev, nij1]: random columns with zcut itself and its two float64 neighbours planted in them"""
    rng = np.random.default_rng(seed)
    z = zcut_of(p)
    h = np.sort(rng.uniform(20.0, 19000.0, (nlev, nij1)), axis=0)
    flat = h.reshape(-1)
    spots = rng.permutation(flat.size)[:min(3, flat.size)]
    for s, val in zip(spots, (z, np.nextafter(z, np.inf), np.nextafter(z, 0.0))):
        flat[s] = val
    return h


BETA_FLAGS = [(1, 0.0), (0, 5000.0), (1, 5000.0), (0, 0.0)]   # radar_only x buffer


def infl_init(w, infl_mul, infl_mul_min):
    """letkf_tools.f90:237-267 (the read-in branch leaves the caller's field in place)"""
    out = np.full_like(w, infl_mul) if infl_mul > 0.0 else w.copy()
    return np.maximum(out, infl_mul_min) if infl_mul_min > 0.0 else out


INFL_SIGNS = [(1.3, 0.0), (-1.0, 0.95), (0.8, 1.0), (-1.0, 0.0)]


# ------------------------------------------------------------------------------------------ additive inflation, weights
def additive_ld(anal3, add3, k, nij1, infl_add, weight=None, qmean2=None, iv_q_first=5, iv_q_last=10, ishuf=None):
    """letkf_tools.f90:884-913 on logical [nv, k+1, npts] arrays (qmean2 [nv, npts]); returns (anal in longdouble, |x|):
    the term added and, for the bound, its size.  The mean slot is not touched."""
    nv, _, npts = anal3.shape
    src = np.arange(k) if ishuf is None else np.asarray(ishuf)
    x = add3[:, src, :].astype(LD) * LD(infl_add)
    if weight is not None:
        x = x * np.tile(weight.astype(LD), npts // nij1)[None, None, :]
    if qmean2 is not None:
        for v in range(nv):
            if iv_q_first <= v <= iv_q_last:
                x[v] = x[v] * qmean2[v].astype(LD)[None, :]
    out = anal3.astype(LD)
    out[:, :k] = out[:, :k] + x
    ax = np.zeros(anal3.shape)
    ax[:, :k] = np.abs(x).astype(np.float64)
    return out, ax


def additive_bound(anal3, ax):
    """4 u (|anal| + |x|): three roundings in the product x, one in the sum"""
    return 4 * U * (np.abs(anal3) + ax)


def shuffle_with_fixed_points(k):
    """members 1 <-> 2, 4 <-> 5, ... swapped, 0, 3, ... where they are"""
    s = np.arange(k, dtype=np.int32)
    for a in range(1, k - 1, 3):
        s[a], s[a + 1] = a + 1, a
    return s


def additive_case(k, nv, nij1, nlev, seed):
    rng = np.random.default_rng(seed)
    npts = nij1 * nlev
    return dict(k=k, nv=nv, nij1=nij1, nlev=nlev, npts=npts, infl_add=0.3,
                anal=rng.normal(0.0, 1.0, (nv, k + 1, npts)), add=rng.normal(0.0, 0.1, (nv, k + 1, npts)),
                gues=rng.uniform(1e-4, 1e-2, (nv, k + 1, npts)), weight=rng.uniform(0.0, 1.0, max(nij1, 1)),
                ishuf=shuffle_with_fixed_points(k))


# (weight, qmean, ishuf) all eight ways with the layouts and q layouts dealt round; then the edges
#   qmean: None, "packed" ([nv, npts], q_sp 1, q_sv npts) or the name of the layout of the gues buffer whose mean slot it views
ADD_CASES = [dict(weight=w, qmean=q, ishuf=s, layout=lay)
             for (w, q, s), lay in zip([(0, None, 0), (1, None, 0), (0, "packed", 0), (0, None, 1), (1, "point", 0),
                                        (1, None, 1), (0, "member", 1), (1, "packed", 1)],
                                       ["point", "member", "padded", "point", "member", "padded", "point", "member"])]
ADD_CASES += [dict(weight=1, qmean="padded", ishuf=1, layout="padded"),
              dict(weight=1, qmean="packed", ishuf=1, layout="point", q=(7, 7)),          # iv_q_first == iv_q_last
              dict(weight=0, qmean="point", ishuf=0, layout="member", q=(11, 10)),        # a q range without a variable
              dict(weight=1, qmean="packed", ishuf=0, layout="padded", k=1),
              dict(weight=0, qmean=None, ishuf=1, layout="member", k=1)]
for _c in ADD_CASES:
    _c.setdefault("k", 6)
    _c.setdefault("q", (5, 10))


def addinfl_weight_d(rig, rjg, ob_ri, ob_rj, dx, dy, hori_loc):
    """:818-830 in float64, operation by operation as the reference writes them: the scaled squared distance to the nearest
    observation (1e33 / hori_loc^2 without one)"""
    if len(ob_ri) == 0:
        best = np.full(len(rig), 1.0e33)
    else:
        rdx = (rig[:, None] - ob_ri[None, :]) * dx
        rdy = (rjg[:, None] - ob_rj[None, :]) * dy
        best = np.minimum((rdx * rdx + rdy * rdy).min(axis=1), 1.0e33)
    return best / (hori_loc * hori_loc)


def addinfl_weight_ld(d):
    """:831-833: exp(-d/2) up to and including the cut-off, exactly 0 beyond"""
    return np.where(d <= CUT2, np.exp(LD(-0.5) * d.astype(LD)), LD(0))


def cutoff_construction():
    """(hori_loc, t_eq, t_beyond): with dx = 1, an observation at the origin and a grid point at (t, 0), the float64
    arithmetic of :822-830 gives t*t / (hori_loc*hori_loc) == CUT2 for t_eq and the next double above CUT2 for t_beyond.
    Found by a fixed search (about every second double is reachable as a rounded square)."""
    above = np.nextafter(CUT2, np.inf)
    for j in range(4096):
        h = 1.0 + j * 2.0 ** -20
        h2 = h * h
        t0 = np.sqrt(CUT2 * h2)
        found = {}
        t = t0
        for _ in range(16):
            t = np.nextafter(t, 0.0)
        for _ in range(48):
            d = (t * t + 0.0) / h2
            if d == CUT2 and "eq" not in found:
                found["eq"] = t
            if d == above and "above" not in found:
                found["above"] = t
            t = np.nextafter(t, np.inf)
        if len(found) == 2:
            return h, found["eq"], found["above"]
    raise AssertionError("no construction found")


def weight_case(nij1, nob, seed):
    """grid points and reflectivity observations a few localisation lengths apart: weights from 1 down to the cut-off and 0"""
    rng = np.random.default_rng(seed)
    rig, rjg = rng.uniform(2.5, 40.5, nij1), rng.uniform(2.5, 40.5, nij1)
    ob_ri, ob_rj = rng.uniform(10.0, 25.0, nob), rng.uniform(10.0, 25.0, nob)
    if nob > 0:                                   # the LAST observation exactly on a grid point (lane nob-1 mod 64 finds it)
        rig[nij1 // 2], rjg[nij1 // 2] = ob_ri[-1], ob_rj[-1]
    return dict(rig=rig, rjg=rjg, ob_ri=ob_ri, ob_rj=ob_rj, dx=1000.0, dy=1000.0, hori_loc=4000.0, on_obs=nij1 // 2)


WEIGHT_NOB = [0, 1, 63, 64, 65, 1000]
WEIGHT_NIJ1 = [1, 90]


# ------------------------------------------------------------------------------------------------------------ monit_dep
ID_T, ID_TV, ID_REF, ID_RE0 = 3073, 3074, 4001, 4004       # common_obs_scale.f90:50-51, 65-66
ELEM_UID = np.array([2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, 4003, 8800, 99991, 99992,
                     99993], dtype=np.int32)               # :74-77; lists 3074 and 4004 themselves


def monit_table(nid):
    if nid == 1:
        return np.array([ID_T], dtype=np.int32)
    if nid == 16:
        return ELEM_UID.copy()
    return np.concatenate([ELEM_UID, np.arange(5001, 5001 + nid - 16, dtype=np.int32)])


def monit_dep_ld(table, elm, dep, qc):
    """common_obs_scale.f90:1851-1895: (nobs, bias, mean square, mean |dep|) per table slot in longdouble; rmse is the root
    of the third.  A row whose (folded) id the table lacks counts nowhere; undef where nothing counted."""
    e = np.where(elm == ID_TV, ID_T, elm)
    e = np.where(e == ID_RE0, ID_REF, e)
    good = qc == 0
    nid = len(table)
    nobs = np.zeros(nid, np.int32)
    bias, ms, mabs = np.full(nid, LD(UNDEF)), np.full(nid, LD(UNDEF)), np.zeros(nid, LD)
    for u, uid in enumerate(table):
        d = dep[good & (e == uid)].astype(LD)
        nobs[u] = d.size
        if d.size:
            bias[u], ms[u], mabs[u] = d.sum() / LD(d.size), (d * d).sum() / LD(d.size), np.abs(d).sum() / LD(d.size)
    return nobs, bias, ms, mabs


def monit_chain(nn, nblk):
    """L, the longest chain of additions of the two-level reduction: a thread's run over its block's share, the 8 levels of
    the 256-wide tree, the nblk partial sums"""
    per = -(-nn // nblk) if nn > 0 else 0
    return -(-per // 256) + 8 + nblk


def monit_sizes(num_cu):
    nblk = 4 * num_cu
    return dict(one=1, n255=255, n257=257, per257=257 * nblk - 100, ragged=3 * nblk - 5)


def monit_case(nid, nn, kind, seed):
    """kind 'offset': departures with a mean 10^3 times their spread; 'zero': mean about 0.  A fifth of the rows rejected,
    ids drawn from the table, from 3074 / 4004 and from ids no table here lists"""
    rng = np.random.default_rng(seed)
    table = monit_table(nid)
    pool = np.concatenate([table[:12], [ID_TV, ID_RE0, ID_T, ID_REF, 777, 123456]]).astype(np.int32)
    elm = rng.choice(pool, nn).astype(np.int32)
    dep = rng.normal(2000.0, 2.0, nn) if kind == "offset" else rng.normal(0.0, 2.0, nn)
    qc = np.where(rng.random(nn) < 0.2, 5, 0).astype(np.int32)
    return table, elm, dep, qc
