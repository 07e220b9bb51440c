"""lon / lat -> letkf_phys2ij_dev -> letkf_obsscan_dev -> letkf_obsope_slot_dev: obsope_cal from the files' own columns.
tests/test_gpu_obsscan_chain.py's case (two subdomains of 6 x 10 points, three slots, two files), but starting from lon / lat:
the case's ri / rj go through the statement's inverse once, and the chain fed the device's ri, rj and rotc (rotc gathered per
obsda row with letkf_obs_gather_rows_dev) is compared with the same chain fed the statement's ri, rj, rotc.  Every integer output
is bit for bit equal; ensval agrees within 1e-10 * max|value|, the project's member tolerance.  The builder asserts on the CPU
that the statement's ri / rj stay 1e-6 from every edge at which an integer could flip: no row is dropped.

Then letkf_mapproj_grid_dev's lon2d / lat2d / rotc2d as letkf_obssim_dev's on its 5 x 3 fixture, to the simulator's own
tolerances (tests/_obssim.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mapproj as M
import _obssim as SIM
import _obsscan as S

pytestmark = pytest.mark.gpu
K = 4
CANARY = -4321.0
INTS = ("rank", "slot", "set", "idx", "qc", "bsn", "bsna")


def chain_inputs():
    """the scan chain's case with lon / lat that project onto its ri / rj, and the statement's ri, rj, rotc of those"""
    import test_gpu_obsscan_chain as T
    case, scan_in, _ = T.scan_chain_case()
    p = dict(M.configs()["BDA_d3_1km_9p_bf20"])          # 1 km cells; the 12 x 10 domain lies 90 km south-west of the base point
    q = M.setup(p)
    back = M.ij2phys(q, case["files"]["ri"], case["files"]["rj"])
    lon, lat = back["lon"], back["lat"]
    st = M.phys2ij(q, lon, lat)
    # every edge at which rij_rank's and the operator's integers change: the integers and the half-integers
    for v in (st["ri"], st["rj"]):
        assert np.abs(2.0 * v - np.round(2.0 * v)).min() >= 2e-6, "a row lies within 1e-6 of a ceiling or subdomain edge"
    assert np.abs(st["ri"] - case["files"]["ri"]).max() < 1e-9 and len(lon) == case["nrow"]
    assert np.abs(st["rotc"][:, 1]).min() > 1e-3          # the rotation is no identity here
    return T, case, scan_in, p, lon, lat, st


def run_chain(pkg, c, T, case, scan_in, lon, lat, ri, rj, rotc_rows, gather):
    """obsscan on ri / rj (device tensors), then the operator slot by slot; rotc_rows: device [file rows, 2]; gather: per obsda
    row by letkf_obs_gather_rows_dev (else by torch indexing)"""
    d = torch.device("cuda:0")
    files = dict(case["files"], ri=ri.cpu().numpy(), rj=rj.cpu().numpy(), lon=lon, lat=lat)
    scan = None
    ens = None
    for ip in range(T.PX):
        v3, v2, g, ri_off = T.subdomain(case, ip)
        sub = dict(case, g=g, v3=v3, v2=v2, files=files, rotc=np.zeros((1, 2)))
        dc = T.O.DeviceCase(pkg, sub, T.config(ri_off), d)
        dc.files.ri, dc.files.rj = C.c_void_p(ri.data_ptr()), C.c_void_p(rj.data_ptr())       # the device's own arrays, not a copy
        if scan is None:
            scan = c.obsscan(dc.files, torch.from_numpy(scan_in["dif"]).cuda(), scan_in["layout"], T.SLOTS)
            nlist = scan["set"].numel()
            off = torch.from_numpy(case["off"]).cuda()
            src_row = (off[(scan["set"] - 1).long()] + scan["idx"].long() - 1).to(torch.int32)
            rot = torch.full((nlist, 2), CANARY, dtype=torch.float64, device=d)
            if gather:
                c.obs_gather_rows(src_row, 2, rotc_rows, 2, rot, 2)
            else:
                rot = rotc_rows[src_row.long()].contiguous()
            ens = torch.full((nlist, K), CANARY, dtype=torch.float64, device=d)
        dc.params.rotc = C.c_void_p(rot.data_ptr())
        for islot in range(T.SLOTS[0], T.SLOTS[1] + 1):
            c.obsope_slot(scan, T.SLOTS[0], ip, islot, dc.params, dc.files, dc.fields, ens, K)
        torch.cuda.synchronize()
    out = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in scan.items() if v is not None}
    out["ensval"], out["rot"] = ens.cpu().numpy(), rot.cpu().numpy()
    return out


def test_the_chain_from_lon_lat_gives_the_integers_of_the_chain_from_the_statement():
    from _gpu import ctx, pkg
    c = ctx()
    T, case, scan_in, p, lon, lat, st = chain_inputs()
    proj = pkg.mapproj_setup(**M.setup_args(p))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ri, rj, rotc = c.phys2ij(proj, t(lon), t(lat))
    got = run_chain(pkg, c, T, case, scan_in, lon, lat, ri, rj, rotc, gather=True)
    want = run_chain(pkg, c, T, case, scan_in, lon, lat, t(st["ri"]), t(st["rj"]), t(st["rotc"]), gather=False)
    for k in INTS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert got["set"].size == case["nrow"] and (got["qc"] == 0).sum() > 100             # no row left out, most of them observed
    assert np.abs(got["rot"] - want["rot"]).max() <= 2 * M.BOUND_ROTC and (got["rot"] != CANARY).all()
    inside = want["ensval"] != CANARY
    assert np.array_equal(inside, got["ensval"] != CANARY) and inside.sum() > 400
    scale = np.abs(want["ensval"][inside]).max()
    err = np.abs(got["ensval"][inside] - want["ensval"][inside]).max()
    print(f"chain: {inside.sum()} values, max |difference| / max|value| {err / scale:.2e}")
    assert err <= 1e-10 * scale
    # the wind rows felt the rotation: with rotc = (1, 0) they differ
    ident = run_chain(pkg, c, T, case, scan_in, lon, lat, ri, rj, t(np.tile(np.array([1.0, 0.0]), (case["nrow"], 1))), gather=True)
    assert np.abs(ident["ensval"][inside] - got["ensval"][inside]).max() > 1e-6


def test_the_grid_loop_feeds_the_simulator():
    from _gpu import ctx, pkg
    c = ctx()
    d = torch.device("cuda:0")
    base = SIM.make_case("8x5x3")
    g = base["g"]
    p = M.configs()["BDA_d3_1km_9p_bf20"]
    q, proj = M.setup(p), pkg.mapproj_setup(**M.setup_args(p))
    cx1, cy1 = p["cxg1"] + 84 * p["dx"], p["cyg1"] + 88 * p["dy"]                  # a subdomain next to the base point
    st_grid = M.grid(q, g["nlon"], g["nlat"], g["ihalo"], g["jhalo"], cx1, cy1)
    case = dict(base, lon=st_grid["lon"], lat=st_grid["lat"], rotc=st_grid["rotc"], radar=(135.45, 34.75, 300.0), on_radar=None)
    cfg = SIM.default_cfg(method_ref_calc=2, use_terminal_velocity=1, stggrd=0)
    st = SIM.statement(case, cfg, SIM.VARS3, SIM.VARS2)
    dc = SIM.DeviceCase(pkg, case, cfg, SIM.VARS3, SIM.VARS2, d)
    fed_statement = dc.run(c)
    out = c.mapproj_grid(proj, g["nlon"], g["nlat"], g["ihalo"], g["jhalo"], cx1, cy1)
    dc.params.lon, dc.params.lat, dc.params.rotc = (C.c_void_p(out[k].data_ptr()) for k in ("lon", "lat", "rotc"))
    fed_device = dc.run(c)
    for got in (fed_statement, fed_device):
        bad, worst, excluded = SIM.compare(got["v3"], got["v2"], st)
        assert bad == [], bad[:3]
    # ... and against each other, to the same tolerances
    bad, worst, _ = SIM.compare(fed_device["v3"], fed_device["v2"], dict(st, val3=fed_statement["v3"], val2=fed_statement["v2"]))
    print(f"obssim fed by the grid loop: worst difference / tolerance {worst}")
    assert bad == []
    assert np.abs(out["rotc"].cpu().numpy()[..., 1]).max() > 1e-4                   # a rotation that is no identity
