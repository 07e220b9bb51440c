"""Context.obsscan -> Context.obsope_slot per subdomain and slot: CALL obsope_cal replaced whole.  The rows of
tests/test_gpu_obsope_chain.py's case (12 x 10 points, two files) on two subdomains of 6 x 10 points and three time slots, each
subdomain with its own window of the history fields.  ensval / qc must be bit for bit what letkf_obsope_dev gives on the rows the
numpy statement of the scan resolves; the out-of-time rows carry 97, the out-of-domain rows 98, and the operator touches
neither."""
import numpy as np
import pytest
import torch

import _obsope as O
import _obsscan as S

K = 4
PX, NLON = 2, 6
SLOTS = (1, 3, 2, 600.0)
CANARY = -4321.0


def scan_chain_case():
    """the operator chain's case, a dif per file row (three slots and both sides of the window) and the statement of the scan"""
    from test_gpu_obsope_chain import chain_case
    case = chain_case()
    g = case["g"]
    assert g["nlon"] == PX * NLON
    rng = np.random.default_rng(77)
    dif = rng.uniform(-1100.0, 1100.0, case["nrow"])
    scan_in = dict(off=case["off"], ri=case["files"]["ri"], rj=case["files"]["rj"], dif=dif,
                   layout=(NLON, g["nlat"], g["ihalo"], g["jhalo"], PX, 1), slots=SLOTS, run=None)
    st = S.scan(scan_in)
    assert (st["bsn"][:, :3] >= 5).all() and (st["bsn"][:, 3] >= 5).all() and st["bsn"][0, 4] >= 5
    return case, scan_in, st


def subdomain(case, ip):
    """(fields v3, v2 of subdomain ip with its halo, its grid, its ri_off): rij_g2l"""
    g = dict(case["g"], nlon=NLON, nlonh=NLON + 2 * case["g"]["ihalo"])
    i0 = ip * NLON
    v3 = np.ascontiguousarray(case["v3"][:, :, :, i0:i0 + g["nlonh"], :])
    v2 = np.ascontiguousarray(case["v2"][:, :, :, i0:i0 + g["nlonh"]])
    return v3, v2, g, float(i0)


def config(ri_off):
    return O.default_cfg(method_ref_calc=2, ri_off=ri_off, rj_off=0.0, use_obs=np.ones(O.NOBTYPE, dtype=np.int32),
                         min_radar_ref_dbz=5.0, low_ref_shift=-1.0)


def device_case(pkg, case, st, ip, dev):
    """O.DeviceCase of subdomain ip with obsda's rows as the scan's statement lists them"""
    v3, v2, g, ri_off = subdomain(case, ip)
    nlist = len(st["set"])
    sub = dict(case, g=g, v3=v3, v2=v2, set=st["set"], idx=st["idx"], nrow=nlist, rotc=np.tile(np.array([1.0, 0.0]), (nlist, 1)))
    return O.DeviceCase(pkg, sub, config(ri_off), dev)


@pytest.mark.gpu
def test_scan_then_slot_operator_gives_the_bits_of_the_operator_on_the_statements_rows():
    from _gpu import ctx, dev, pkg
    c = ctx()
    case, scan_in, st = scan_chain_case()
    nlist = len(st["set"])
    d = torch.device("cuda:0")
    dcs = [device_case(pkg, case, st, ip, d) for ip in range(PX)]

    # the reference path: letkf_obsope_dev on row ranges resolved by the statement, qc starting as the statement leaves it
    ens_a = torch.full((nlist, K), CANARY, dtype=torch.float64, device=d)
    qc_a = dev(st["qc"])
    for ip in range(PX):
        for islot in range(SLOTS[0], SLOTS[1] + 1):
            first, count = S.rows_of(st["bsna"], SLOTS[0], ip, islot)
            c.obsope(dcs[ip].params, dcs[ip].files, dcs[ip].fields, dcs[ip].set, dcs[ip].idx, qc_a, ens_a, K, row0=first, nrows=count)

    # the path under test: the scan on the device, then one call per subdomain and slot
    scan = c.obsscan(dcs[0].files, dev(scan_in["dif"]), scan_in["layout"], SLOTS)
    torch.cuda.synchronize()
    assert scan["own"] is None                                            # (no myrank_d was given)
    S.assert_same_bits({k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in scan.items() if v is not None}, st)
    qc_scan = scan["qc"].cpu().numpy()
    ens_b = torch.full((nlist, K), CANARY, dtype=torch.float64, device=d)
    for ip in range(PX):
        for islot in range(SLOTS[0], SLOTS[1] + 1):
            c.obsope_slot(scan, SLOTS[0], ip, islot, dcs[ip].params, dcs[ip].files, dcs[ip].fields, ens_b, K)
    torch.cuda.synchronize()

    ea, eb, qa, qb = ens_a.cpu().numpy(), ens_b.cpu().numpy(), qc_a.cpu().numpy(), scan["qc"].cpu().numpy()
    assert np.array_equal(ea.view(np.int64), eb.view(np.int64))
    assert np.array_equal(qa, qb)
    out_time, out_dom = qc_scan == S.IQC_TIME, qc_scan == S.IQC_OUT_H
    assert out_time.sum() >= 10 and out_dom.sum() >= 5
    assert (qb[out_time] == S.IQC_TIME).all() and (qb[out_dom] == S.IQC_OUT_H).all()
    assert (eb[out_time | out_dom] == CANARY).all()                       # ... untouched by the operator
    inside = ~(out_time | out_dom)
    assert (eb[inside] != CANARY).all() and (qb[inside] == 0).sum() > 100
    # the second subdomain's rows start where the first one's end
    first, count = S.rows_of(st["bsna"], SLOTS[0], 1, 0)
    assert first == st["bsna"][0, -1] and count == st["bsn"][1].sum()
