"""Context.state_to_history -> Context.obssim with stggrd = 1, the `restart` branch of scale/obs/obssim.f90:79-86, on the small
fixture of the departure monitor (tests/_monit.py, nlev = 8): the simulator reads the history fields the first call left on the
device.  Compared with the statement of tests/_obssim.py applied to the numpy history fields of tests/_monit.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import _monit as M
import _obsope as O
import _obssim as S

pytestmark = pytest.mark.gpu
VARS3 = (O.ID_REF, O.ID_VR, O.ID_U, O.ID_V, O.ID_T, O.ID_Q)
VARS2 = (O.ID_T, O.ID_PS)


def test_the_simulator_runs_on_the_history_fields_built_on_the_device():
    from _gpu import ctx, pkg
    c, device = ctx(), torch.device("cuda:0")
    g = O.make_grid(8)
    st = M.make_state(g, M.SEEDS[8])
    v3, v2 = M.history(st, g)
    base = S.make_case("8x5x3")                                            # its lon / lat / rotc: the same interior
    case = dict(g=g, v3=v3, v2=v2, lon=base["lon"], lat=base["lat"], rotc=base["rotc"], radar=S.RADAR)
    cfg = S.default_cfg(method_ref_calc=2, stggrd=1, ps_adjust_thres=1.0e4)
    want = S.statement(case, cfg, VARS3, VARS2)
    assert want["dist"] > 1e-6, want["dist"]
    assert not want["terrain3"].any()
    # the history fields on the device, then the simulator on them
    ds = M.DeviceState(pkg, st, device)
    fl = M.hist_layout(pkg, g)
    d3 = torch.full((O.NV3DD * g["nlath"] * g["nlonh"] * g["nlevh"],), np.nan, dtype=torch.float64, device=device)
    d2 = torch.full((O.NV2DD * g["nlath"] * g["nlonh"],), np.nan, dtype=torch.float64, device=device)
    fl.v3d, fl.v2d = C.c_void_p(d3.data_ptr()), C.c_void_p(d2.data_ptr())
    c.state_to_history(ds.hs, fl, d3, d2)
    dc = S.DeviceCase(pkg, case, cfg, VARS3, VARS2, device, states=(0, 1))
    out = dc.outputs()
    c.obssim(dc.params, fl, out["v3"], out["v2"], out["rec"])
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy() for n, t in out.items()}
    bad, worst, excluded = S.compare(got["v3"], got["v2"], want)
    print(f"worst error / tolerance {worst}")
    assert excluded == 0 and bad == []
    assert {"dbz", "vr", "interp", "pass", "ps", "undef"} <= set(want["kind3"].ravel()) | set(want["kind2"].ravel())
    assert np.array_equal(got["rec"].view(np.int32), S.records(got["v3"], got["v2"]).view(np.int32))
