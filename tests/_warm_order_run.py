"""Run by tests/test_gpu_warm_order.py in a process of its own with LETKF_AMD_LIB = the PROF twin of the library (make PROF=1: the
only build that reads LETKF_AMD_WARM_DBG).  C2-mini through letkf_das_points_dev with runs up the columns (warm_stride = nij1),
once with the sorted eigenvectors handed over at line position rank ^ 1 (the default) and once at position rank (bit 5 of the
knob), in ONE build.  Prints one JSON line: mean nsweep over the warm-started points of both calls, the largest status, whether
the analyses agree, and the twin's own phase record of each call (stderr line "[letkf prof] wave-time share by phase": p4 x total
is the time inside the Jacobi iteration, which is what the step pairs cost)."""
import json
import os
import re
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import bench_workload as bw
    from __graft_entry__ import load_package
    pkg = load_package()
    assert "prof" in os.path.basename(pkg.LIB_PATH), pkg.LIB_PATH
    dev = torch.device("cuda:0")
    cx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    w = bw.build("C2-mini", dev)
    k, nv, npts = w["k"], w["nv"], w["npts"]
    nij1, nlev = w["cfg"]["nx"] * w["cfg"]["ny"], w["cfg"]["nz"]
    nobs = (w["obs_off"][1:] - w["obs_off"][:-1]).view(nlev, nij1)
    # a point is warm-started when the level below it in its column was solved (whole-column runs: warm_run = 0)
    warm = torch.zeros(nlev, nij1, dtype=torch.bool, device=dev)
    warm[1:] = (nobs[1:] > 0) & (nobs[:-1] > 0)
    warm = warm.view(-1)
    out = {}
    for tag, knob in (("pair", None), ("rank", "32")):
        os.environ.pop("LETKF_AMD_WARM_DBG", None)
        if knob:
            os.environ["LETKF_AMD_WARM_DBG"] = knob
        anal = torch.zeros_like(w["gues"])
        infl = torch.ones(npts * nv, dtype=torch.float64, device=dev)
        ns = torch.zeros(npts, dtype=torch.int32, device=dev)
        st = torch.full((npts,), -1, dtype=torch.int32, device=dev)
        # the twin writes its phase record to stderr (file descriptor 2): kept per call
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile() as tf:
            os.dup2(tf.fileno(), 2)
            try:
                cx.das_points(k, nv, w["obs_off"], w["obs_idx"], w["rdiag"], w["rloc"], w["ensval"], w["kld"], w["dep"], infl,
                              w["gues"], anal, w["sp"], w["sm"], w["sv"], relax_alpha_spread=0.95, nsweep=ns, status=st, warm_run=0,
                              warm_stride=nij1)
                torch.cuda.synchronize()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tf.seek(0)
            log = tf.read().decode(errors="replace")
        assert cx.last_path().startswith("letkf_wave_kernel<KR=50"), cx.last_path()
        m = re.search(r"wave-time share by phase.*? p4=([0-9.]+)%.* total=(\d+)", log)
        out[tag] = dict(warm=ns[warm].double().mean().item(), cold=ns[~warm & (nobs.view(-1) > 0)].double().mean().item(),
                        status_max=int(st.abs().max()), anal=anal.view(nv, w["nens"], npts)[:, :k].clone(),
                        jacobi_ticks=(float(m.group(1)) / 100.0 * int(m.group(2))) if m else None)
    os.environ.pop("LETKF_AMD_WARM_DBG", None)
    x = w["gues"].view(nv, w["nens"], npts)
    rel = 0.0
    for v in range(nv):
        scale = max(x[v, k].abs().max().item(), x[v, :k].abs().max().item())
        rel = max(rel, (out["pair"]["anal"][v] - out["rank"]["anal"][v]).abs().max().item() / scale)
    print(json.dumps(dict(warm_points=int(warm.sum()), nsweep_pair=out["pair"]["warm"], nsweep_rank=out["rank"]["warm"],
                          nsweep_cold_pair=out["pair"]["cold"], nsweep_cold_rank=out["rank"]["cold"],
                          status_max_pair=out["pair"]["status_max"], status_max_rank=out["rank"]["status_max"],
                          jacobi_ticks_pair=out["pair"]["jacobi_ticks"], jacobi_ticks_rank=out["rank"]["jacobi_ticks"],
                          anal_max_rel=rel)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
