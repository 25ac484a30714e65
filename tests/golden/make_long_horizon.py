"""Record the reference's runs at long time horizons (T + 1 in (256, 1024]: mode pitches 512 and 1024).

Same recording as make_golden.py's solver runs (run_reference / save_run layout: ``last_iteration``, ``hist_*``, ``kw_*``,
``sol_*``), on ``meshes.plane(8)`` at tol 1e-3.  The files are named ``long_*.npz`` so that the suites that walk
``run_*.npz`` with every Laplacian solver (the modal PCG takes T + 1 <= 256 only) do not pick them up.  Of the solution
only ``mu`` is kept (31 k doubles at T = 383, 83 k at T = 1023): every file stays well under 1 MB.

    python tests/golden/make_long_horizon.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402
from dots_socp_amd import meshes  # noqa: E402
from make_golden import geometry_for, run_reference  # noqa: E402

CASES = [
    ("plane8_T383_tol1e-3", 383, dict(nit=3000, tol=1e-3)),
    ("plane8_T383_cong_tol1e-3", 383, dict(nit=3000, tol=1e-3, congestion=0.05)),
    ("plane8_T1023_tol1e-3", 1023, dict(nit=3000, tol=1e-3)),
]


def save_long(name, geometry, n_time, kw, sol, hist):
    out = dict(vertices=geometry["vertices"], triangles=geometry["triangles"], mu0=geometry["mu0"], mu1=geometry["mu1"],
               n_time=np.array(n_time))
    for k, val in kw.items():
        out[f"kw_{k}"] = np.array(val)
    out["sol_mu"] = sol["mu"]
    out["hist_kkt_errors"] = np.asarray(hist.kkt_errors, dtype=np.float64)
    out["hist_kkt_iteration"] = np.asarray(hist.kkt_iteration, dtype=np.float64)
    for k, val in hist.history.items():
        out["hist_" + k.replace(" ", "_")] = np.asarray(val, dtype=np.float64)
    out["last_iteration"] = np.array(int(hist.kkt_iteration[-1]))
    path = os.path.join(HERE, f"long_{name}.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes, last iteration", int(hist.kkt_iteration[-1]),
          "cost", hist.history["Transportation cost"][-1], flush=True)


def main(argv):
    ref = ref_shim.load_reference()
    g, _ = geometry_for(ref, *meshes.plane(8))
    for name, T, kw in CASES:
        if argv and name not in argv:
            continue
        sol, hist = run_reference(ref, g, T, **kw)
        save_long(name, g, T, kw, sol, hist)


if __name__ == "__main__":
    main(sys.argv[1:])
