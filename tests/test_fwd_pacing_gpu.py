"""The priority pacing of the register forward kernels (csrc/hode_solve_body.h, pace_prio) changes WHEN a wave issues its
instructions and nothing about what they compute: the paced product library and the lab library with the pacing switched off
(HODE_FWD_PACE=off) give identical bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")
LAB_LIB = os.path.join(PKG, "hode", "lab", "libhode_lab.so")


def test_paced_forward_is_bitwise_the_unpaced_forward(golden_dir, tmp_path):
    """At the benchmark tolerances (rtol 1e-6, atol 1e-8, the defaults of solve_fwd), on the golden inputs: a plain solve, a taping
    solve (and its adjoint, up to summation order), two parameter sets on a ragged batch (38 trajectories = 19 per set, not a
    multiple of anything), the fp64 kernel, and 8 203 trajectories on four grid points, which take the MULTI instantiation with two trajectories per wave
    and one wave that gets a single one.  (The lab switch is read once per process, so each side runs in a child process.)"""
    out = str(tmp_path / "pace.npz")
    code = f"""
import sys, numpy as np, torch
sys.path.insert(0, {PKG!r})
import hode
g = np.load({os.path.join(golden_dir, "g4_t61_pulses.npz")!r}); w = np.load({os.path.join(golden_dir, "g0_weights_h64_l4.npz")!r})
f = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), dtype=dt, device="cuda")
n = len(g["x0"])
rep = lambda a, B: np.concatenate([a] * (B // n + 1))[:B]
res = {{}}
def keep(tag, s):
    for k in ("y", "status", "nsteps", "nfev"):
        res[tag + "_" + k] = getattr(s, k).cpu().numpy()
nn, ode, t = f(w["nn_flat"]), f(w["ode"]), f(g["t"])
# plain and taping, one parameter set, ragged (37 trajectories)
x0, meal, tv = f(rep(g["x0"], 37)), f(rep(g["meal"], 37)), f(rep(g["tvns"], 37))
keep("plain", hode.solve_fwd(x0, t, meal, tv, None, ode, nn, 64, 4))
st = hode.solve_fwd(x0, t, meal, tv, None, ode, nn, 64, 4, want_tape=True)
keep("tape", st)
gx0, gnn, _ = hode.solve_bwd(st, torch.ones_like(st.y))
res["tape_gx0"] = gx0.cpu().numpy()
# two parameter sets, 19 trajectories each, with and without the tape
x0, meal, tv = f(rep(g["x0"], 38)), f(rep(g["meal"], 38)), f(rep(g["tvns"], 38))
nn2 = torch.cat([nn, 0.5 * nn]); ode2 = torch.cat([ode, ode])
keep("sets2", hode.solve_fwd(x0, t, meal, tv, None, ode2, nn2, 64, 4, n_sets=2))
keep("sets2_tape", hode.solve_fwd(x0, t, meal, tv, None, ode2, nn2, 64, 4, n_sets=2, want_tape=True))
# the fp64 register kernel
d = torch.float64
keep("fp64", hode.solve_fwd(f(rep(g["x0"], 5), d), f(g["t"], d), f(rep(g["meal"], 5), d), f(rep(g["tvns"], 5), d), None, f(w["ode"], d),
                            f(w["nn_flat"], d), 64, 4))
# MULTI: T <= 4, one parameter set, more than 8 192 trajectories
B = 8203
keep("multi", hode.solve_fwd(f(rep(g["x0"], B)), f(g["t"][:4]), f(rep(g["meal"], B)[:, :4]), f(rep(g["tvns"], B)[:, :4]), None, ode, nn, 64, 4))
torch.cuda.synchronize()
np.savez({out!r}, **res)
"""
    got = {}
    for side in ("paced", "unpaced"):
        if side == "paced":
            env = {k: v for k, v in os.environ.items() if k not in ("HODE_LIB", "HODE_FWD", "HODE_FWD_PACE")}
        else:
            env = dict({k: v for k, v in os.environ.items() if k != "HODE_FWD"}, HODE_LIB=LAB_LIB, HODE_FWD_PACE="off")
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[side] = dict(np.load(out))
        os.remove(out)
    assert sorted(got["paced"]) == sorted(got["unpaced"]) and len(got["paced"]) == 6 * 4 + 1
    for k in got["paced"]:
        if k == "tape_gx0":
            continue
        assert np.array_equal(got["paced"][k], got["unpaced"][k]), k
    # the adjoint is not the kernel under test, and the lab library lays its tape out differently: equal up to summation order, the
    # bound tests/test_hip_parity.py holds the lab library's adjoints to
    a, b = got["paced"]["tape_gx0"].astype(np.float64), got["unpaced"]["tape_gx0"].astype(np.float64)
    assert np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-5
    # the solves did what the cases say: every trajectory integrated, and the MULTI batch took its twelve-odd evaluations each
    for tag in ("plain", "tape", "sets2", "sets2_tape", "fp64", "multi"):
        assert int(got["paced"][tag + "_status"].max()) == 0, tag
    assert got["paced"]["multi_y"].shape == (8203, 4, 6) and int(got["paced"]["plain_nsteps"].min()) >= 60
    assert np.array_equal(got["paced"]["plain_y"], got["paced"]["tape_y"])
