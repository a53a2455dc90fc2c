"""The cases of tests/test_fwd_stage_trim_gpu.py, shared with tools/record_fwd_stage_trim.py (which records what the library of the
commit BEFORE a change of the per-stage work around the hidden layers gives for them): the paths of a stage -- stage time, forcing,
state broadcasts, mechanistic terms, first layer -- that the fixtures of tests/golden/fwd_asm_merge/ and tests/golden/fwd_lds_rot/
do not pin.  B = 4, T = 9 throughout.

Two input sets, both on a grid with ONE REPEATED TIME (t[5] == t[4]: the interval that copies the state):
  tvns    5-minute grid; tVNS non-zero and different at every grid point (input mode 2), the meal ONE constant per trajectory
          (input mode 1)
  pulse   2.5-hour grid (17.5 h in all, the span of the benchmark's 20 h); a meal pulse at one grid point, tall enough (the recorder
          searches heights and tolerances, and stores what it took) that a trajectory rejects a step (nfev > 6 nsteps + 2) and takes
          two steps in one interval; its last trajectory has no meal and starts from a z-scored state (N(0,1)^6, the regime of the
          benchmark's z-score leg) that runs into the pole of G / (K_m + G): status 2, step-size underflow (within the 5-minute
          grid's 35 minutes no z-scored state gets there)
Four configurations on each: L = 4 plain (the benchmark instantiation), L = 4 taped with its adjoint, L = 3 plain, RK4 at L = 4.
And the RHS and tangent-linear entry points of the C ABI on the same states.

Networks are cut out of the golden 64 x 4 network as in _fwd_asm_merge_cases; all inputs are stored in the fixtures, and of a
result everything but the parameter gradients, of which a fixture keeps every 64th and the sha256 of all (digest)."""
import hashlib
import os

import numpy as np

import _fwd_asm_merge_cases as A

H0, L0 = A.H0, A.L0
B, T = 4, 9
REPEAT = 5                                     # t[REPEAT] == t[REPEAT - 1]
FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_stage_trim")
INPUT_SETS = ("tvns", "pulse")
# name, L, taped, method (0 = DP5(4), 1 = RK4)
CONFIGS = [("l4", 4, False, 0), ("l4_tape", 4, True, 0), ("l3", 3, False, 0), ("rk4_l4", 4, False, 1)]
SOLVE_CASES = [(f"{s}_{c}", s, L, taped, method) for s in INPUT_SETS for (c, L, taped, method) in CONFIGS]
SOLVE_KEYS = ("y", "status", "nsteps", "nfev")


def fixture(name):
    return os.path.join(FIXTURE_DIR, name + ".npz")


def grid(hours):
    """Nine points `hours` apart, one of them twice."""
    k = np.arange(T)
    k[REPEAT:] -= 1
    return (k * hours).astype(np.float32)


def positive_intervals(t):
    return int((np.diff(np.asarray(t, dtype=np.float64)) > 0).sum())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def digest(out):
    """What a fixture keeps of a result: everything, but of the 13 510 parameter gradients every 64th and the sha256 of all of them."""
    out = dict(out)
    if "gnn" in out:
        g = np.ascontiguousarray(out.pop("gnn"))
        out["gnn_some"] = g[::64].copy()
        out["gnn_sha256"] = np.frombuffer(hashlib.sha256(g.tobytes()).digest(), dtype=np.uint8).copy()
    return out


def rejected_and_two_steps(out, t):
    """The two conditions of the `pulse` set on a DP5(4) result: some trajectory rejected a step, and some trajectory that ended well
    took more steps than its grid has intervals of positive length."""
    ok = out["status"] == 0
    return bool((out["nfev"] > 6 * out["nsteps"] + 2).any()) and bool((ok & (out["nsteps"] > positive_intervals(t))).any())


def run(hode, torch, inp, nn, ode, H, L, taped=False, method=0):
    """One solve at the tolerances stored with the inputs and, taped, its adjoint for the stored cotangent -> {name: numpy array}."""
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    sol = hode.solve_fwd(f(inp["x0"]), f(inp["t"]), f(inp["meal"]), f(inp["tvns"]), None, f(ode), f(nn), H, L, method=method,
                         rtol=float(inp["rtol"]), atol=float(inp["atol"]), want_tape=taped)
    out = {k: getattr(sol, k).cpu().numpy() for k in SOLVE_KEYS}
    if taped and "c" in inp:
        gx0, gnn, _ = hode.solve_bwd(sol, f(inp["c"]))
        out["gx0"], out["gnn"] = gx0.cpu().numpy(), gnn.cpu().numpy()
    return out, sol


def run_rhs(hode, torch, inp, nn, ode):
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    return {"f": hode.rhs_fwd(f(inp["x"]), f(inp["t"]), f(inp["meal"]), f(inp["tvns"]), None, f(ode), f(nn), H0, L0).cpu().numpy()}


def run_jvp(hode, torch, inp, nn, ode):
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    out, sol = run(hode, torch, inp, nn, ode, H0, L0, taped=True)
    out["dy"] = hode.solve_jvp(sol, v_ode=f(inp["v_ode"]), v_x0=f(inp["v_x0"])).cpu().numpy()
    return out
