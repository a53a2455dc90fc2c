"""The case table of the GENERIC tangent-linear solve: at which shapes and in which directions hode.solve_jvp on a network outside the
tuned envelope (hode_solve_jvp_any_*, csrc/hode_generic_jvp.hip) is held to the C oracle's hode_oracle_solve_jvp.  A plain module
(nothing of the product imported).  The solve cases, their data recipe and the bounds are those of tests/_input_grad_cases.py (IC); the
directions, the oracle helpers and the scaled norm are those of tests/_jvp_cases.py (JC) -- reused, not copied.
tests/test_jvp_generic_host.py admits every case on the CPU from the oracle alone; tests/test_jvp_generic_gpu.py runs the kernel.

Parts:
  g  the 12 cases of IC.SOLVE["b"] (the six GENERIC_SHAPES, 64x5 relu .. 128x5 relu, tanh / leaky / elu among them, both methods,
     with and without GD), unit directions (K = 23), both dtypes
  c  the ten g100x3-* row-bookkeeping cases of IC.SOLVE["c"]; unit directions and dense directions at K = 9
  k  direction tiling and pointers on g100x3-tbatched and g100x3-sets3x3, dense directions: K in JC.K_TILING; v_ode only / v_x0 only
  e  g100x3-budget6: a trajectory that runs out of steps (status 1), fp64, unit directions

Figures and bounds: those of JC's docstring (scaled norm; fp64 per (direction, component) for unit directions, per direction for dense
ones, within IC.FP64_TOL; fp32 per direction within min(MARGIN[part] x d_ref, IC.FP32_CAP), d_ref = the oracle's fp32 result against
its fp64 result on the same case and direction; admission holds d_ref <= cap / 8).  Nothing is measured against the kernel itself.

Measured on an MI355X (first GPU run of tests/test_jvp_generic_gpu.py, every MARGIN at 8: every test of parts g / c / k / e passed),
fp32 kernel error / d_ref, largest over the directions and cases of each part:

  part  figures  largest ratio  where                                                            margin
  g       266       4.01        h128l5relu-gnn1-gode1-gd1-m122-dp5 g (err 6.3e-7, d_ref 1.6e-7)   8 (not widened)
  c       288       5.77        g100x3-gdzero unit g (9.3e-7, 1.6e-7)                             8 (not widened)
  k       152       1.34        g100x3-sets3x3 K = 16, direction 14 (6.8e-8, 5.0e-8)              8
  (part e is fp64 only.)  d_ref: 9.0e-9 .. 1.15e-6, median 6.0e-8.  fp64: RK4 <= 5.9e-15, DP5(4) <= 2.0e-9 (part e; part g <= 1.2e-11).

Both ratios above 4 belong to the direction g, whose d_ref is ordinary (1.6e-7, above the table's median): no margin is widened.
It is the column JC's docstring explains for the tuned kernel -- the coefficient log GD - log IGD_50 carries one ulp of the device's
logf (1 ulp against glibc's half) through the same expression as the oracle -- and the mechanistic coefficients (jvp_coeffs,
csrc/hode_jvp.h) are shared by the two kernels.  Every figure is within 8 x d_ref.

The calibration case (calibration_case): 6 noise-free patients on a 13-point grid over 0..240, a tanh 96 x 3 network (IC.rand_net:
its output layer is not zero), CAL_NAMES perturbed within 2 sd of REFERENCE_PRIORS, least squares (priors=None).  Everything a
kernel reads through fp32 on its way in (the model's weights and constants, x0, t, meal) is rounded to fp32 here, so the oracle on the
CPU and fit_patients on the GPU see the same numbers.
"""
import functools

import numpy as np

import _input_grad_cases as IC
import _jvp_cases as JC

PARTS = ("g", "c", "k", "e")
# fp32 margin per part (see the docstring)
MARGIN = {"g": 8.0, "c": 8.0, "k": 8.0, "e": 8.0}
# part -> largest measured (fp32 kernel error) / d_ref
MEASURED = {"g": 4.01, "c": 5.77, "k": 1.34}

_by_name = {c["name"]: c for part in ("c", "e") for c in IC.SOLVE[part]}

# Seeds replaced because the first one failed an admission condition of tests/test_jvp_generic_host.py (no condition relaxed):
#   (none)
_REPLACED_SEEDS = {}


def _own(c):
    return dict(c, seed=_REPLACED_SEEDS.get(c["name"], c["seed"]))


CASES = {
    "g": [_own(c) for c in IC.SOLVE["b"]],
    "c": [_own(_by_name[f"g100x3-{n}"]) for n in JC._C_NAMES],
    "k": [_own(_by_name["g100x3-tbatched"]), _own(_by_name["g100x3-sets3x3"])],
    "e": [_own(_by_name["g100x3-budget6"])],
}


def find(part, name):
    return next(c for c in CASES[part] if c["name"] == name)


def direction_sets(part, c, d):
    """(label, v_ode, v_x0) of every launch the GPU tests make on case c of `part`."""
    if part in ("g", "e"):
        return [("unit",) + JC.unit_directions(c)]
    if part == "c":
        return [("unit",) + JC.unit_directions(c), (f"dense{JC.K_DENSE_C}",) + JC.dense_directions(c, d, JC.K_DENSE_C)]
    out = [(f"dense{K}",) + JC.dense_directions(c, d, K) for K in JC.K_TILING]
    vo, vx = JC.dense_directions(c, d, JC.K_POINTERS)
    return out + [("ode-only", vo, None), ("x0-only", None, vx)]


def tolerance(part, method, dt, d_ref):
    if dt == "f64":
        return IC.FP64_TOL[method]
    return min(MARGIN[part] * d_ref, IC.FP32_CAP[method])


# ------------------------------------------------------------------ finite differences (RK4, fp64, tanh 96 x 5)
# The grid 0..240 and the seed are chosen for the REFERENCE: a central difference with relative step 1e-6 carries rounding noise
# eps |y| / (1e-6 |theta dy/dtheta|), so every constant must have moved the trajectory by then (on 0..120 rho and EC_50, the least
# sensitive constants, miss 1e-8 with 4.7e-8 / 1.1e-8 of pure quotient noise; beyond 0..300 RK4's six steps are so long that the
# quotient's O(step^2) term shows, x0:GE 1.6e-5).  On this case the oracle's largest figure is 2.8e-9 (x0:GE).
FD = dict(H=96, L=5, act=IC.TANH, B=3, T=7, seed=901, t_end=240.0, rel_step=1e-6, bound_oracle=1e-8, bound_gpu=1e-7)


def fd_case():
    """fp32-representable arrays (the class surface reads its inputs through fp32): x0 [3,6], t [7], meal [3,7], nn, ode."""
    g = np.random.default_rng(FD["seed"])
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)     # noqa: E731
    x0 = f32(np.array([5., 60., 80., 10., 0.5, 1.]) * (1 + 0.1 * g.standard_normal((FD["B"], 6))))
    t = np.linspace(0.0, FD["t_end"], FD["T"])
    meal = f32(0.05 * g.random((FD["B"], FD["T"])))
    return dict(x0=x0, t=f32(t), meal=meal, nn=f32(IC.rand_net(FD["H"], FD["L"], g)), ode=f32(IC._ode0()))


# ------------------------------------------------------------------ calibration
CAL = dict(H=96, L=3, act=IC.TANH, B=6, T=13, seed=910, rtol=1e-10, atol=1e-12, max_steps=1500, sigma=0.1,
           bound_oracle=1e-7, bound_gpu=1e-6)
CAL_NAMES = ("k_I", "E_max", "k_L")


@functools.lru_cache(maxsize=None)
def calibration_case():
    """dict(x0 [6,6], t [13], meal [6,13], nn, ode (the model's constants), truth {name: [6]}, idx (positions of CAL_NAMES)).
    The observations are the oracle's (tests/test_jvp_generic_host.py: calibration_observations)."""
    from inference.hmc import REFERENCE_PRIORS                 # a table of numbers; nothing is launched
    g = np.random.default_rng(CAL["seed"])
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)     # noqa: E731
    B, T = CAL["B"], CAL["T"]
    x0 = f32(np.array([5.0, 60.0, 80.0, 10.0, 0.0, 1.0]) * (1 + 0.1 * g.standard_normal((B, 6))))
    t = np.linspace(0.0, 240.0, T)
    meal = np.zeros((B, T))
    for b in range(B):
        k = g.integers(1, 5)
        meal[b, k:k + 2] = g.uniform(0.02, 0.08)
    truth = {n: REFERENCE_PRIORS[n][0] + REFERENCE_PRIORS[n][1] * np.clip(g.standard_normal(B), -2, 2) for n in CAL_NAMES}
    idx = [JC.ODE_NAMES.index(n) for n in CAL_NAMES]
    return dict(x0=x0, t=f32(t), meal=f32(meal), nn=f32(IC.rand_net(CAL["H"], CAL["L"], g)), ode=f32(IC._ode0()), truth=truth, idx=idx)


def calibration_observations(O):
    """[6,13,6] the oracle's noise-free records of the six patients (fp64, DP5(4) at CAL's tolerances), each with its own constants."""
    c = calibration_case()
    ys = []
    for b in range(CAL["B"]):
        ode = c["ode"].copy()
        for n, j in zip(CAL_NAMES, c["idx"]):
            ode[j] = c["truth"][n][b]
        sol = O.solve(c["x0"][b:b + 1], c["t"], c["meal"][b:b + 1], None, None, ode, c["nn"], CAL["H"], IC.layers(CAL["L"], CAL["act"]),
                      method=IC.DP5, rtol=CAL["rtol"], atol=CAL["atol"], max_steps=CAL["max_steps"], dtype=np.float64)
        assert int(sol.status[0]) == 0
        ys.append(sol.y[0])
    return np.stack(ys)
