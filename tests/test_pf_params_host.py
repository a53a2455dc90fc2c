"""Host-side tests of the particle filter's parameter move: the C ABI's surface and argument validation
(no launch, no GPU), ParameterLearning / run_filter(learn=...) validation, the properties of the numpy restatement
tests/_pf_params_reference.py that tests/test_pf_params_gpu.py holds the kernel to, and the method itself against an augmented
Kalman filter on a linear-Gaussian model with an unknown drift."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hode

import _filter_reference as FR
import _pf_params_cases as PC
import _pf_params_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ surface
def test_header_declares_and_capi_binds_the_parameter_move():
    hdr = open(os.path.join(ROOT, "include", "hode.h")).read()
    declared = set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    lib = hode.load()
    for name in ("hode_pf_params_f32", "hode_pf_params_f64"):
        assert name in declared and name in hode.capi.SYMBOLS and hasattr(lib, name), name
    assert "Particle filter: parameter move" in hdr
    for macro, value in (("HODE_PF_MOVE_CARRIED", 0), ("HODE_PF_MOVE_IDENTITY", 1), ("HODE_PF_MOVE_LOG", 2)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    assert hode.capi.PF_MOVE == {"carried": 0, "identity": 1, "log": 2} and callable(hode.capi.pf_params)
    philox = open(os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd", "csrc", "hode_philox.h")).read()
    assert re.search(r"kRngFilterParam = 11\b", philox)
    assert PR.PARAM == 11 and (PR.CARRIED, PR.IDENTITY, PR.LOG) == (0, 1, 2)


def test_inference_exports_parameter_learning():
    import inference
    from inference.filter import LearnedParameters, ParameterLearning
    assert "ParameterLearning" in inference.__all__ and inference.ParameterLearning is ParameterLearning
    assert inference.LearnedParameters is LearnedParameters


def _call(sfx="f32", B=1, N=8, n_aux=3, shrink=0.9, null=()):
    """hode_pf_params_* with dummy non-null pointers (never dereferenced: every case here returns before a launch)."""
    names = ["lw", "aux", "mode", "walk", "dt", "pstats"]
    p = {n: C.c_void_p(16 * (k + 1)) for k, n in enumerate(names)}
    for n in null:
        p[n] = C.c_void_p(0)
    f = getattr(hode.load(), f"hode_pf_params_{sfx}")
    return f(C.c_void_p(0), C.c_int(B), C.c_int(N), C.c_uint32(0), C.c_uint64(1), C.c_uint32(0), p["lw"], C.c_int(n_aux), p["aux"],
             p["mode"], p["walk"], p["dt"], C.c_double(shrink), p["pstats"])


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_argument_validation_without_gpu(sfx):
    """Every HODE_EINVAL / HODE_EUNSUPPORTED case of the header returns before a launch."""
    EINVAL, EUNSUPPORTED = -1, -2
    assert _call(sfx, B=0) == EINVAL and _call(sfx, B=-3) == EINVAL
    assert _call(sfx, N=0) == EINVAL and _call(sfx, N=-1) == EINVAL
    assert _call(sfx, n_aux=0) == EINVAL and _call(sfx, n_aux=-1) == EINVAL and _call(sfx, n_aux=18) == EINVAL
    for bad in (-0.01, 1.01, math.nan, math.inf):
        assert _call(sfx, shrink=bad) == EINVAL, bad
    for name in ("lw", "aux", "mode", "walk", "dt", "pstats"):
        assert _call(sfx, null=(name,)) == EINVAL, name
    assert _call(sfx, N=4097) == EUNSUPPORTED
    assert _call(sfx, N=4097, shrink=2.0) == EINVAL               # a bad argument outranks the unsupported size
    assert _call(sfx, N=4097, null=("aux",)) == EINVAL


def test_parameter_learning_rejects_bad_arguments():
    from inference import ParameterLearning
    with pytest.raises(ValueError, match="at least one"):
        ParameterLearning([])
    with pytest.raises(ValueError, match="unknown mechanistic constant"):
        ParameterLearning(["no_such_constant"])
    with pytest.raises(ValueError, match="twice"):
        ParameterLearning(["a_GI", "ode_a_GI"])
    with pytest.raises(ValueError, match="link"):
        ParameterLearning(["a_GI"], link="probit")
    for bad in (1.0 / 3.0, 0.2, 1.01, math.nan):
        with pytest.raises(ValueError, match="discount"):
            ParameterLearning(["a_GI"], discount=bad)
    for kw in (dict(walk=-0.1), dict(walk=[0.1, 0.2]), dict(walk=math.nan), dict(walk=math.inf)):
        with pytest.raises(ValueError, match="walk"):
            ParameterLearning(["a_GI"], **kw)
    for kw in (dict(initial_spread=-0.1), dict(initial_spread=[0.1, 0.2, 0.3]), dict(initial_spread=math.nan)):
        with pytest.raises(ValueError, match="initial_spread"):
            ParameterLearning(["a_GI", "k_I"], **kw)
    p = ParameterLearning(["ode_a_GI", "k_I"], discount=0.95, walk=[0.0, 0.2], initial_spread=0.3, link="identity")
    assert p.names == ["a_GI", "k_I"] and p.link == "identity" and p.walk.tolist() == [0.0, 0.2] and p.initial_spread.tolist() == [0.3, 0.3]
    assert p.shrink == (3 * 0.95 - 1) / (2 * 0.95) and ParameterLearning("a_GI", discount=1.0).shrink == 1.0


def test_run_filter_rejects_a_bad_learn_before_any_launch():
    import torch
    from inference import run_filter
    from models import HybridODENN
    m = HybridODENN(nn_hidden=8, nn_layers=1, device="cpu")
    data = {"initial_state": torch.ones(2, 6), "time_points": torch.linspace(0, 1, 4), "observations": torch.ones(2, 4, 6)}
    with pytest.raises(ValueError, match="ParameterLearning"):
        run_filter(m, data, n_particles=4, learn=["a_GI"])
    with pytest.raises(ValueError, match="ParameterLearning"):
        run_filter(m, data, n_particles=4, learn={"names": ["a_GI"]})


# ------------------------------------------------------------------ the restatement's properties
def _cloud(rng, N, n_aux=5):
    aux = PC.SCALE[:n_aux] * np.exp(0.3 * rng.standard_normal((N, n_aux)))
    return aux, 0.5 * rng.standard_normal(N)


def test_skipped_carried_and_dead_entries_are_untouched():
    rng = np.random.default_rng(1)
    aux, lw = _cloud(rng, 40)
    lw[[3, 17]] = -np.inf
    lw[9] = np.nan
    aux[5, 2] = np.inf                                           # a non-finite selected value: the row does not count
    mode, walk = [PR.LOG, PR.CARRIED, PR.IDENTITY, PR.LOG, PR.CARRIED], [0.1, 0.3, 0.0, 0.0, 0.3]
    r = PR.move(lw, aux, mode, walk, 2.0, 1.0, 4, seed=3, key=1)
    dead = [3, 5, 9, 17]
    assert not r["counts"][dead].any() and r["counts"].sum() == 36
    assert np.array_equal(r["aux"][dead], aux[dead])                                  # dead rows
    assert np.array_equal(r["aux"][:, [1, 4]], aux[:, [1, 4]]) and np.isnan(r["pstats"][[2, 3, 8, 9]]).all()   # carried columns
    assert np.array_equal(r["aux"][:, [2, 3]], aux[:, [2, 3]]) and np.isfinite(r["pstats"][[4, 5, 6, 7]]).all()  # a = 1, walk = 0
    live = np.delete(np.arange(40), dead)
    assert (r["aux"][live, 0] != aux[live, 0]).all()
    r = PR.move(np.full(40, -np.inf), aux, mode, walk, 2.0, 0.9, 4)
    assert np.array_equal(r["aux"], aux) and np.isnan(r["pstats"]).all()               # nobody counts


def test_a_constant_added_to_the_log_weights_changes_nothing():
    rng = np.random.default_rng(2)
    aux, lw = _cloud(rng, 50)
    kw = dict(mode=[PR.LOG, PR.IDENTITY, 0, 0, PR.LOG], walk=[0.1, 0.0, 0, 0, 0.05], dt=1.5, shrink=0.95, step=2, seed=9, key=1)
    a, b = PR.move(lw, aux, **kw), PR.move(lw + 8.0, aux, **kw)
    np.testing.assert_allclose(a["pstats"], b["pstats"], rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(a["aux"], b["aux"], rtol=1e-12, atol=0)


def test_the_draws_of_a_column_do_not_depend_on_which_other_columns_are_moved():
    rng = np.random.default_rng(3)
    aux, lw = _cloud(rng, 30, 17)
    walk = np.full(17, 0.1)
    kw = dict(dt=1.0, shrink=0.9, step=6, seed=11, key=4)
    every = PR.move(lw, aux, np.full(17, PR.LOG), walk, **kw)
    for k in (0, 3, 4, 16):
        one = np.zeros(17, dtype=int)
        one[k] = PR.LOG
        alone = PR.move(lw, aux, one, walk, **kw)
        assert np.array_equal(alone["aux"][:, k], every["aux"][:, k]), k
        assert np.array_equal(np.delete(alone["aux"], k, 1), np.delete(aux, k, 1))
    # and the four columns of a group share a block, a fifth starts the next one
    assert PR.epsilon(11, 4, 6, 2, 3) == PR.normals4(PR.hmc_rng(11, 4, 6, 11, 10))[3]
    assert PR.epsilon(11, 4, 6, 2, 4) == PR.normals4(PR.hmc_rng(11, 4, 6, 11, 11))[0]
    assert PR.epsilon(11, 4, 6, 2, 16) == PR.normals4(PR.hmc_rng(11, 4, 6, 11, 14))[0]


def test_the_log_link_keeps_every_value_positive_and_the_shrinkage_keeps_the_moments():
    rng = np.random.default_rng(4)
    N = 2000
    aux = 0.01 * np.exp(1.5 * rng.standard_normal((N, 1)))       # a very wide cloud: additive noise of its size would cross zero
    lw = 0.5 * rng.standard_normal(N)
    r = PR.move(lw, aux, [PR.LOG], [2.0], 1.0, 0.7, 1, seed=5)
    assert (r["aux"] > 0).all() and np.isfinite(r["aux"]).all()
    # Liu & West's shrinkage keeps the weighted mean and variance in expectation: the moved cloud's moments lie within 5
    # standard errors (N draws of variance (1 - a^2) V each) of the ones before the move
    r = PR.move(lw, aux, [PR.LOG], [0.0], 1.0, 0.7, 1, seed=5)
    after = PR.move(lw, r["aux"], [PR.LOG], [0.0], 1.0, 1.0, 1)["pstats"]
    mean, var = r["pstats"]
    w = np.exp(lw - lw.max())
    n_eff = w.sum() ** 2 / (w * w).sum()
    assert abs(after[0] - mean) < 5 * math.sqrt((1 - 0.49) * var / n_eff)
    assert abs(after[1] - var) < 5 * var * math.sqrt(2.0 / n_eff)


# ------------------------------------------------------------------ the GPU file's bounds hold under another summation order
@pytest.mark.parametrize("idx", range(len(PC.CASES)), ids=[PC.case_id(c) for c in PC.CASES])
def test_another_summation_order_stays_inside_the_bound_of_the_case(idx):
    """The restatement with the sums taken sequentially from the last particle to the first, in place of math.fsum: what it
    changes in pstats and in the moved values lies inside the bound tests/test_pf_params_gpu.py allows the kernel."""
    d = PC.inputs(idx)
    backwards = lambda v: float(sum(reversed(v), 0.0))                                                       # noqa: E731
    worst = 0.0
    for b, ref in enumerate(PC.reference(idx)):
        alt = PC.restate(d, b, total=backwards)
        bd = PC.bounds(d, b, ref)
        assert np.array_equal(alt["counts"], ref["counts"]) and np.array_equal(np.isnan(alt["pstats"]), np.isnan(ref["pstats"]))
        assert np.array_equal(np.isnan(alt["phi_new"]), np.isnan(ref["phi_new"]))
        for k, o in bd.items():
            assert abs(alt["pstats"][2 * k] - ref["pstats"][2 * k]) <= o["mean"], (b, k)
            assert abs(alt["pstats"][2 * k + 1] - ref["pstats"][2 * k + 1]) <= o["var"], (b, k)
            if "value_abs" in o:
                live = ref["counts"]
                err = np.abs(alt["aux"][live, k] - ref["aux"][live, k])
                tol = o["value_abs"] + o["value_rel"] * np.abs(ref["aux"][live, k])
                assert (err <= tol).all(), (b, k)
                worst = max(worst, float((err / tol).max()))
                # the bound must stay far below an fp32 ulp (2^-24 relative) for the fp32 one-ulp criterion to mean anything
                assert o["value_rel"] < 2.0 ** -30 and o["value_abs"] < 2.0 ** -30 * np.abs(ref["aux"][live, k]).max()
    print("worst error / bound", worst)


# ------------------------------------------------------------------ the method: an unknown drift, against an augmented Kalman filter
S_STEPS, N_PART, DELTA, SEEDS = 25, 256, 0.95, 64
Q0, Q, SIGMA, THETA0, SPREAD0 = 0.5, 0.3, 0.5, 0.0, 0.5
SPREAD_STEP = 0xFFFFFFFF


def _model_data():
    rng = np.random.default_rng(21)
    dts = np.concatenate([[1.0], 0.5 + rng.random(S_STEPS - 1)])
    theta = THETA0 + SPREAD0 * rng.standard_normal()
    x = 1.0 + Q0 * rng.standard_normal()
    ys = []
    for s in range(S_STEPS):
        if s > 0:
            x = x + theta * dts[s] + Q * math.sqrt(dts[s]) * rng.standard_normal()
        ys.append(x + SIGMA * rng.standard_normal())
    return dts, np.array(ys), theta


def _kalman(dts, ys):
    """The posterior mean and sd of the drift under z = (x, theta): x_s = x_{s-1} + theta dt_s + N(0, Q^2 dt_s), theta constant,
    y_s = x_s + N(0, SIGMA^2); x_0 ~ N(1, Q0^2), theta ~ N(THETA0, SPREAD0^2), independent."""
    m, P = np.array([1.0, THETA0]), np.diag([Q0 ** 2, SPREAD0 ** 2])
    H = np.array([[1.0, 0.0]])
    for s, y in enumerate(ys):
        if s > 0:
            F = np.array([[1.0, dts[s]], [0.0, 1.0]])
            m, P = F @ m, F @ P @ F.T + np.diag([Q ** 2 * dts[s], 0.0])
        Sy = H @ P @ H.T + SIGMA ** 2
        K = P @ H.T / Sy
        m, P = m + (K * (y - H @ m)).reshape(-1), (np.eye(2) - K @ H) @ P
    return float(m[1]), math.sqrt(P[1, 1])


def _filter(seed, dts, ys, variant):
    """The restated filter (FR.step, the drift in aux, a matrix product as the solve, identity link) with the restated move.
    variant: "fsum" the restatement as it is; "backwards" its sums in another order; "noshrink" the shrinkage dropped;
    "none" no move after the initial spread.  Returns (weighted mean, weighted sd, distinct values) of the final drifts."""
    N = N_PART
    a = (3 * DELTA - 1) / (2 * DELTA)
    x = np.zeros((N, 6))
    x[:, 0] = 1.0
    aux, lw = np.full((N, 1), THETA0), np.zeros(N)
    sigma = np.full(6, SIGMA)
    obs = np.full(6, np.nan)
    total = (lambda v: float(sum(reversed(v), 0.0))) if variant == "backwards" else math.fsum
    for s in range(S_STEPS):
        if s > 0:
            z = np.column_stack([x[:, 0], aux[:, 0]]) @ np.array([[1.0, dts[s]], [0.0, 1.0]]).T
            x = x.copy()
            x[:, 0] = z[:, 0]
        obs[0] = ys[s]
        q = np.array([Q0 if s == 0 else Q, 0, 0, 0, 0, 0.0])
        r = FR.step(x, obs, sigma, q, dts[s], lw, s, seed=seed, key=0, link=0, ess_frac=0.5, aux=aux)
        x, lw, aux = r["x_out"], r["lw"], r["aux_out"]
        if s == 0:
            aux = PR.move(lw, aux, [PR.IDENTITY], [SPREAD0], 1.0, 1.0, SPREAD_STEP, seed=seed, key=0)["aux"]
        if variant != "none":
            aux = PR.move(lw, aux, [PR.IDENTITY], [0.0], dts[s], a, s, seed=seed, key=0, total=total, shrinkage=variant != "noshrink")["aux"]
    w = np.exp(lw - lw.max())
    w /= w.sum()
    mean = float((w * aux[:, 0]).sum())
    return mean, math.sqrt(float((w * (aux[:, 0] - mean) ** 2).sum())), len(np.unique(aux[:, 0]))


@pytest.fixture(scope="module")
def method():
    dts, ys, theta = _model_data()
    k_mean, k_sd = _kalman(dts, ys)
    runs = {v: np.array([_filter(seed, dts, ys, v) for seed in range(SEEDS)]) for v in ("fsum", "backwards", "noshrink", "none")}
    for v, r in runs.items():
        ratio = r[:, 1] / k_sd
        print(f"{v:9s}: drift mean {r[:, 0].mean():+.4f} (Kalman {k_mean:+.4f}, truth {theta:+.4f}), z "
              f"{(r[:, 0].mean() - k_mean) / (r[:, 0].std(ddof=1) / math.sqrt(SEEDS)):+.2f}; sd ratio {ratio.mean():.3f} +- "
              f"{ratio.std(ddof=1) / math.sqrt(SEEDS):.3f}; distinct median {np.median(r[:, 2]):.0f}, max {r[:, 2].max():.0f}")
    return runs, k_mean, k_sd


def _ratio(r, k_sd):
    v = r[:, 1] / k_sd
    return float(v.mean()), float(v.std(ddof=1) / math.sqrt(len(v)))


def test_the_learned_drift_agrees_with_the_augmented_kalman_filter(method):
    """25 steps, N = 256, delta = 0.95, 64 seeds: the final mean of the drift over the seeds lies within 4 standard errors of
    the Kalman filter's."""
    runs, k_mean, _ = method
    means = runs["fsum"][:, 0]
    assert abs(means.mean() - k_mean) < 4 * means.std(ddof=1) / math.sqrt(SEEDS)


def test_the_spread_of_the_cloud_is_a_property_of_the_method_not_of_rounding(method):
    """The seed-mean ratio (cloud sd / Kalman sd) is the same, within 4 of its standard errors, when the restatement sums in
    another order."""
    runs, _, k_sd = method
    (r0, se0), (r1, se1) = _ratio(runs["fsum"], k_sd), _ratio(runs["backwards"], k_sd)
    assert abs(r0 - r1) < 4 * math.hypot(se0, se1)


def test_the_move_keeps_every_drift_distinct_where_the_bare_filter_collapses(method):
    runs, _, _ = method
    assert (runs["fsum"][:, 2] == N_PART).all()
    assert (runs["none"][:, 2] < N_PART / 4).all()


def test_without_the_shrinkage_the_same_comparison_fails(method):
    """The control: phi' = phi + sd eps (the noise without the shrinkage that pays for it) inflates the cloud at every step; its
    sd ratio is NOT within 4 standard errors of the method's."""
    runs, _, k_sd = method
    (r0, se0), (r2, se2) = _ratio(runs["backwards"], k_sd), _ratio(runs["noshrink"], k_sd)
    assert not abs(r2 - r0) < 4 * math.hypot(se0, se2)
    assert r2 > r0
