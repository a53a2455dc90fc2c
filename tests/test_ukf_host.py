"""Host-side tests of the unscented Kalman filter: the C ABI's surface and argument validation (no launch,
no GPU), run_ukf's argument errors, and the properties of the numpy restatement tests/_ukf_reference.py that
tests/test_ukf_gpu.py holds the kernel to -- above all that with the identity link it IS a Kalman filter on linear-Gaussian models."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hode

import _ukf_cases as UC
import _ukf_reference as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ surface
def test_header_declares_and_capi_binds_the_ukf_step():
    hdr = open(os.path.join(ROOT, "include", "hode.h")).read()
    declared = set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    lib = hode.load()
    for name in ("hode_ukf_step_f32", "hode_ukf_step_f64"):
        assert name in declared and name in hode.capi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define HODE_UKF_COLS 16\b", hdr) and "Unscented Kalman filter" in hdr
    assert hode.capi.UKF_COLS == UR.COLS == 16 and callable(hode.capi.ukf_step) and callable(hode.capi.ukf_weights)
    assert UR.MOVE == hode.capi.PF_MOVE and UR.LINK == hode.capi.PF_LINK


def test_inference_exports_run_ukf():
    import inference
    assert "run_ukf" in inference.__all__ and "UKFResult" in inference.__all__
    from inference.ukf import UKFResult, run_ukf
    assert inference.run_ukf is run_ukf and inference.UKFResult is UKFResult


POINTERS = ["x_in", "status", "aux_in", "obs", "mask", "sigma", "q", "walk", "dt", "alive", "mean", "cov", "x_out", "aux_out", "stats"]


def _call(sfx="f32", B=1, predict=1, link=1, mode=(0,) * 17, w=(2.6, 0.1, 0.1, 0.07), null=(), alias=()):
    """hode_ukf_step_* with dummy non-null device pointers (never dereferenced: every case here returns before a launch); mode
    is the one host array, and real."""
    p = {n: C.c_void_p(16 * (k + 1)) for k, n in enumerate(POINTERS)}
    for n in null:
        p[n] = C.c_void_p(0)
    for dst, src in alias:
        p[dst] = p[src]
    md = C.c_void_p(0) if mode is None else (C.c_int32 * 17)(*mode)
    f = getattr(hode.load(), f"hode_ukf_step_{sfx}")
    return f(C.c_void_p(0), C.c_int(B), C.c_int(predict), C.c_int(link), md, *(C.c_double(v) for v in w),
             *(p[n] for n in POINTERS))


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_argument_validation_without_gpu(sfx):
    """Every HODE_EINVAL case of the header returns before a launch."""
    EINVAL = -1
    assert _call(sfx, B=0) == EINVAL and _call(sfx, B=-2) == EINVAL
    assert _call(sfx, predict=2) == EINVAL and _call(sfx, predict=-1) == EINVAL
    assert _call(sfx, link=2) == EINVAL and _call(sfx, link=-1) == EINVAL
    for bad in (3, -1, 7):
        for at in (0, 9, 16):
            mode = [0] * 17
            mode[at] = bad
            assert _call(sfx, mode=mode) == EINVAL, (bad, at)
    assert _call(sfx, mode=None) == EINVAL
    for gamma in (0.0, -1.0, math.nan, math.inf):
        assert _call(sfx, w=(gamma, 0.1, 0.1, 0.07)) == EINVAL, gamma
    for k in (1, 2, 3):
        for bad in (math.nan, math.inf, -math.inf):
            w = [2.6, 0.1, 0.1, 0.07]
            w[k] = bad
            assert _call(sfx, w=w) == EINVAL, (k, bad)
    for name in POINTERS:
        if name not in ("status", "mask"):                              # (the two optional ones)
            assert _call(sfx, null=(name,)) == EINVAL, name
    assert _call(sfx, alias=(("x_out", "x_in"),)) == EINVAL
    assert _call(sfx, alias=(("aux_out", "aux_in"),)) == EINVAL


def test_run_ukf_rejects_bad_arguments_before_any_launch():
    import torch
    from inference import ParameterLearning, run_ukf
    from inference.observation import ObservationModel
    from models import HybridODENN
    m = HybridODENN(nn_hidden=8, nn_layers=1, device="cpu")
    data = {"initial_state": torch.ones(2, 6), "time_points": torch.linspace(0, 1, 4), "observations": torch.ones(2, 4, 6)}
    with pytest.raises(ValueError, match="noise_link"):
        run_ukf(m, data, noise_link="probit")
    with pytest.raises(ValueError, match="dtype"):
        run_ukf(m, data, dtype=torch.float16)
    with pytest.raises(ValueError, match="process_noise"):
        run_ukf(m, data, process_noise=-0.1)
    with pytest.raises(ValueError, match="initial_spread"):
        run_ukf(m, data, initial_spread=[0.1, 0.2])
    with pytest.raises(ValueError, match="marginal"):
        run_ukf(m, data, noise_sigma=ObservationModel(1.0, noise="marginal"))
    with pytest.raises(ValueError, match="ascending"):
        run_ukf(m, data, steps=[2, 1])
    with pytest.raises(ValueError, match="initial_state"):
        run_ukf(m, dict(data, initial_state=torch.ones(2, 5)))
    with pytest.raises(ValueError, match="observations"):
        run_ukf(m, dict(data, observations=torch.ones(2, 3, 6)))
    with pytest.raises(ValueError, match="ParameterLearning"):
        run_ukf(m, data, learn={"names": ["k_empt"]})
    name = hode_param_name()
    with pytest.raises(ValueError, match="initial_spread > 0 or walk > 0"):
        run_ukf(m, data, learn=ParameterLearning([name]))
    with pytest.raises(ValueError, match="lambda"):
        run_ukf(m, data, kappa=-6.0)
    with pytest.raises(ValueError, match="lambda"):
        run_ukf(m, data, learn=ParameterLearning([name], initial_spread=0.1), kappa=-7.0)
    with pytest.raises(ValueError, match="lambda"):
        run_ukf(m, data, alpha=0.0)
    with pytest.raises(ValueError, match="beta"):
        run_ukf(m, data, beta=math.nan)


def hode_param_name():
    from models.ode_core import ODE_PARAM_NAMES
    return ODE_PARAM_NAMES[3]


def test_ukf_weights_follow_the_formulas():
    for n, a, b, k in ((6, 1.0, 0.0, 1.0), (23, 1.0, 0.0, 1.0), (9, 0.5, 2.0, 0.0), (7, 1e-1, 2.0, 3.0 - 7), (6, 1.0, 0.0, 2.0)):
        lam = a * a * (n + k) - n
        gamma, wm0, wc0, wi = hode.capi.ukf_weights(n, a, b, k)
        assert gamma == math.sqrt(n + lam) and wm0 == lam / (n + lam) and wc0 == wm0 + 1 - a * a + b and wi == 1 / (2 * (n + lam))
        assert abs(wm0 + 2 * n * wi - 1) < 1e-12
        assert (gamma, wm0, wc0, wi) == UR.weights(n, a, b, k)
    assert min(hode.capi.ukf_weights(6)) > 0 and min(hode.capi.ukf_weights(23)) > 0        # the defaults: all weights positive
    with pytest.raises(hode.capi.HodeError):
        hode.capi.ukf_weights(6, 1.0, 0.0, -6.0)


# ------------------------------------------------------------------ the restatement is a Kalman filter on linear-Gaussian models
def _restated(M):
    w = UR.weights(M["n"])

    def fn(x, aux, obs, dt, alive, mean, cov, predict):
        return UR.step(x, aux, M["mode"], obs, M["sigma"], M["q"], M["walk"], dt, alive, mean, cov, w, predict=predict, link=0)
    return fn


@pytest.mark.parametrize("which", [1, 2])
def test_identity_link_reproduces_the_kalman_filter(which):
    M = UC.linear_model(which)
    kal, ukf = UC.kalman(M), UC.ukf_on_linear_model(M, _restated(M))
    worst = [0.0, 0.0, 0.0]
    for (e0, m0, P0), (e1, m1, P1) in zip(kal, ukf):
        worst = [max(worst[0], abs(e0 - e1)), max(worst[1], np.abs(m0 - m1).max()), max(worst[2], np.abs(P0 - P1).max())]
    print(f"model {which}: evidence {worst[0]:.2e}, mean {worst[1]:.2e}, covariance {worst[2]:.2e}")
    assert max(worst) <= 1e-12
    if which == 2:                                                     # the singular start: a zero column, an exact coordinate
        assert M["P0"][1, 1] == 0.0 and UR.cholesky(M["P0"])[1] == [1]


def test_a_step_without_observations_changes_nothing_and_adds_exactly_zero():
    M = UC.linear_model(1)
    assert not np.isfinite(M["ys"][4]).any()
    fn = _restated(M)
    seen = []

    def spy(x, aux, obs, dt, alive, mean, cov, predict):
        r = fn(x, aux, obs, dt, alive, mean, cov, predict)
        seen.append(r)
        return r
    UC.ukf_on_linear_model(M, spy)
    r = seen[4]
    assert r["stats"][0] == 0.0 and r["stats"][1] == 0.0 and r["stats"][2] == 0 and r["stats"][3] == 1
    assert np.array_equal(r["mean"], r["m_pred"]) and np.array_equal(r["cov"], r["P_pred"])
    # and with the moments given (predict == 0), they come back bit for bit, under a mask as under NaN
    c = UC.case(UC.SPECS.index(dict(P=2, B=3, link=1, predict=0, mask="none")))
    for kw in (dict(obs=c["obs"][0]), dict(obs=UC.SCALE, mask=np.zeros(6, dtype=np.uint8))):
        r = UR.step(c["x_in"][0], c["aux_in"][0], c["mode"], kw["obs"], c["sigma"], c["q"], c["walk"], 1.0, 1, c["mean"][0], c["cov"][0],
                    c["w"], predict=False, link=1, mask=kw.get("mask"))
        assert np.array_equal(r["mean"], c["mean"][0]) and np.array_equal(r["cov"], c["cov"][0]) and r["stats"][0] == 0.0


def test_a_zero_covariance_gives_equal_points_and_a_zero_column_stays_exact():
    idx = UC.SPECS.index(dict(P=1, B=3, link=1, predict=0, mask="one", edge="zero_cov"))
    c = UC.case(idx)
    assert not c["cov"].any()
    for r in UC.reference(idx):
        assert r["alive"] == 1 and (r["x_out"] == r["x_out"][0]).all() and (r["aux_out"] == r["aux_out"][0]).all()
        # (the unscented mean of K equal values v is v up to the rounding of sum w_k v, so the variance is 0 up to its square)
        assert not r["cov"].any() and (r["stats"][10:16] <= (8 * UR.EPS * r["stats"][4:10]) ** 2).all()
    for link in (0, 1):                                                # a state with no spread in and q = 0: an exact zero column
        idx = UC.SPECS.index(dict(P=1, B=3, link=link, predict=1, mask="complete", edge="zero_state"))
        for r in UC.reference(idx):
            assert not r["P_pred"][2].any() and not r["P_pred"][:, 2].any() and (r["x_out"][:, 2] == 1.0).all()
            assert not r["cov"][2].any() and r["stats"][6] == 1.0 and r["stats"][12] == 0.0
            assert r["cov"][0, 0] > 0 and np.ptp(r["x_out"][:, 0]) > 0


def test_a_lost_patient_stays_lost():
    idx = UC.SPECS.index(dict(P=1, B=3, link=1, predict=1, mask="complete", edge="lost_status"))
    c = UC.case(idx)
    r = UC.reference(idx)[1]
    assert r["alive"] == 0 and r["stats"][0] == -math.inf and r["stats"][2] == 6 and r["stats"][3] == 0
    assert np.isnan(r["stats"][[1] + list(range(4, 16))]).all() and np.isnan(r["mean"]).all() and np.isnan(r["cov"]).all()
    assert np.array_equal(r["x_out"], c["x_in"][1]) and np.array_equal(r["aux_out"], c["aux_in"][1])
    # the next step, on perfectly good inputs
    good = UC.reference(idx)[0]
    again = UR.step(good["x_out"], good["aux_out"], c["mode"], c["obs"][1], c["sigma"], c["q"], c["walk"], 1.0, r["alive"], r["mean"], r["cov"],
                    c["w"], predict=True, link=1)
    assert again["alive"] == 0 and again["stats"][0] == -math.inf and np.array_equal(again["x_out"], good["x_out"])
    for edge, lost in (("lost_entry", 1), ("lost_nan", 1), ("lost_nan_par", 2), ("lost_nonpos", 1), ("lost_nonpos_par", 0)):
        for i, s in enumerate(UC.SPECS):
            if s.get("edge") == edge:
                assert [r["alive"] for r in UC.reference(i)] == [0 if b == lost else 1 for b in range(s["B"])], (edge, i)


# ------------------------------------------------------------------ the GPU file's cases are well conditioned
@pytest.mark.parametrize("idx", range(len(UC.SPECS)), ids=[UC.case_id(s) for s in UC.SPECS])
def test_gpu_cases_keep_the_condition_numbers_within_the_cap(idx):
    """The GPU test's tolerance is 64 n c 2^-52 with c the larger condition number of P- (on its non-zero columns) and S; the
    cases keep c <= 1e6 (far below: the bound stays meaningful)."""
    for r in UC.reference(idx):
        assert 1.0 <= r["cond"] <= UC.COND_CAP, r["cond"]
