"""Host-side checks of the population model (no GPU): the numpy restatement (tests/_population_reference.py) is its own
transpose, the layout helper, argument errors before any device is touched, a PopulationResult built from arrays, and the
declared / listed / exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import _population_reference as PR

torch = pytest.importorskip("torch")
import hode  # noqa: E402


def hyper_values(K, rng):
    mu0 = rng.uniform(0.01, 10.0, K)
    return mu0, 0.2 * mu0, 0.15 * mu0


@pytest.mark.parametrize("K", [1, 7, 17])
@pytest.mark.parametrize("B", [1, 3])
def test_reference_transpose_equals_central_differences_of_the_reference_map(K, B):
    """<J v, G> = <v, J^T G> with J v from central differences of the map along v.  Bound: relative to the summed magnitudes of
    the terms of <v, J^T G>.  With h = 1e-6 the truncation is h^2 / 6 times third derivatives of order omega^3 (1e-13), and the
    rounding of the difference quotient is eps |theta| / h relative to |J v| ~ sd0 = 0.2 |theta|: 2.2e-16 / 1e-6 / 0.2 = 1.1e-9
    per term, summed in quadrature over few terms: 5e-9 is asserted."""
    rng = np.random.default_rng(100 * K + B)
    mu0, sd0, tau0 = hyper_values(K, rng)
    omega, h, D = 0.5, 1e-6, PR.layout(K, B)["D"]
    for trial in range(4):
        c, v, G = rng.standard_normal(D), rng.standard_normal(D), rng.standard_normal((B, K))
        Jv = (PR.pop_map(c + h * v, K, B, mu0, sd0, tau0, omega) - PR.pop_map(c - h * v, K, B, mu0, sd0, tau0, omega)) / (2 * h)
        g, mag = PR.pop_transpose(c, G, K, B, sd0, tau0, omega)
        lhs, rhs = float((Jv * G).sum()), float(v @ g)
        scale = float(np.abs(v) @ mag)
        assert abs(lhs - rhs) <= 5e-9 * scale, (lhs, rhs, scale)


def test_layout_is_the_documented_row():
    from inference.population import layout
    for K, B in ((1, 1), (7, 3), (17, 5)):
        lay = layout(K, B)
        assert lay == PR.layout(K, B)
        row = np.arange(lay["D"])
        assert lay["D"] == K * (B + 2)
        assert list(row[lay["m"]]) == list(range(K)) and list(row[lay["s"]]) == list(range(K, 2 * K))
        z = row[lay["z"]].reshape(B, K)
        for b in range(B):
            for k in range(K):
                assert z[b, k] == 2 * K + b * K + k
    with pytest.raises(ValueError):
        layout(0, 3)


def test_argument_errors_raise_before_any_device_is_touched(monkeypatch):
    import models.hybrid_ode_nn as HN
    from inference.population import run_population

    def no_device():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(HN, "_compute_device", no_device)
    data = {"initial_state": torch.zeros(3, 6), "observations": torch.zeros(3, 5, 6), "time_points": torch.linspace(0, 1, 5)}
    bad = [dict(ode_priors={"no_such_constant": (1.0, 1.0)}), dict(tau_log_sd=0.0), dict(tau_log_sd=-1.0), dict(tau_scale=0.0),
           dict(tau_scale=-2.0), dict(tau_scale={"a_GI": 0.0}), dict(init=torch.zeros(3, 6)), dict(init=torch.zeros(2, 7)),
           dict(sampler="gibbs"), dict(noise="no_such_mode"), dict(noise_sigma=-1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            run_population(None, data, **kw)
    with pytest.raises(ValueError):
        run_population(None, None)                      # the prior alone needs n_patients


def test_result_from_arrays_maps_raw_draws_as_the_reference_does():
    from inference.population import PopulationResult
    rng = np.random.default_rng(5)
    C, n, B, names = 3, 40, 4, ["a_GI", "V_max", "k_L"]
    K = len(names)
    mu0, sd0, tau0 = hyper_values(K, rng)
    raw = rng.standard_normal((C, n, K * (B + 2)))
    r = PopulationResult(torch.as_tensor(raw), names, B, mu0, sd0, tau0, tau_log_sd=0.4)
    mu, tau = PR.hyper(raw, K, B, mu0, sd0, tau0, 0.4)
    th = PR.pop_map(raw, K, B, mu0, sd0, tau0, 0.4)
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a), b, rtol=1e-14, atol=0)      # noqa: E731
    pop = r.population()
    close(pop["mu"], mu)
    close(pop["tau"], tau)
    assert tuple(r.patients().shape) == (C, n, B, K)
    close(r.patients(), th)
    s = r.samples
    assert list(s) == [f"pop.mu.{k}" for k in names] + [f"pop.tau.{k}" for k in names] + [f"patient.{k}" for k in names]
    for k, name in enumerate(names):
        close(s[f"pop.mu.{name}"], mu[..., k])
        close(s[f"pop.tau.{name}"], tau[..., k])
        assert s[f"patient.{name}"].shape == (C, n, B)
        close(s[f"patient.{name}"], th[..., k])
    assert r.flat()["patient.a_GI"].shape == (C * n, B)
    off = tau[..., None, :] * PR.split(raw, K, B)[2]
    close(r.pooling(), PR.pooling(off.reshape(C * n, B, K)))
    rh, es = r.rhat(), r.ess("mean")
    assert list(rh) == list(s) and rh["patient.k_L"].shape == (B,) and es["pop.tau.a_GI"].shape == ()
    assert r.n_chains == C and r.n_draws == n
    with pytest.raises(ValueError):
        r.predict()
    with pytest.raises(ValueError):
        PopulationResult(torch.zeros(2, 3, 7), names, B, mu0, sd0, tau0)


def test_new_symbols_are_declared_listed_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hode.h")).read()
    declared = set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(hode.lib_path())
    for name in ("hode_pop_params_f32", "hode_pop_params_f64", "hode_pop_grad_f32", "hode_pop_grad_f64"):
        assert name in declared and name in hode.capi.SYMBOLS and hasattr(lib, name), name
    import inference
    assert inference.run_population is not None and "run_population" in inference.__all__ and "PopulationResult" in inference.__all__


def test_return_codes_without_a_launch():
    """A == 0 is HODE_OK; K < 1, K > 17, popcount(ode_mask) != K, B < 1 and ld < K (B + 2) are HODE_EINVAL: checked on the host."""
    lib = hode.load()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    d = ctypes.c_double(0.5)
    u = ctypes.c_uint32

    def params(A, B, K, ld, mask):
        return lib.hode_pop_params_f32(z, A, B, K, ld, one, u(mask), one, one, one, d, one, one)

    def grad(A, B, K, ld, mask):
        return lib.hode_pop_grad_f64(z, A, B, K, ld, one, one, u(mask), one, one, d, one)
    for f in (params, grad):
        assert f(0, 3, 2, 10, 0b11) == 0
        assert f(1, 3, 0, 10, 0) == -1 and f(1, 3, 18, 200, 0x1ffff) == -1
        assert f(1, 3, 2, 10, 0b111) == -1 and f(1, 3, 2, 10, 0b1) == -1
        assert f(1, 0, 2, 10, 0b11) == -1 and f(1, 3, 2, 9, 0b11) == -1
    assert lib.hode_pop_params_f32(z, 1, 3, 2, 10, z, u(3), one, one, one, d, one, one) == -1
