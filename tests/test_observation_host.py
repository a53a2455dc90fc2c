"""The observation model on the host (inference/observation.py): validation, the observed set and its counts from NaN and an
explicit mask, the noise draws against the inverse-gamma moments, the constants, the C ABI's new symbols, and the samplers'
argument validation up to the point where a device is needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

import hode
from inference.observation import ObservationModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validation():
    om = ObservationModel()
    assert om.sigma.tolist() == [1.0] * 6 and not om.marginal and om.scalar_sigma
    om = ObservationModel([1, 2, 3, 4, 5, 6])
    assert om.sigma.tolist() == [1, 2, 3, 4, 5, 6] and not om.scalar_sigma and np.allclose(om.w, 1 / om.sigma ** 2)
    assert ObservationModel(torch.tensor([0.5] * 6)).scalar_sigma
    om = ObservationModel(0.5, "marginal")
    assert om.a.tolist() == [2.0] * 6 and om.b.tolist() == [0.25] * 6            # prior mean of sigma^2 = b / (a - 1) = 0.25
    om = ObservationModel(0.5, "marginal", noise_prior=(3.0, [1, 2, 3, 4, 5, 6]))
    assert om.a.tolist() == [3.0] * 6 and om.b.tolist() == [1, 2, 3, 4, 5, 6]
    for bad in (0.0, -1.0, float("nan"), [1, 2, 3], [1, 2, 3, 4, 5, 0]):
        with pytest.raises(ValueError):
            ObservationModel(bad)
    with pytest.raises(ValueError):
        ObservationModel(1.0, "sampled")
    with pytest.raises(ValueError):
        ObservationModel(1.0, "fixed", noise_prior=(2.0, 1.0))
    with pytest.raises(ValueError):
        ObservationModel(1.0, "marginal", noise_prior=(2.0, -1.0))
    with pytest.raises(ValueError):
        ObservationModel(1.0, "marginal", noise_prior=(2.0,))
    with pytest.raises(RuntimeError):
        ObservationModel().log_norm()


def test_observed_set_counts_and_mask():
    g = torch.Generator().manual_seed(0)
    obs = torch.randn(3, 5, 6, generator=g)
    om = ObservationModel().prepare(obs)
    assert om.complete and om.mask is None and om.n.tolist() == [15.0] * 6 and not om.needs_kernel
    assert ObservationModel([1, 1, 1, 1, 1, 2]).prepare(obs).needs_kernel and ObservationModel(1.0, "marginal").prepare(obs).needs_kernel
    o2 = obs.clone()
    o2[0, 0, 0] = float("nan")
    o2[1, 2, 3] = float("inf")
    o2[:, :, 4] = float("nan")                                                 # a state observed nowhere is legal
    om = ObservationModel().prepare(o2)
    assert not om.complete and om.needs_kernel and om.n.tolist() == [14.0, 15.0, 15.0, 14.0, 0.0, 15.0]
    assert om.mask.dtype == torch.uint8 and tuple(om.mask.shape) == (3, 30) and tuple(om.obs.shape) == (3, 30)
    assert torch.equal(om.mask.view(3, 5, 6).bool(), torch.isfinite(o2))
    mask = torch.ones(3, 5, 6, dtype=torch.bool)
    mask[2, :, 1] = False
    om = ObservationModel().prepare(o2, mask)
    assert om.n.tolist() == [14.0, 10.0, 15.0, 14.0, 0.0, 15.0]
    assert torch.equal(om.mask.view(3, 5, 6).bool(), torch.isfinite(o2) & mask)
    om64 = ObservationModel().prepare(o2, mask, dtype=torch.float64)
    assert om64.obs.dtype == torch.float64
    with pytest.raises(ValueError):
        ObservationModel().prepare(torch.full((3, 5, 6), float("nan")))
    with pytest.raises(ValueError):
        ObservationModel().prepare(obs, torch.zeros(3, 5, 6, dtype=torch.bool))
    with pytest.raises(ValueError):
        ObservationModel().prepare(obs, torch.ones(3, 5, 5, dtype=torch.bool))
    with pytest.raises(ValueError):
        ObservationModel().prepare(torch.randn(3, 5, 4))


def test_sample_noise_moments():
    """sigma^2 ~ InvGamma(alpha, beta) with alpha = a + n/2, beta = b + SSE/2: mean beta / (alpha - 1), variance
    beta^2 / ((alpha - 1)^2 (alpha - 2)).  Tolerance: 5 Monte-Carlo standard errors of the N draws (the standard error of the
    sample variance from the draws' own fourth moment)."""
    N = 200000
    obs = torch.zeros(4, 5, 6)
    obs[:, :, 5] = float("nan")
    om = ObservationModel([0.5, 1, 2, 3, 4, 5], "marginal", noise_prior=(2.0, [1, 2, 3, 4, 5, 6])).prepare(obs)
    sse = torch.tensor([3.0, 10.0, 0.5, 40.0, 7.0, 0.0], dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    sig = om.sample_noise(sse.expand(N, 6), g)
    assert tuple(sig.shape) == (N, 6) and bool((sig > 0).all())
    v = sig ** 2
    al = torch.as_tensor(om.a + 0.5 * om.n)
    be = torch.as_tensor(om.b) + 0.5 * sse
    assert al.tolist() == [12.0] * 5 + [2.0]                                  # the unobserved state: its prior
    mean, var = be / (al - 1), be ** 2 / ((al - 1) ** 2 * (al - 2))
    se_mean = v.std(0) / math.sqrt(N)
    assert bool(((v.mean(0) - mean).abs() < 5 * se_mean)[:5].all()), (v.mean(0), mean, se_mean)
    c = v - v.mean(0)
    se_var = torch.sqrt(((c ** 4).mean(0) - (c ** 2).mean(0) ** 2) / N)
    assert bool(((v.var(0) - var).abs() < 5 * se_var)[:5].all()), (v.var(0), var, se_var)
    # alpha = 2 has no finite variance: check the mean of sigma itself, sqrt(beta) Gamma(1.5) / Gamma(2), finite variance beta - mean^2
    want = math.sqrt(float(be[5])) * math.gamma(1.5)
    assert abs(float(sig[:, 5].mean()) - want) < 5 * math.sqrt((float(be[5]) - want ** 2) / N)
    # the same generator state, the same draws; fixed mode repeats the fixed values
    assert torch.equal(sig, om.sample_noise(sse.expand(N, 6), torch.Generator().manual_seed(1)))
    fx = ObservationModel([1, 2, 3, 4, 5, 6]).sample_noise(torch.zeros(3, 6))
    assert fx.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]] * 3


def test_log_norm_is_the_gaussian_and_student_constant():
    obs = torch.zeros(2, 3, 6)
    obs[:, :, 2] = float("nan")
    sig = np.array([0.5, 1, 2, 3, 4, 5.0])
    om = ObservationModel(sig).prepare(obs)
    n = np.array([6, 6, 0, 6, 6, 6.0])
    assert math.isclose(om.log_norm(), float(np.sum(n * np.log(sig * math.sqrt(2 * math.pi)))), rel_tol=1e-14)
    # marginal, one state, against numerical integration over sigma^2 of prod N(r | 0, sigma^2) InvGamma(sigma^2 | a, b)
    o1 = torch.full((1, 4, 6), float("nan"))
    r = np.array([0.3, -1.1, 0.7, 0.2])
    o1[0, :, 0] = torch.tensor(r)
    a, b = 2.5, 0.8
    om = ObservationModel(1.0, "marginal", noise_prior=(a, b)).prepare(o1)
    sse = float(np.sum(r ** 2))
    nll = (a + 2.0) * math.log(b + 0.5 * sse)
    v = np.exp(np.linspace(math.log(1e-4), math.log(1e5), 400001))
    f = (2 * math.pi * v) ** -2.0 * np.exp(-0.5 * sse / v) * b ** a / math.gamma(a) * v ** (-a - 1) * np.exp(-b / v)
    integral = float(np.sum(0.5 * (f[1:] * v[1:] + f[:-1] * v[:-1]) * np.diff(np.log(v))))
    assert math.isclose(-(nll + om.log_norm()), math.log(integral), rel_tol=1e-8)


def test_new_symbols_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "hode.h")).read()
    declared = set(re.findall(r"\b(hode_obs_\w+)\s*\(", header))
    assert declared == {"hode_obs_nll_sets_f32", "hode_obs_nll_sets_f64"}
    assert declared <= set(hode.capi.SYMBOLS)
    for name, val in (("HODE_OBS_FIXED", hode.capi.OBS_FIXED), ("HODE_OBS_MARGINAL", hode.capi.OBS_MARGINAL),
                      ("HODE_OBS_SUMS_ONLY", hode.capi.OBS_SUMS_ONLY), ("HODE_OBS_FROM_SSE", hode.capi.OBS_FROM_SSE)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    lib = hode.load()
    assert all(hasattr(lib, s) for s in declared)


def test_abi_validates_before_any_launch():
    """Bad modes, flags and per-state values are refused on the host (no device is touched: the pointers are never read)."""
    import ctypes as C
    lib = hode.load()
    six = lambda *v: (C.c_double * 6)(*v)                                       # noqa: E731
    ok, bad = six(1, 1, 1, 1, 1, 1), six(1, 1, 0, 1, 1, 1)
    for sfx in ("f32", "f64"):
        f = getattr(lib, f"hode_obs_nll_sets_{sfx}")
        call = lambda n_sets, ln, mode, flags, w, a, b, n, y=1: f(None, C.c_int(n_sets), C.c_int64(ln), C.c_void_p(0), C.c_void_p(0), None,   # noqa: E731
                                                                  C.c_int(mode), C.c_int(flags), w, a, b, n, None, None, None)
        assert call(0, 10, 0, 0, ok, None, None, None) == 0                       # nothing to do
        assert call(2, 0, 1, 0, None, ok, ok, ok) == 0
        assert call(-1, 10, 0, 0, ok, None, None, None) == -1
        assert call(1, 10, 2, 0, ok, None, None, None) == -1                      # unknown mode
        assert call(1, 10, 0, 3, ok, None, None, None) == -1                      # unknown flags
        assert call(1, 10, 0, 0, None, ok, ok, ok) == -1                          # fixed mode needs w
        assert call(1, 10, 0, 0, bad, None, None, None) == -1                     # w must be positive
        assert call(1, 10, 1, 0, None, ok, bad, ok) == -1                         # b must be positive
        assert call(1, 10, 1, 0, None, ok, ok, None) == -1
        assert call(1, 10, 0, 0, ok, None, None, None) == -1                      # NULL y / obs / sse


def test_samplers_accept_the_new_arguments_up_to_the_device():
    from inference.hmc import run_hmc
    from inference.nuts import run_nuts
    from models.hybrid_ode_nn import HybridODENN
    m = HybridODENN(nn_hidden=16, nn_layers=2)
    for run, kw in ((run_hmc, dict(n_leapfrog=2)), (run_nuts, {})):
        for good in (dict(noise_sigma=[0.1, 1.0, 1.0, 0.2, 1e-4, 0.05]), dict(noise="marginal"),
                     dict(noise_sigma=torch.tensor([0.5] * 6), noise="marginal", noise_prior=(2.0, [1.0] * 6))):
            try:
                run(m, None, num_samples=1, num_warmup=0, n_chains=2, **good, **kw)
            except hode.capi.HodeError as e:                                    # past validation: only the device is missing
                assert "HIP device" in str(e) and not torch.cuda.is_available()
        for bad in (dict(noise_sigma=[1.0, 2.0]), dict(noise_sigma=-1.0), dict(noise="sampled"), dict(noise_prior=(2.0, 1.0)),
                    dict(noise="marginal", noise_prior=(0.0, 1.0))):
            with pytest.raises(ValueError):
                run(m, None, num_samples=1, num_warmup=0, n_chains=2, **bad, **kw)
