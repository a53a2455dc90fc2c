"""Every route through the one driver (inference.hmc._run_schedule): {run_hmc, run_nuts} x {the plain target, latent initial
states, the population, the population with latent initial states in front}.  Each route runs twice from one seed at the
smallest shapes that still use every buffer -- num_warmup = 20 is the first count at which Stan's schedule opens a slow window,
so the Welford passes and a second step-size search run -- and must give the same draws and stats, bit for bit, the result
type of the route and its draw width D."""
import numpy as np
import pytest
import torch

import hode

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, T, C, WARM, N = 3, 5, 4, 20, 3
X0_TYPICAL = [8.0, 90.0, 80.0, 10.0, 0.0, 0.5]
MEAN = [8.0, 90.0, 80.0, 10.0, 0.5, 0.5]
STATES = ("G", "I", "GLP1")


@pytest.fixture(scope="module")
def case():
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN(nn_hidden=16, nn_layers=2, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    x0 = torch.tensor(X0_TYPICAL, device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
    t = torch.linspace(0.0, 2.0, T, device=DEV)
    with torch.no_grad():
        y = m.forward_ode_sets({"a_GI": torch.tensor([0.0104])}, x0, t)[0]
    obs = y + 0.2 * torch.randn(y.shape, device=DEV, generator=g)
    return m, {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {}}


def _run(kind, route, m, data):
    from inference import InitialStatePrior, run_population
    from inference.hmc import run_hmc
    from inference.nuts import run_nuts
    kw = dict(num_samples=N, num_warmup=WARM, n_chains=C, noise_sigma=0.2, seed=5, solver="rk4", dtype=torch.float64)
    kw.update(dict(n_leapfrog=2) if kind == "hmc" else dict(max_tree_depth=3))
    if "latent" in route:
        mean = np.array(MEAN)
        kw["initial_state"] = InitialStatePrior(mean, 0.1 * mean + 0.01, states=STATES)
    if route.startswith("population"):
        return run_population(m, data, sampler=kind, **kw)
    return (run_hmc if kind == "hmc" else run_nuts)(m, data, sample_nn=route == "plain", **kw)


@pytest.mark.parametrize("route", ["plain", "latent", "population", "population+latent"])
@pytest.mark.parametrize("kind", ["hmc", "nuts"])
def test_same_seed_same_draws_on_every_route(case, kind, route):
    from inference import LatentStateResult, PopulationResult
    from inference.hmc import HMCResult
    m, data = case
    a, b = _run(kind, route, m, data), _run(kind, route, m, data)
    raw = (lambda r: r.raw) if route == "latent" else (lambda r: r.draws)          # the chain coordinates as the driver left them
    assert torch.equal(raw(a), raw(b)) and torch.equal(a.draws, b.draws)
    assert set(a.stats) == set(b.stats)
    for k, v in a.stats.items():
        assert np.array_equal(v, b.stats[k], equal_nan=True), k
    n_w = B * len(STATES)
    cls, D = {"plain": (HMCResult, 7 + hode.n_params(16, 2)), "latent": (LatentStateResult, 7 + n_w),
              "population": (PopulationResult, 7 * (B + 2)), "population+latent": (PopulationResult, 7 * (B + 2) + n_w)}[route]
    assert type(a) is cls and tuple(raw(a).shape) == (C, N, D)
    assert tuple(a.stats["inv_mass"].shape) == (D,) and tuple(a.stats["step_size"].shape) == (C,)
    if kind == "nuts":
        assert tuple(a.stats["trajectories_solved"].shape) == (WARM + N,)
    else:
        assert "trajectories_solved" not in a.stats
