"""GPU tests of inference.fit_patients: per-patient Levenberg-Marquardt on synthetic patients whose constants are drawn from the
reference's priors (recovery without noise, the MAP and its Laplace uncertainty with noise, sparse records, failures, and
the independence of patients)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("a_GI", "k_I", "rho", "E_max", "V_max", "K_m", "k_L")
KW = dict(rtol=1e-10, atol=1e-12, max_steps=1500)


@pytest.fixture(scope="module")
def M():
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN()
    with torch.no_grad():                               # a small residual: the mechanistic model carries the dynamics
        for p in m.nn_residual.parameters():
            p.mul_(0.05)
    return m


def cohort(M, B=256, T=61, sigma=0.0, seed=0):
    """Patients with constants drawn from REFERENCE_PRIORS (within 2 sd), their exact (noise-free) or noisy records on a 0..240
    grid.  Draws whose own solve fails (G reaching the pole -K_m) are replaced by further draws."""
    from inference.hmc import REFERENCE_PRIORS
    rng = np.random.default_rng(seed)
    n0 = B + B // 4 + 4
    truth = {n: REFERENCE_PRIORS[n][0] + REFERENCE_PRIORS[n][1] * np.clip(rng.standard_normal(n0), -2, 2) for n in NAMES}
    x0 = np.array([5.0, 60.0, 80.0, 10.0, 0.0, 1.0]) * (1 + 0.1 * rng.standard_normal((n0, 6)))
    t = np.linspace(0.0, 240.0, T)
    meal = np.zeros((n0, T))
    for b in range(n0):
        k = rng.integers(2, 12)
        meal[b, k:k + 4] = rng.uniform(0.02, 0.08)
    batch = {"initial_state": torch.tensor(x0), "time_points": torch.tensor(t), "external_inputs": {"meal": torch.tensor(meal)}}
    y, _ = M.sensitivities(batch["initial_state"], batch["time_points"], batch["external_inputs"], wrt=("a_GI",),
                           ode_sets={n: torch.tensor(v) for n, v in truth.items()}, dtype=torch.float64, **KW)
    keep = torch.nonzero(M.last_solve_info["status"].cpu() == 0).flatten()[:B]
    assert keep.numel() == B
    obs = y.double().cpu()[keep] + sigma * torch.tensor(rng.standard_normal((B,) + tuple(y.shape[1:])))
    batch = {"initial_state": batch["initial_state"][keep], "time_points": batch["time_points"], "observations": obs,
             "external_inputs": {"meal": batch["external_inputs"]["meal"][keep]}}
    return batch, {n: v[keep.numpy()] for n, v in truth.items()}


def test_noise_free_patients_recover_their_constants(M):
    from inference import fit_patients
    batch, truth = cohort(M)
    res = fit_patients(M, batch, params=NAMES, priors=None, noise_sigma=0.1, max_iter=100, **KW)
    ev = res.fim_eigvals.cpu().numpy()
    cond = ev[:, -1] / np.maximum(ev[:, 0], ev[:, -1] * 1e-30)
    st = res.status.cpu().numpy()
    good = np.isfinite(cond) & (cond < 1e8)
    assert good.mean() > 0.5, np.median(cond)
    # a well-conditioned patient converges (a few stall in a valley of the least-squares surface within max_iter: status 1) ...
    assert (st[good] == 0).mean() >= 0.95, np.bincount(st[good])
    # ... and every converged one recovers its truth
    for n in NAMES:
        est, tr = res.params[n].cpu().numpy(), truth[n]
        rel = np.abs(est - tr) / np.abs(tr)
        assert rel[good & (st == 0)].max() < 1e-6, (n, rel[good & (st == 0)].max())


def test_noisy_map_gradient_and_laplace_coverage(M):
    import hode
    from inference import fit_patients
    from inference.hmc import REFERENCE_PRIORS
    sigma = 0.05
    batch, truth = cohort(M, B=128, sigma=sigma, seed=3)
    res = fit_patients(M, batch, params=NAMES, priors=REFERENCE_PRIORS, noise_sigma=sigma, max_iter=100, **KW)
    st = res.status.cpu().numpy()
    assert (st == 0).mean() > 0.95, np.bincount(st)
    mu = torch.tensor([REFERENCE_PRIORS[n][0] for n in NAMES], dtype=torch.float64, device="cuda")
    sd = torch.tensor([REFERENCE_PRIORS[n][1] for n in NAMES], dtype=torch.float64, device="cuda")
    idx = [0, 1, 2, 5, 8, 9, 10]
    obs = batch["observations"].to("cuda")

    def grad_z(theta):
        """d F / d z through the existing adjoint: F = 1/2 |(y - obs) / sigma|^2 + 1/2 |z|^2, z = (theta - mu) / sd."""
        nn_flat, ode_vec = M._params_on(torch.device("cuda"))
        B = theta.shape[0]
        ode = ode_vec.double().repeat(B, 1)
        ode[:, idx] = theta
        f = lambda v: v.to("cuda").float().double()              # noqa: E731  (the fit reads its inputs through fp32)
        sol = hode.solve_fwd(f(batch["initial_state"]), f(batch["time_points"]), f(batch["external_inputs"]["meal"]),
                             None, None, ode.reshape(-1).contiguous(), nn_flat.detach().double().repeat(B).contiguous(), 64, 4, n_sets=B,
                             want_tape=True, **KW)
        _, _, gode = hode.solve_bwd(sol, (sol.y - obs) / sigma ** 2, want_gnn=False, want_gode=True)
        z = (theta - mu) / sd
        return gode.view(B, 17)[:, idx] * sd + z
    theta_hat = torch.stack([res.params[n] for n in NAMES], 1)
    theta0 = mu.expand_as(theta_hat)                          # the model's constants = the prior means
    g0, g1 = grad_z(theta0).norm(dim=1), grad_z(theta_hat).norm(dim=1)
    ok = torch.tensor(st == 0, device="cuda")
    assert bool((g1[ok] <= 1e-6 * g0[ok]).all()), float((g1 / g0)[ok].max())
    tr = np.stack([truth[n] for n in NAMES], 1)
    inside = np.abs(theta_hat.cpu().numpy() - tr) <= 2 * res.std.cpu().numpy()
    assert inside[st == 0].mean() >= 0.85, inside.mean()
    assert torch.allclose(torch.diagonal(res.corr, dim1=1, dim2=2), torch.ones(1, dtype=torch.float64, device="cuda"))


def test_glucose_only_records_failures_and_patient_independence(M):
    from inference import fit_patients
    from inference.hmc import REFERENCE_PRIORS
    batch, truth = cohort(M, B=12, sigma=0.05, seed=5)
    obs = batch["observations"].clone()
    obs[:, :, 1:] = float("nan")                             # glucose only
    obs[:, 1::3, 0] = float("nan")                           # sparse
    obs[4] = float("nan")                                    # no data at all: the prior
    x0 = batch["initial_state"].clone()
    x0[7, 2] = float("nan")                                  # this patient's solve fails
    b2 = dict(batch, observations=obs, initial_state=x0)
    res = fit_patients(M, b2, params=NAMES, noise_sigma=0.05, max_iter=50, **KW)
    st = res.status.cpu().numpy()
    assert st[7] == 2 and (st[np.arange(12) != 7] != 2).all(), st
    for n in NAMES:
        assert abs(float(res.params[n][4]) - REFERENCE_PRIORS[n][0]) <= 1e-12 * REFERENCE_PRIORS[n][0]
        assert abs(float(res.std[4, NAMES.index(n)]) - REFERENCE_PRIORS[n][1]) <= 1e-9 * REFERENCE_PRIORS[n][1]
    assert bool(torch.isfinite(res.objective[np.arange(12) != 7]).all())
    keep = [b for b in range(12) if b != 7]
    sub = {"initial_state": x0[keep], "time_points": batch["time_points"], "observations": obs[keep],
           "external_inputs": {"meal": batch["external_inputs"]["meal"][keep]}}
    res2 = fit_patients(M, sub, params=NAMES, noise_sigma=0.05, max_iter=50, **KW)
    for n in NAMES:
        a, b = res.params[n][keep].cpu().numpy(), res2.params[n].cpu().numpy()
        assert np.allclose(a, b, rtol=1e-8, atol=0), n
    one = {"initial_state": x0[[2]], "time_points": batch["time_points"], "observations": obs[[2]],
           "external_inputs": {"meal": batch["external_inputs"]["meal"][[2]]}}
    res1 = fit_patients(M, one, params=NAMES, noise_sigma=0.05, max_iter=50, **KW)
    for n in NAMES:
        assert abs(float(res1.params[n][0]) - float(res.params[n][2])) <= 1e-8 * abs(float(res1.params[n][0])), n
    y = res.predict()
    assert y.shape == (12, 61, 6) and bool(torch.isfinite(y[keep]).all())
