"""Multi-chain HMC on the GPU (inference/hmc.py, csrc/hode_hmc.hip): the per-set likelihood kernel, the momentum stream, one
leapfrog trajectory against a torch-fp64 restatement, the order of the energy error, the prior, a posterior against
quadrature, determinism, failed solves, and run_hmc end to end on the 4GI data path."""
import math

import numpy as np
import pytest
import torch

import hode

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(H=64, L=4, seed=0):
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(seed)
    return HybridODENN(nn_hidden=H, nn_layers=L, device=DEV)


def _data(model, B=4, T=13, sigma=0.05, seed=1, ode=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.tensor([8.0, 90.0, 80.0, 10.0, 0.0, 0.5], device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
    t = torch.linspace(0.0, 2.0, T, device=DEV)
    with torch.no_grad():
        y = model.forward_ode_sets({k: [v] for k, v in (ode or {"a_GI": 0.0104}).items()}, x0, t)[0]
    obs = y + sigma * torch.randn(y.shape, device=DEV, generator=g)
    return {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {}}


# ------------------------------------------------------------------ 1. per-set sum of squares
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_mse_sets_against_torch(dt):
    g = torch.Generator(device=DEV).manual_seed(0)
    S, n = 5, 1001
    buf = torch.randn(S * n + 1, dtype=dt, device=DEV, generator=g)
    y = buf[1:].view(S, n)                                          # unaligned: one element in
    obs = torch.randn(n + 3, dtype=dt, device=DEV, generator=g)[3:]
    ls = torch.zeros(S, dtype=torch.float64, device=DEV)
    gy = hode.capi.mse_sets(y, obs, 0.7, ls)
    d = (y - obs)                                                  # the kernel's residual, in the input precision
    want = (d.double() ** 2).sum(1)
    torch.testing.assert_close(ls, want, rtol=1e-13, atol=0)
    torch.testing.assert_close(gy, (2 * torch.tensor(0.7, dtype=dt)) * d, rtol=1e-6 if dt == torch.float32 else 1e-15, atol=0)
    ls2 = torch.zeros(S, dtype=torch.float64, device=DEV)
    gy2 = hode.capi.mse_sets(y, obs, 0.7, ls2)
    assert torch.equal(ls, ls2) and torch.equal(gy, gy2)
    # aligned 16-byte path, and one set in two pieces (accumulate semantics)
    ya, oa = torch.randn(S, 1024, dtype=dt, device=DEV, generator=g), torch.randn(1024, dtype=dt, device=DEV, generator=g)
    whole = torch.zeros(S, dtype=torch.float64, device=DEV)
    hode.capi.mse_sets(ya, oa, 1.0, whole)
    parts = torch.zeros(S, dtype=torch.float64, device=DEV)
    hode.capi.mse_sets(ya[:, :333].contiguous(), oa[:333], 1.0, parts)
    hode.capi.mse_sets(ya[:, 333:].contiguous(), oa[333:], 1.0, parts)
    assert float(((parts - whole).abs() / whole).max()) < 1e-15
    torch.testing.assert_close(whole, ((ya - oa).double() ** 2).sum(1), rtol=1e-13, atol=0)


# ------------------------------------------------------------------ 2. momentum
def _refresh(C, D, seed=7, it=3):
    f64 = dict(dtype=torch.float64, device=DEV)
    ld = D
    z = torch.zeros(C, ld, dtype=torch.float32, device=DEV)
    p = torch.empty_like(z)
    ke0 = torch.empty(C, **f64)
    hode.capi.hmc_refresh(C, D, ld, seed, it, 0.0, torch.ones(ld, dtype=torch.float32, device=DEV), torch.zeros(C, **f64), z, z.clone(),
                          torch.zeros(C, **f64), p, torch.empty_like(z), torch.empty_like(z), torch.empty(C, **f64), ke0,
                          torch.empty(C, **f64), torch.empty(C, dtype=torch.int32, device=DEV))
    return p, ke0


def test_momentum_stream_is_per_chain_and_standard_normal():
    D = 131075
    p4, k4 = _refresh(4, D)
    p8, k8 = _refresh(8, D)
    assert torch.equal(p8[:4], p4) and torch.equal(k8[:4], k4)
    p8b, _ = _refresh(8, D)
    assert torch.equal(p8, p8b)
    x = p8.double().reshape(-1)
    n = x.numel()
    assert n >= 10 ** 6
    assert abs(float(x.mean())) < 5 / math.sqrt(n)
    assert abs(float(x.var()) - 1) < 5 * math.sqrt(2 / n)
    torch.testing.assert_close(k8, 0.5 * (p8.double() ** 2).sum(1), rtol=1e-12, atol=0)
    p_other, _ = _refresh(8, D, it=4)
    assert not torch.equal(p_other, p8)


# ------------------------------------------------------------------ 3./4. leapfrog against torch fp64
def _small_sampler(C=3, jitter=0.0, sample_nn=True, sigma=0.2):
    from inference.hmc import _Sampler
    m = _model(16, 2)
    data = _data(m, B=2, T=5, sigma=sigma)
    s = _Sampler(m, data, C, noise_sigma=sigma, seed=11, solver="rk4", dtype=torch.float64, jitter=jitter, sample_nn=sample_nn)
    s.initial_jitter()
    s.gradient()
    return s


def _torch_U_grad(s, z):
    """U and grad U by the existing fp64 solve / adjoint, with plain torch arithmetic around them."""
    from models.ode_core import ODE_PARAM_NAMES
    C, P = s.C, s.P
    zd = z[:, :s.D].double()
    ode = s.ode_base.double().reshape(1, 17).repeat(C, 1)
    idx = [ODE_PARAM_NAMES.index(n) for n in s.ode_names]
    ode[:, idx] = s.mu + s.sd * zd[:, :s.n_ode]
    nn = zd[:, s.n_ode:]
    N = s.N
    sol = hode.solve_fwd(s.x0.repeat(C, 1), s.t.repeat(C, 1) if s.t.dim() == 2 else s.t, None, None, None, ode.reshape(-1),
                         nn.reshape(-1), s.H, s.L, method=hode.METHOD_RK4, n_sets=C, want_tape=True)
    r = sol.y.view(C, N, -1) - s.obs.view(1, N, -1)
    ss = (r ** 2).sum((1, 2))
    _, gnn, gode = hode.solve_bwd(sol, (2 * s.lik_scale * r).view_as(sol.y), want_gnn=True, want_gode=True)
    grad = torch.cat([gode.view(C, 17)[:, idx] * s.sd, gnn.view(C, P)], 1) + zd
    return s.lik_scale * ss + 0.5 * (zd ** 2).sum(1), grad


def test_one_trajectory_matches_torch_fp64_and_is_reversible():
    s = _small_sampler()
    s.log_eps.fill_(math.log(0.02))
    s.refresh(5)
    z0, p0 = s.z.clone(), s.p.clone()
    U0, g0 = _torch_U_grad(s, z0)
    torch.testing.assert_close(s.U, U0, rtol=1e-12, atol=0)
    torch.testing.assert_close(s.g[:, :s.D], g0, rtol=1e-12, atol=1e-12)
    L = 4
    s.trajectory(L)
    # restatement: the same xi (read back from the refresh kernel: p0, minv = 1), the same eps
    e = s.eps.view(-1, 1)
    z, p, g = z0[:, :s.D].clone(), p0[:, :s.D].clone(), g0
    p = p - 0.5 * e * g
    for i in range(L):
        z = z + e * p
        U, g = _torch_U_grad(s, z)
        p = p - (0.5 if i == L - 1 else 1.0) * e * g
    H1 = U + 0.5 * (p ** 2).sum(1)
    torch.testing.assert_close(s.z[:, :s.D], z, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(s.p[:, :s.D], p, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(s.U + s.ke, H1, rtol=1e-12, atol=0)
    # reversibility: flip p, L steps back
    s.p.neg_()
    s.trajectory(L)
    assert float((s.z - z0).abs().max()) < 1e-10


def test_energy_error_is_second_order():
    s = _small_sampler(sample_nn=False, sigma=1.0)          # the seven constants: a smooth, well-conditioned U
    z_start = s.z.clone()

    def dH(eps, L):
        s.z.copy_(z_start)
        s.gradient()
        s.log_eps.fill_(math.log(eps))
        s.refresh(9)
        H0 = s.U + s.ke0
        s.trajectory(L)
        return (s.U + s.ke - H0).abs()

    eps, T = 0.4, 1.6
    while True:
        d1 = dH(eps, round(T / eps))
        if bool(torch.isfinite(d1).all()) and float(d1.max()) < 0.5:
            break
        eps /= 2
        assert eps > 1e-4
    eps /= 2                                                        # one halving deeper into the asymptotic regime
    d1 = dH(eps, round(T / eps))
    d2 = dH(eps / 2, 2 * round(T / eps))
    assert float(d2.min()) > 1e-9, d2                              # well above rounding
    ratio = d1 / d2
    assert bool(((ratio > 3) & (ratio < 5.5)).all()), (eps, ratio)


# ------------------------------------------------------------------ 5. prior only
def test_prior_only_run_recovers_the_prior():
    from inference.hmc import REFERENCE_PRIORS, run_hmc
    m = _model()
    # L = 8: with eps adapted to 0.8 in 13 517 dimensions (~0.2), L = 16 is half a period of the unit Gaussian -- nearly
    # antithetic draws, whose ESS (and so the MCSE) the Geyer estimate gets only roughly
    r = run_hmc(m, None, num_samples=300, num_warmup=200, n_chains=64, n_leapfrog=8, seed=3)
    x = r.draws.double()                                           # [64, 300, D] natural coordinates
    mu = torch.zeros(x.shape[2], dtype=torch.float64, device=x.device)
    sd = torch.ones_like(mu)
    for i, n in enumerate(r.ode_names):
        mu[i], sd[i] = REFERENCE_PRIORS[n]
    flat = x.reshape(-1, x.shape[2])
    mean, psd = flat.mean(0), flat.std(0)
    mcse = psd / r.ess(kind="mean").sqrt()
    assert float(((mean - mu).abs() / mcse).max()) < 5
    assert float((psd / sd - 1).abs().max()) < 0.10
    acc = float(np.mean(r.stats["accept_prob"]))
    assert abs(acc - 0.8) < 0.1, acc
    assert int(r.stats["divergent"].sum()) == 0


# ------------------------------------------------------------------ 6. posterior against quadrature
def test_posterior_matches_quadrature():
    from inference.hmc import run_hmc
    m = _model()
    sig = 0.05
    data = _data(m, B=4, T=13, sigma=sig, seed=2, ode={"a_GI": 0.0110, "k_I": 0.022})
    pri = {"a_GI": (0.0104, 0.002), "k_I": (0.025, 0.005)}
    x0, t, obs = data["initial_state"], data["time_points"], data["observations"].double()

    def logpost(a, k):
        y = m.forward_ode_sets({"a_GI": a, "k_I": k}, x0, t).double()
        ss = ((y - obs) ** 2).sum((1, 2, 3))
        za, zk = (a.double() - pri["a_GI"][0]) / pri["a_GI"][1], (k.double() - pri["k_I"][0]) / pri["k_I"][1]
        return -ss / (2 * sig ** 2) - 0.5 * (za ** 2 + zk ** 2)

    def moments(ca, wa, ck, wk, n):
        ga = torch.linspace(ca - wa, ca + wa, n, dtype=torch.float64, device=DEV)
        gk = torch.linspace(ck - wk, ck + wk, n, dtype=torch.float64, device=DEV)
        A, K = torch.meshgrid(ga, gk, indexing="ij")
        lp = logpost(A.reshape(-1).float(), K.reshape(-1).float())
        w = torch.exp(lp - lp.max())
        w = w / w.sum()
        a, k = A.reshape(-1), K.reshape(-1)
        ma, mk = float((w * a).sum()), float((w * k).sum())
        return ma, mk, float((w * (a - ma) ** 2).sum().sqrt()), float((w * (k - mk) ** 2).sum().sqrt())

    ma, mk, sa, sk = moments(pri["a_GI"][0], 5 * pri["a_GI"][1], pri["k_I"][0], 5 * pri["k_I"][1], 128)
    ma, mk, sa, sk = moments(ma, 6 * sa, mk, 6 * sk, 128)
    ma, mk, sa, sk = moments(ma, 6 * sa, mk, 6 * sk, 160)
    r = run_hmc(m, data, num_samples=200, num_warmup=150, n_chains=256, n_leapfrog=8, noise_sigma=sig, ode_priors=pri,
                sample_nn=False, seed=5)
    x = r.draws.double().reshape(-1, 2)
    mcse = x.std(0) / r.ess(kind="mean").sqrt()
    got_m, got_s = x.mean(0), x.std(0)
    assert abs(float(got_m[0]) - ma) < 4 * float(mcse[0]) and abs(float(got_m[1]) - mk) < 4 * float(mcse[1]), (got_m, ma, mk, mcse)
    assert abs(float(got_s[0]) / sa - 1) < 0.1 and abs(float(got_s[1]) / sk - 1) < 0.1, (got_s, sa, sk)


# ------------------------------------------------------------------ 7. determinism
def test_same_seed_same_draws():
    from inference.hmc import run_hmc
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    kw = dict(num_samples=10, num_warmup=20, n_chains=32, n_leapfrog=4, noise_sigma=0.5, seed=9)
    a, b = run_hmc(m, data, **kw), run_hmc(m, data, **kw)
    assert torch.equal(a.draws, b.draws)
    for k in ("accept_prob", "log_posterior", "divergent", "failed_solve", "step_size", "inv_mass"):
        assert np.array_equal(a.stats[k], b.stats[k]), k


# ------------------------------------------------------------------ 8. failed solves
def test_failed_solves_are_rejected_and_counted():
    from inference.hmc import run_hmc
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    # K_m ~ N(7, 20^2) reaches K_m + G ~ 0: the GLP-1 production term blows up, the solve reports status 2 / 3
    kw = dict(num_samples=40, num_warmup=0, n_leapfrog=4, noise_sigma=0.5, ode_priors={"K_m": (7.0, 20.0), "k_L": (0.02, 0.005)},
              sample_nn=False, seed=1)
    r = run_hmc(m, data, n_chains=16, **kw)
    st = r.stats
    assert int(st["failed_solve"].sum()) > 0
    assert bool(st["divergent"][st["failed_solve"]].all()) and float(np.abs(st["accept_prob"][st["failed_solve"]]).max()) == 0.0
    assert bool(torch.isfinite(r.draws).all()) and np.isfinite(st["log_posterior"]).all()
    # chains are independent: the first 8 of 16 chains are those of an 8-chain run, failures or not
    r8 = run_hmc(m, data, n_chains=8, **kw)
    torch.testing.assert_close(r8.draws, r.draws[:8], rtol=1e-5, atol=1e-6)
    assert np.array_equal(r8.stats["failed_solve"], st["failed_solve"][:8])


# ------------------------------------------------------------------ 9. end to end on the 4GI batch
def test_run_hmc_end_to_end_on_4gi_batch():
    from hode.datagen import FourGIModel, GlucoseDataset
    from inference.hmc import run_hmc
    gen = torch.Generator(device=DEV).manual_seed(0)
    table, status = FourGIModel("T2DM").generate_cohort(32, duration_hours=5, sampling_interval_min=5, meal_times=(0.5, 2.5),
                                                        meal_sizes=(75, 50), noise_cv=0.1, generator=gen)
    ds = GlucoseDataset(table, sequence_length=61, stride=61)
    batch = ds.batch(torch.arange(32))
    assert tuple(batch["observations"].shape) == (32, 61, 6)
    m = _model()
    r = run_hmc(m, batch, num_samples=4, num_warmup=4, n_chains=8, n_leapfrog=2, seed=2)
    s = r.samples
    names = [n for n, _ in m.nn_residual.named_parameters()]
    assert list(s) == [f"ode.{k}" for k in ("a_GI", "k_I", "rho", "E_max", "V_max", "K_m", "k_L")] + [f"nn.{n}" for n in names]
    for n, p in m.nn_residual.named_parameters():
        assert s[f"nn.{n}"].shape == (8, 4) + tuple(p.shape)
    assert r.flat()["ode.k_L"].shape == (32,)
    assert r.stats["accept_prob"].shape == (8, 4) and r.stats["step_size"].shape == (8,)
    pred = r.predict(batch["initial_state"], batch["time_points"], batch["external_inputs"])
    assert tuple(pred.shape) == (32, 32, 61, 6)
    flat = r.flat()
    sets = []
    for i in range(32):
        d = {f"ode_{k[4:]}": torch.tensor(v[i]) for k, v in flat.items() if k.startswith("ode.")}
        d.update({f"nn_{k[3:].replace('.', '_')}": torch.as_tensor(v[i]) for k, v in flat.items() if k.startswith("nn.")})
        sets.append(d)
    want = m.forward_param_sets(sets, batch["initial_state"], batch["time_points"], batch["external_inputs"])
    torch.testing.assert_close(pred, want, rtol=1e-6, atol=1e-6)
