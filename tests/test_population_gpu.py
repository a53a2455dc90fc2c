"""The hierarchical population posterior on the GPU (inference/population.py, csrc/hode_population.hip): the two kernels against
the numpy restatement (tests/_population_reference.py), the transpose on the device, U and grad U end to end against a torch
restatement, per-patient parameter sets through models.hybrid_ode_nn._run_sets against the oracle, the prior, a posterior with
real coupling between two patients against quadrature, and the properties of a run."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _population_reference as PR
import hode

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NCPU = max(1, min(os.cpu_count() or 1, 16))


def _model(H=64, L=4, seed=0):
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(seed)
    return HybridODENN(nn_hidden=H, nn_layers=L, device=DEV)


def _data(model, B=4, T=13, sigma=0.05, seed=1, ode=None):
    """A batch of B patients on a grid of T points; ode: name -> one true value per patient (default: the model's constants)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.tensor([8.0, 90.0, 80.0, 10.0, 0.0, 0.5], device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
    t = torch.linspace(0.0, 2.0, T, device=DEV)
    sets = {k: torch.as_tensor(v, dtype=torch.float32).reshape(-1).expand(B) for k, v in (ode or {"a_GI": [0.0104]}).items()}
    with torch.no_grad():
        y = model.forward_ode_sets(sets, x0, t)                       # [B sets, B patients, T, 6]: patient b with set b
    y = y[torch.arange(B), torch.arange(B)]
    obs = y + sigma * torch.randn(y.shape, device=DEV, generator=g)
    return {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {}}


def _hyper_values(K, rng):
    mu0 = rng.uniform(0.01, 10.0, K)
    return mu0, 0.2 * mu0, 0.15 * mu0


# ------------------------------------------------------------------ 1. the kernels against the restatement
SHAPES = [(1, 1, 1), (3, 3, 7), (2, 257, 7), (2, 5, 17)]


def _kernel_case(A, B, K, dt, aligned, seed=0):
    rng = np.random.default_rng(seed + 1000 * A + 10 * B + K)
    D = K * (B + 2)
    ld = (D + 3) // 4 * 4 if aligned else D
    idx = sorted(int(j) for j in rng.choice(17, K, replace=False))
    mask = sum(1 << j for j in idx)
    mu0, sd0, tau0 = _hyper_values(K, rng)
    f64 = dict(dtype=torch.float64, device=DEV)
    c = dict(A=A, B=B, K=K, D=D, ld=ld, idx=idx, mask=mask, omega=0.5, mu0=mu0, sd0=sd0, tau0=tau0,
             mu0_d=torch.tensor(mu0, **f64), sd0_d=torch.tensor(sd0, **f64), tau0_d=torch.tensor(tau0, **f64))
    c["coords"] = torch.as_tensor(rng.standard_normal((A, ld)), dtype=dt, device=DEV)        # the pad holds values, too: never read
    c["gode"] = torch.as_tensor(rng.standard_normal((A * B, 17)), dtype=dt, device=DEV)
    c["base"] = torch.as_tensor(rng.uniform(0.5, 2.0, 17), dtype=dt, device=DEV)
    if aligned:
        assert ld % 4 == 0 and c["coords"].data_ptr() % 16 == 0
    return c


def _params(c, coords=None, A=None):
    coords = c["coords"] if coords is None else coords
    A = c["A"] if A is None else A
    out = torch.full((A * c["B"], 17), float("nan"), dtype=coords.dtype, device=DEV)
    hode.capi.pop_params(A, c["B"], c["K"], c["ld"], coords, c["mask"], c["mu0_d"], c["sd0_d"], c["tau0_d"], c["omega"], c["base"], out)
    return out


def _grad(c, coords=None, gode=None, A=None):
    coords = c["coords"] if coords is None else coords
    gode = c["gode"] if gode is None else gode
    A = c["A"] if A is None else A
    out = torch.full((A, c["ld"]), float("nan"), dtype=coords.dtype, device=DEV)
    hode.capi.pop_grad(A, c["B"], c["K"], c["ld"], coords, gode, c["mask"], c["sd0_d"], c["tau0_d"], c["omega"], out)
    return out


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("A,B,K", SHAPES)
def test_pop_params_against_the_restatement(A, B, K, aligned, dt):
    """fp64: 1e-15 relative; fp32: one rounding (2^-23) of the fp64 value computed from the same fp32 inputs; entries that are
    not sampled equal ode_base exactly.  "Relative" is to |mu_pop| + |tau z|, the magnitudes of the two terms of theta: the
    device's exp and numpy's differ by an ulp, which is that much of tau z whatever the sum cancels to."""
    c = _kernel_case(A, B, K, dt, aligned)
    got = _params(c).view(A, B, 17).double().cpu().numpy()
    cn = c["coords"].double().cpu().numpy()
    base = c["base"].double().cpu().numpy()
    want = PR.pop_params(cn, K, B, c["idx"], c["mu0"], c["sd0"], c["tau0"], c["omega"], base)
    mu, tau = PR.hyper(cn, K, B, c["mu0"], c["sd0"], c["tau0"], c["omega"])
    mag = np.abs(mu)[:, None, :] + np.abs(tau[:, None, :] * PR.split(cn, K, B)[2])
    err = np.abs(got - want)[..., c["idx"]]
    bound = 1e-15 * mag + (2.0 ** -23 * np.abs(want[..., c["idx"]]) if dt == torch.float32 else 0.0)
    print(f"\npop_params {(A, B, K)} {dt} aligned={aligned}: worst err / bound {float((err / bound).max()):.3f}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    rest = [j for j in range(17) if j not in c["idx"]]
    assert np.array_equal(got[..., rest], np.broadcast_to(base[rest], (A, B, len(rest))))
    assert torch.equal(_params(c), _params(c))


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("A,B,K", SHAPES)
def test_pop_grad_against_the_restatement(A, B, K, aligned, dt):
    """Every entry of g_m, g_s, g_z to 4 eps x (the sum of the absolute values of its terms), eps = 2^-52 / 2^-23: double
    accumulation and one output rounding, with a fourfold margin.  Pad entries are 0, a second call gives the same bits, and a
    row computed alone has the bits of the same row among others and at another row index."""
    c = _kernel_case(A, B, K, dt, aligned)
    D, ld = c["D"], c["ld"]
    got = _grad(c)
    cn = c["coords"].double().cpu().numpy()
    G = c["gode"].double().cpu().numpy().reshape(A, B, 17)[..., c["idx"]]
    want, mag = PR.pop_transpose(cn, G, K, B, c["sd0"], c["tau0"], c["omega"])
    eps = 2.0 ** -52 if dt == torch.float64 else 2.0 ** -23
    err = np.abs(got[:, :D].double().cpu().numpy() - want)
    print(f"\npop_grad {(A, B, K)} {dt} aligned={aligned}: worst err / (eps * sum|terms|) {float((err / (eps * mag)).max()):.3f}")
    assert np.all(err <= 4 * eps * mag)
    assert ld == D or bool((got[:, D:] == 0).all())
    assert torch.equal(got, _grad(c))
    for r in range(A):                                           # the row alone
        alone = _grad(c, c["coords"][r:r + 1].clone(), c["gode"].view(A, B, 17)[r].clone(), A=1)
        assert torch.equal(alone[0], got[r])
    if A > 1:                                                    # ... and at another row index
        rev = _grad(c, c["coords"].flip(0).contiguous(), c["gode"].view(A, B, 17).flip(0).contiguous())
        assert torch.equal(rev.flip(0), got)


# ------------------------------------------------------------------ 2. the transpose on the device
@pytest.mark.parametrize("A,B,K", SHAPES)
def test_pop_grad_is_the_transpose_of_pop_params(A, B, K):
    """fp64: <J v, G> from central differences of hode_pop_params along v against <v, hode_pop_grad(G)>, relative to the summed
    magnitudes of the terms; the bound of the host check (h = 1e-6: O(h^2) truncation 1e-13, rounding eps |theta| / h / sd0 =
    1.1e-9 per term): 5e-9."""
    c = _kernel_case(A, B, K, torch.float64, False, seed=3)
    rng = np.random.default_rng(17)
    h = 1e-6
    v = torch.as_tensor(rng.standard_normal((A, c["ld"])), dtype=torch.float64, device=DEV)
    Jv = (_params(c, c["coords"] + h * v) - _params(c, c["coords"] - h * v)) / (2 * h)
    lhs = (Jv * c["gode"])[:, c["idx"]].view(A, -1).sum(1)
    g = _grad(c)[:, :c["D"]]
    rhs = (v[:, :c["D"]] * g).sum(1)
    cn = c["coords"].cpu().numpy()
    G = c["gode"].cpu().numpy().reshape(A, B, 17)[..., c["idx"]]
    _, mag = PR.pop_transpose(cn, G, K, B, c["sd0"], c["tau0"], c["omega"])
    scale = (np.abs(v[:, :c["D"]].cpu().numpy()) * mag).sum(1)
    err = (lhs - rhs).abs().cpu().numpy()
    print(f"\ntranspose {(A, B, K)}: worst err / scale {float((err / scale).max()):.2e}")
    assert np.all(err <= 5e-9 * scale)


# ------------------------------------------------------------------ 3. U and grad U end to end
def _small_sampler(C=3, **kw):
    from inference.hmc import _Sampler
    from inference.population import _PopulationTarget
    m = _model(16, 2)
    data = _data(m, B=3, T=5, sigma=0.2, ode={"a_GI": [0.0095, 0.0104, 0.0115]})
    s = _Sampler(m, data, C, noise_sigma=0.2, seed=11, solver="rk4", dtype=torch.float64, jitter=0.0, target=_PopulationTarget(data, **kw))
    s.initial_jitter()
    s.gradient()
    return s


def _torch_U_grad(s, z):
    """U and grad U by ONE fp64 solve with n_sets = C B, the residuals, the adjoint, and the map and its transpose in torch."""
    from models.ode_core import ODE_PARAM_NAMES
    t = s.target
    C, B, K, w = s.C, t.B, t.K, t.omega
    zd = z[:, :s.D].double()
    m_, s_, zz = zd[:, :K], zd[:, K:2 * K], zd[:, 2 * K:].reshape(C, B, K)
    mu, tau = t.mu0 + t.sd0 * m_, t.tau0 * torch.exp(w * s_)
    theta = mu.unsqueeze(1) + tau.unsqueeze(1) * zz
    idx = [ODE_PARAM_NAMES.index(n) for n in t.pop_names]
    ode = s.ode_base.double().reshape(1, 17).repeat(C * B, 1)
    ode[:, idx] = theta.reshape(C * B, K)
    sol = hode.solve_fwd(s.x0.repeat(C, 1), s.t, None, None, None, ode.reshape(-1), s.nn_base.double().repeat(C * B), s.H, s.L,
                         method=hode.METHOD_RK4, n_sets=C * B, want_tape=True)
    r = sol.y.view(C, B, -1) - s.obs.view(1, B, -1)
    ss = (r ** 2).sum((1, 2))
    _, _, gode = hode.solve_bwd(sol, (2 * s.lik_scale * r).view_as(sol.y), want_gnn=False, want_gode=True)
    G = gode.view(C, B, 17)[:, :, idx]
    grad = torch.cat([t.sd0 * G.sum(1), w * tau * (G * zz).sum(1), (tau.unsqueeze(1) * G).reshape(C, B * K)], 1) + zd
    return s.lik_scale * ss + 0.5 * (zd ** 2).sum(1), grad


def test_one_trajectory_matches_torch_fp64_and_is_reversible():
    s = _small_sampler()
    assert s.D == 7 * 5 and s.ld == 36 and s.target.K == 7
    s.log_eps.fill_(math.log(0.02))
    s.refresh(5)
    z0, p0 = s.z.clone(), s.p.clone()
    U0, g0 = _torch_U_grad(s, z0)
    torch.testing.assert_close(s.U, U0, rtol=1e-12, atol=0)
    torch.testing.assert_close(s.g[:, :s.D], g0, rtol=1e-12, atol=1e-12)
    L = 4
    s.trajectory(L)
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
    s.p.neg_()
    s.trajectory(L)
    assert float((s.z - z0).abs().max()) < 1e-10


# ------------------------------------------------------------------ 4. per-patient sets beyond one workgroup round
def _oracle_gode(ode_rows, nn, x0, t, cot):
    from oracle import oracle as O   # checker only

    def work(i):
        b = i % x0.shape[0]
        sol = O.solve(x0[b:b + 1], t, None, None, None, ode_rows[i], nn, 64, 4, rtol=1e-10, atol=1e-12, dtype=np.float64, want_tape=True)
        return O.solve_bwd(sol, cot[i:i + 1], want_gnn=False, want_gode=True)[2]
    with ThreadPoolExecutor(NCPU) as ex:
        return np.stack(list(ex.map(work, range(len(ode_rows)))))


_SETS = {}


def _sets_case():
    """C = 5 chains x B = 64 patients = 320 sets of one trajectory each, T = 5; the oracle's per-set gode, computed once."""
    if not _SETS:
        from models.ode_core import ODE_PARAM_NAMES
        from inference.hmc import REFERENCE_PRIORS
        C, B, T = 5, 64, 5
        m = _model()
        rng = np.random.default_rng(2)
        x0 = (np.array([8.0, 90.0, 80.0, 10.0, 0.0, 0.5]) * (1 + 0.1 * rng.standard_normal((B, 6)))).astype(np.float32).astype(np.float64)
        t = np.linspace(0.0, 2.0, T).astype(np.float32).astype(np.float64)
        with torch.no_grad():
            nn, ode = m._params_on(DEV)
        nn, ode = nn.double().cpu().numpy(), ode.double().cpu().numpy()
        rows = np.tile(ode, (C * B, 1))
        for n in REFERENCE_PRIORS:
            j = ODE_PARAM_NAMES.index(n)
            rows[:, j] = (rows[:, j] * (1 + 0.1 * rng.standard_normal(C * B))).astype(np.float32)
        cot = rng.standard_normal((C * B, T, 6)).astype(np.float32).astype(np.float64)
        _SETS.update(C=C, B=B, T=T, m=m, x0=x0, t=t, nn=nn, rows=rows, cot=cot, ref=_oracle_gode(rows, nn, x0, t, cot))
    return _SETS


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_per_patient_sets_through_run_sets_vs_oracle(dt):
    """gode of every (chain, patient) set through _run_sets(own_sets=True) against the oracle's adjoint of that set on its own
    (fp64, 1e-10 / 1e-12), each against the set's largest entry, to 1e-4 (tests/test_sobol_gpu.py's 32-set adjoint); two calls
    give the same bits."""
    import models.hybrid_ode_nn as HN
    c = _sets_case()
    C, B, T = c["C"], c["B"], c["T"]
    R = dict(dtype=dt, device=DEV)
    x0, t = torch.as_tensor(c["x0"], **R), torch.as_tensor(c["t"], **R)
    ode_vec, nn = torch.as_tensor(c["rows"], **R).reshape(-1), torch.as_tensor(c["nn"], **R)
    cot = torch.as_tensor(c["cot"], **R).view(C, B, T, 6)
    plan = HN._plan_sets(DEV, C, B, T, hode.METHOD_DP54, x0.element_size(), 4, 64, None, max_traj=HN.OWN_SETS_MAX)
    assert plan[1] == [(0, C, 0, B)]
    stat = []

    def cotangent(sol, s0, s1, lo, hi):
        stat.append(sol.status)
        assert sol.y.shape[0] == (s1 - s0) * (hi - lo)
        return cot[s0:s1, lo:hi].reshape(sol.y.shape).contiguous()

    def run():
        return HN._run_sets(plan, cotangent, (False, False, True), x0, t, None, None, None, ode_vec, nn, 64, 4, hode.METHOD_DP54, 1e-6, 1e-8,
                            own_sets=True)[2]
    gode = run()
    assert int(stat[0].max()) == 0 and gode.numel() == C * B * 17
    got, ref = gode.view(C * B, 17).double().cpu().numpy(), c["ref"]
    worst = float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())
    print(f"\nown sets {dt}: worst gode error against the oracle {worst:.2e}")
    assert worst < 1e-4
    assert torch.equal(gode, run())
    with pytest.raises(ValueError):
        HN._run_sets(plan, cotangent, (False, True, True), x0, t, None, None, None, ode_vec, nn, 64, 4, hode.METHOD_DP54, 1e-6, 1e-8,
                     own_sets=True)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_a_chain_cut_into_patient_slices_reproduces_the_uncut_run(monkeypatch, dt):
    """A tape budget of 24 trajectories cuts every chain's 64 patients into three slices: loss_sum to 1e-15 relative, gode
    bitwise."""
    import models.hybrid_ode_nn as HN
    from inference.hmc import _Sampler
    from inference.population import _PopulationTarget
    m = _model()
    data = _data(m, B=64, T=5, sigma=0.2)
    s = _Sampler(m, data, 5, noise_sigma=0.2, seed=3, dtype=dt, target=_PopulationTarget(data))
    s.initial_jitter()
    s.leapfrog(hode.capi.HMC_PARAMS)
    s.evaluate()
    loss, gode, glik, status = s.loss_sum.clone(), s.gode_sets.clone(), s.glik.clone(), s.status.clone()
    assert int(status.max()) == 0 and tuple(status.shape) == (5, 64)
    elem = s.x0.element_size()
    steps = HN._small_tape_steps(s.C * s.N, s.T, s.method, elem, s.L, s.H, s.model.tape_steps) or HN._tape_steps(s.T, s.method, s.model.tape_steps)
    per = hode.capi.tape_nbytes(1, steps, elem, s.L, s.H)
    monkeypatch.setattr(HN, "TAPE_BUDGET_BYTES", 24 * per)
    plan = HN._plan_sets(s.dev, s.C, s.N, s.T, s.method, elem, s.L, s.H, s.model.tape_steps, max_traj=HN.OWN_SETS_MAX)
    assert plan[1] == [(c, c + 1, a, min(a + 24, 64)) for c in range(5) for a in (0, 24, 48)]
    s.evaluate()
    rel = float(((s.loss_sum - loss).abs() / loss).max())
    print(f"\ncut chains {dt}: loss_sum rel {rel:.2e}")
    assert rel <= 1e-15
    assert torch.equal(s.gode_sets, gode) and torch.equal(s.glik, glik) and torch.equal(s.status, status)


def test_trajectories_out_of_tape_steps_are_retried_in_one_launch(monkeypatch):
    """With a tape of T - 1 accepted steps some trajectories of the adaptive solve run out (status 1): they are solved again
    with their own constants in ONE launch, whatever their number, and loss_sum and gode are those of the run whose tape held
    every step.  fp64, the same discrete scheme and step sequence either way: 1e-12 / 1e-9 relative (summation order only)."""
    import models.hybrid_ode_nn as HN
    from inference.hmc import _Sampler
    from inference.population import _PopulationTarget
    m = _model()
    data = _data(m, B=8, T=13, sigma=0.2)
    s = _Sampler(m, data, 3, noise_sigma=0.2, seed=3, dtype=torch.float64, target=_PopulationTarget(data))
    s.initial_jitter()
    s.leapfrog(hode.capi.HMC_PARAMS)
    seen, real = [], HN._solve_taped

    def spy(*a, **k):
        sol = real(*a, **k)
        seen.append((sol.n_retried, [e[1] for e in sol.extras]))
        return sol
    monkeypatch.setattr(HN, "_solve_taped", spy)
    s.evaluate()
    assert seen == [(0, [])] and int(s.status.max()) == 0
    loss, gode = s.loss_sum.clone(), s.gode_sets.clone()
    m.tape_steps = 12
    s.evaluate()
    print(f"\nretried {seen[1][0]} of 24 trajectories")
    assert 0 < seen[1][0] and seen[1][1] == [None] and int(s.status.max()) == 0
    assert float(((s.loss_sum - loss).abs() / loss).max()) <= 1e-12
    torch.testing.assert_close(s.gode_sets, gode, rtol=1e-9, atol=1e-9 * float(gode.abs().max()))


def test_a_launch_holds_at_most_1024_sets():
    import models.hybrid_ode_nn as HN
    _, pieces = HN._plan_sets(DEV, 40, 32, 5, hode.METHOD_DP54, 4, 4, 64, None, max_traj=HN.OWN_SETS_MAX)
    assert pieces == [(s, min(s + 32, 40), 0, 32) for s in (0, 32)]
    _, pieces = HN._plan_sets(DEV, 2, 1500, 5, hode.METHOD_DP54, 4, 4, 64, None, max_traj=HN.OWN_SETS_MAX)
    assert pieces == [(s, s + 1, a, min(a + 1024, 1500)) for s in range(2) for a in (0, 1024)]
    assert HN._plan_sets(DEV, 40, 32, 5, hode.METHOD_DP54, 4, 4, 64, None)[1] == [(0, 40, 0, 32)]      # existing callers: as before


# ------------------------------------------------------------------ 5. prior only
@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
def test_prior_only_run_recovers_the_prior(sampler):
    from inference.hmc import REFERENCE_PRIORS, _ess, _split
    from inference.population import run_population
    r = run_population(_model(), None, num_samples=300, num_warmup=200, n_chains=64, sampler=sampler, n_leapfrog=8, seed=3, n_patients=5)
    assert tuple(r.draws.shape) == (64, 300, 7 * 7)
    pop, th = r.population(), r.patients()
    mu0 = torch.tensor([REFERENCE_PRIORS[n][0] for n in r.names], dtype=torch.float64, device=th.device)
    sd0 = torch.tensor([REFERENCE_PRIORS[n][1] for n in r.names], dtype=torch.float64, device=th.device)
    zb = ((th - pop["mu"].unsqueeze(2)) / pop["tau"].unsqueeze(2)).reshape(64, 300, -1)
    x = torch.cat([pop["mu"], pop["tau"].log(), zb], 2)                       # N(mu0, sd0^2), N(log tau0, omega^2), N(0, 1)
    want_m = torch.cat([mu0, sd0.log(), torch.zeros(35, dtype=torch.float64, device=th.device)])
    want_s = torch.cat([sd0, torch.full_like(sd0, 0.5), torch.ones(35, dtype=torch.float64, device=th.device)])
    flat = x.reshape(-1, x.shape[2])
    mean, psd = flat.mean(0), flat.std(0)
    mcse = psd / _ess(_split(x)).sqrt()
    print(f"\nprior {sampler}: worst |mean - mu| / mcse {float(((mean - want_m).abs() / mcse).max()):.2f}, "
          f"worst |sd ratio - 1| {float((psd / want_s - 1).abs().max()):.3f}")
    assert float(((mean - want_m).abs() / mcse).max()) < 5
    assert float((psd / want_s - 1).abs().max()) < 0.10
    assert int(r.stats["divergent"].sum()) == 0


# ------------------------------------------------------------------ 6. posterior against quadrature, two coupled patients
QUAD_SIGMA = 0.015
QUAD_TRUE = [0.0090, 0.0120]
QUAD_PRIOR = {"a_GI": (0.0104, 0.002)}


def _quadrature(m, data, sig, nq=48):
    """The exact posterior moments of (theta_1, theta_2, mu_pop, log tau) for K = 1, B = 2.  Given s, (theta_1, theta_2) are
    jointly Gaussian with mean mu0 and covariance tau(s)^2 I + sd0^2 1 1^T; s is mixed over nq Gauss-Hermite nodes; the
    likelihood of each patient is tabulated on a 1-D grid (forward_ode_sets), the (theta_1, theta_2) grid refined in three
    passes; mu_pop | theta, s is Gaussian in closed form.  -> (means [4], sds [4], the prior marginal sd of theta_b)."""
    mu0, sd0 = QUAD_PRIOR["a_GI"]
    tau0, w = sd0, 0.5
    x0, t, obs = data["initial_state"], data["time_points"], data["observations"].double()
    sq, wq = np.polynomial.hermite_e.hermegauss(nq)
    sq = torch.as_tensor(sq, dtype=torch.float64, device=DEV)
    lwq = torch.as_tensor(np.log(wq), dtype=torch.float64, device=DEV)
    tau2 = (tau0 * torch.exp(w * sq)) ** 2                                     # [Q]

    def loglik(grid, b):
        y = m.forward_ode_sets({"a_GI": grid.float()}, x0[b:b + 1], t).double()           # [n, 1, T, 6]
        return -((y - obs[b:b + 1]) ** 2).sum((1, 2, 3)) / (2 * sig ** 2)

    def moments(c1, w1, c2, w2, n):
        g1 = torch.linspace(c1 - w1, c1 + w1, n, dtype=torch.float64, device=DEV)
        g2 = torch.linspace(c2 - w2, c2 + w2, n, dtype=torch.float64, device=DEV)
        g1, g2 = g1.float().double(), g2.float().double()                      # the values the solve sees
        l1, l2 = loglik(g1, 0), loglik(g2, 1)
        d1, d2 = (g1 - mu0).view(n, 1, 1), (g2 - mu0).view(1, n, 1)
        a, bq = tau2.view(1, 1, -1) + sd0 ** 2, sd0 ** 2                       # Sigma = [[a, b], [b, a]]
        det = a * a - bq * bq
        quad = (a * d1 * d1 - 2 * bq * d1 * d2 + a * d2 * d2) / det
        lp = l1.view(n, 1, 1) + l2.view(1, n, 1) - 0.5 * quad - 0.5 * torch.log(det) + lwq.view(1, 1, -1)
        wgt = torch.exp(lp - lp.max())
        wgt = wgt / wgt.sum()
        prec = 1.0 / sd0 ** 2 + 2.0 / tau2.view(1, 1, -1)
        cm = (mu0 / sd0 ** 2 + (g1.view(n, 1, 1) + g2.view(1, n, 1)) / tau2.view(1, 1, -1)) / prec     # E[mu_pop | theta, s]
        lt = (math.log(tau0) + w * sq).view(1, 1, -1)
        vals = [g1.view(n, 1, 1).expand_as(wgt), g2.view(1, n, 1).expand_as(wgt), cm, lt.expand_as(wgt)]
        extra = [0.0, 0.0, 1.0 / prec, 0.0]                                    # the conditional variance of mu_pop
        mean = [float((wgt * v).sum()) for v in vals]
        sd = [math.sqrt(float((wgt * ((v - mv) ** 2 + e)).sum())) for v, mv, e in zip(vals, mean, extra)]
        return mean, sd

    prior_sd = math.sqrt(sd0 ** 2 + tau0 ** 2 * math.exp(2 * w * w))
    mean, sd = moments(mu0, 5 * prior_sd, mu0, 5 * prior_sd, 128)
    mean, sd = moments(mean[0], 6 * sd[0], mean[1], 6 * sd[1], 128)
    mean, sd = moments(mean[0], 6 * sd[0], mean[1], 6 * sd[1], 160)
    return mean, sd, prior_sd


def test_posterior_of_two_coupled_patients_matches_quadrature():
    """K = 1 (a_GI), B = 2, T = 13, data from two different true values (QUAD_TRUE), complete data, fixed sigma = QUAD_SIGMA.
    sigma is chosen from the quadrature alone so that the posterior sd of each theta_b lies between 0.3 and 0.7 of its prior
    marginal sd sqrt(sd0^2 + tau0^2 e^(2 omega^2)) = 3.25e-3: both the data and the population matter (asserted below).
    The quadrature's ratios over sigma: 0.015 -> 0.347 / 0.593 (posterior sds 1.13e-3 / 1.93e-3), 0.02 -> 0.434 / 0.672,
    0.03 -> 0.569 / 0.771, 0.05 -> 0.733 / 0.871, 0.1 -> 0.892 / 0.952, 0.5 -> 0.989 / 0.992: two hours of data on 13 points say
    little about a_GI unless the noise is small, hence 0.015.  HMC: means within 4 MCSE (ess("mean")), sds within 10 %."""
    from inference.hmc import _ess, _split
    from inference.population import run_population
    m = _model()
    sig = QUAD_SIGMA
    data = _data(m, B=2, T=13, sigma=sig, seed=2, ode={"a_GI": QUAD_TRUE})
    mean, sd, prior_sd = _quadrature(m, data, sig)
    print(f"\nquadrature: means {mean}, sds {sd}, sd(theta_b) / prior marginal sd {sd[0] / prior_sd:.3f} {sd[1] / prior_sd:.3f}")
    assert 0.3 < sd[0] / prior_sd < 0.7 and 0.3 < sd[1] / prior_sd < 0.7
    r = run_population(m, data, num_samples=200, num_warmup=150, n_chains=256, n_leapfrog=8, noise_sigma=sig, ode_priors=QUAD_PRIOR, seed=5)
    pop, th = r.population(), r.patients()
    x = torch.cat([th[:, :, :, 0], pop["mu"], pop["tau"].log()], 2)            # [C, n, 4]: theta_1, theta_2, mu_pop, log tau
    em = r.ess("mean")
    ess = _ess(_split(x))                                                      # what ess("mean") computes, with log tau for tau
    torch.testing.assert_close(ess[:3], torch.stack([em["patient.a_GI"][0], em["patient.a_GI"][1], em["pop.mu.a_GI"]]), rtol=1e-9, atol=0)
    flat = x.reshape(-1, 4)
    got_m, got_s = flat.mean(0), flat.std(0)
    mcse = got_s / ess.sqrt()
    print(f"hmc: means {got_m.tolist()}, sds {got_s.tolist()}, mcse {mcse.tolist()}")
    for i in range(4):
        assert abs(float(got_m[i]) - mean[i]) < 4 * float(mcse[i]), (i, got_m, mean, mcse)
        assert abs(float(got_s[i]) / sd[i] - 1) < 0.1, (i, got_s, sd)


# ------------------------------------------------------------------ 7. run properties
@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
def test_same_seed_same_draws(sampler):
    from inference.population import run_population
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    kw = dict(num_samples=10, num_warmup=20, n_chains=32, n_leapfrog=4, max_tree_depth=6, noise_sigma=0.5, seed=9, sampler=sampler)
    a, b = run_population(m, data, **kw), run_population(m, data, **kw)
    assert torch.equal(a.draws, b.draws) and tuple(a.draws.shape) == (32, 10, 7 * 6)
    keys = ["accept_prob", "log_posterior", "divergent", "failed_solve", "step_size", "inv_mass"]
    keys += ["tree_depth", "n_leapfrog", "trajectories_solved"] if sampler == "nuts" else []
    for k in keys:
        assert np.array_equal(a.stats[k], b.stats[k]), k


def test_chains_do_not_depend_on_the_chain_count():
    from inference.population import run_population
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    kw = dict(num_samples=20, num_warmup=0, n_leapfrog=4, noise_sigma=0.5, seed=1)
    r8, r4 = run_population(m, data, n_chains=8, **kw), run_population(m, data, n_chains=4, **kw)
    torch.testing.assert_close(r4.draws, r8.draws[:4], rtol=1e-5, atol=1e-6)
    assert np.array_equal(r4.stats["failed_solve"], r8.stats["failed_solve"][:4])


def test_failed_solves_are_rejected_and_counted():
    from inference.population import run_population
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    # K_m ~ N(7, 20^2) reaches K_m + G ~ 0: the GLP-1 production term blows up, the solve reports status 2 / 3.  noise_sigma = 20
    # lets the prior dominate, so every patient's own K_m (sd ~ 30 around the population mean) wanders that far in 40 iterations;
    # at noise_sigma = 0.5 the data hold the patients' K_m above -1.1 and a run of this size sees no failure at all
    r = run_population(m, data, num_samples=40, num_warmup=0, n_chains=16, n_leapfrog=4, noise_sigma=20.0,
                       ode_priors={"K_m": (7.0, 20.0), "k_L": (0.02, 0.005)}, seed=1)
    st = r.stats
    assert int(st["failed_solve"].sum()) > 0
    assert bool(st["divergent"][st["failed_solve"]].all()) and float(np.abs(st["accept_prob"][st["failed_solve"]]).max()) == 0.0
    assert bool(torch.isfinite(r.draws).all()) and np.isfinite(st["log_posterior"]).all()


def test_init_from_fit_patients_starts_at_a_lower_U():
    from inference import fit_patients
    from inference.hmc import _Sampler
    from inference.population import _PopulationTarget
    m = _model()
    pri = {"a_GI": (0.0104, 0.002), "k_I": (0.025, 0.005)}
    data = _data(m, B=4, T=13, sigma=0.05, ode={"a_GI": [0.0085, 0.0100, 0.0110, 0.0125], "k_I": [0.021, 0.024, 0.027, 0.030]})
    fit = fit_patients(m, data, params=("a_GI", "k_I"), noise_sigma=0.05, priors=pri)
    U = []
    for init in (None, fit, torch.stack([fit.params["a_GI"], fit.params["k_I"]], 1)):
        s = _Sampler(m, data, 2, noise_sigma=0.05, target=_PopulationTarget(data, ode_priors=pri, init=init))
        s.gradient()
        U.append(s.U.clone())
    print(f"\nU at the default start {U[0].tolist()}, from the fit {U[1].tolist()}")
    assert bool((U[1] < U[0]).all()) and torch.equal(U[1], U[2])


def test_run_population_end_to_end_on_4gi_batch():
    from hode.datagen import FourGIModel, GlucoseDataset
    from inference.population import run_population
    gen = torch.Generator(device=DEV).manual_seed(0)
    table, status = FourGIModel("T2DM").generate_cohort(32, duration_hours=5, sampling_interval_min=5, meal_times=(0.5, 2.5),
                                                        meal_sizes=(75, 50), noise_cv=0.1, generator=gen)
    ds = GlucoseDataset(table, sequence_length=61, stride=61)
    batch = ds.batch(torch.arange(32))
    m = _model()
    r = run_population(m, batch, num_samples=4, num_warmup=4, n_chains=4, n_leapfrog=2, seed=2)
    names = ["a_GI", "k_I", "rho", "E_max", "V_max", "K_m", "k_L"]
    s = r.samples
    assert r.names == names and tuple(r.draws.shape) == (4, 4, 7 * 34)
    assert list(s) == [f"pop.mu.{k}" for k in names] + [f"pop.tau.{k}" for k in names] + [f"patient.{k}" for k in names]
    assert s["pop.mu.a_GI"].shape == (4, 4) and s["pop.tau.k_L"].shape == (4, 4) and s["patient.K_m"].shape == (4, 4, 32)
    assert r.flat()["patient.K_m"].shape == (16, 32) and tuple(r.patients().shape) == (4, 4, 32, 7)
    assert r.stats["accept_prob"].shape == (4, 4) and r.stats["step_size"].shape == (4,) and tuple(r.pooling().shape) == (7,)
    summ = r.summary()
    assert list(summ) == list(s) and summ["patient.K_m"]["q975"].shape == (32,) and summ["pop.mu.rho"]["mean"].shape == ()
    pred = r.predict()
    assert tuple(pred.shape) == (16, 32, 61, 6)
    th = r.patients().reshape(16, 32, 7)
    for i in (0, 5, 15):              # draw i: patient b with their own constants = set b x patient b of forward_ode_sets
        want = m.forward_ode_sets({k: th[i, :, j].float() for j, k in enumerate(names)}, batch["initial_state"], batch["time_points"],
                                  batch["external_inputs"])
        torch.testing.assert_close(pred[i], want[torch.arange(32), torch.arange(32)], rtol=1e-6, atol=1e-6)
    first3 = lambda v: v[:3] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == 32 else v          # noqa: E731
    new = r.predict_new(batch["initial_state"][:3], first3(batch["time_points"]), {k: first3(v) for k, v in batch["external_inputs"].items()},
                        thin=2, seed=4)
    assert tuple(new.shape) == (8, 3, 61, 6) and bool(torch.isfinite(new).all())
    whole = r.predictive_summary(quantiles=(0.025, 0.975))
    assert tuple(whole.quantiles.shape) == (2, 32, 61, 6) and tuple(whole.mean.shape) == (32, 61, 6)
    one = 32 * 61 * 6 * 4
    for max_bytes in (one, 3 * one, 5 * one):
        cut = r.predictive_summary(quantiles=(0.025, 0.975), max_bytes=max_bytes)
        assert torch.equal(cut.quantiles, whole.quantiles) and torch.equal(cut.mean, whole.mean) and torch.equal(cut.std, whole.std)
        assert torch.equal(cut.pit, whole.pit, ) or bool(((cut.pit == whole.pit) | (cut.pit.isnan() & whole.pit.isnan())).all())
