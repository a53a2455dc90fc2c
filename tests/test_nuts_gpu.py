"""Multi-chain No-U-Turn sampling on the GPU (inference/nuts.py, csrc/hode_nuts.hip): the tree bookkeeping against the numpy
restatement of tests/_nuts_reference.py (prior only, then one iteration with a real likelihood, which pins the slot mapping
of the compacted solve), the prior, a posterior against quadrature, determinism and chain independence, failed solves,
the tree limits and the compaction, and run_nuts end to end on the 4GI data path."""
import math

import numpy as np
import pytest
import torch

import hode
import _nuts_reference as ref
from test_hmc_gpu import _data, _model, _torch_U_grad

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _sampler(model, data, C, depth, seed, **kw):
    from inference.nuts import _NutsSampler
    s = _NutsSampler(model, data, C, max_tree_depth=depth, seed=seed, jitter=0.0, **kw)
    s.initial_jitter()
    s.gradient()
    return s


# ------------------------------------------------------------------ 1. exact tree bookkeeping, prior only
def test_tree_bookkeeping_matches_the_restatement_on_the_prior():
    C, depth, n_iter, seed = 8, 6, 20, 21
    s = _sampler(_model(16, 2), None, C, depth, seed, sample_nn=False, dtype=torch.float64)
    D = s.D
    assert D == 7
    minv = np.array([0.5, 0.7, 1.0, 1.3, 1.6, 2.0, 0.8])
    s.minv[:D] = torch.as_tensor(minv, device=DEV)
    # step sizes from 0.05 (trees reach the depth limit) to 2.2 (unstable in the stiffest coordinate: divergences)
    s.log_eps.copy_(torch.log(torch.tensor([0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9, 2.2], dtype=torch.float64, device=DEV)))
    # the numpy Philox against hode_hmc_refresh's momentum words
    s.refresh(1234)
    for c in range(C):
        np.testing.assert_allclose(s.p[c, :D].cpu().numpy(), ref.momentum(seed, c, 1234, minv), rtol=1e-14, atol=1e-15)
    u_grad = lambda z: (0.5 * float(z @ z), z.copy(), False)          # noqa: E731  prior-standardised: U = |z|^2 / 2
    zs = [s.z[c, :D].cpu().numpy().copy() for c in range(C)]
    stats = torch.zeros(C, n_iter, 6, dtype=torch.float64, device=DEV)
    seen_depth, seen_div = set(), 0
    for it in range(n_iter):
        s.transition(it)
        eps = s.eps.cpu().numpy()
        s.finish(False, 0.8, None, stats, n_iter, it)
        st = stats[:, it].cpu().numpy()
        z_gpu = s.z[:, :D].cpu().numpy()
        for c in range(C):
            U, g, _ = u_grad(zs[c])
            r = ref.transition(zs[c], ref.momentum(seed, c, it, minv), g, U, float(eps[c]), minv, u_grad,
                               ref.philox_uniform(seed, c, it), depth)
            assert (int(st[c, 4]), int(st[c, 5]), bool(st[c, 2])) == (r["tree_depth"], r["n_leapfrog"], r["divergent"]), (it, c, st[c], r)
            np.testing.assert_allclose(z_gpu[c], r["z"], rtol=0, atol=1e-12)
            assert abs(st[c, 0] - r["accept_stat"]) < 1e-12 and abs(-st[c, 1] - r["U"]) < 1e-12
            zs[c] = r["z"]
            seen_depth.add(r["tree_depth"])
            seen_div += r["divergent"]
    assert depth in seen_depth and len(seen_depth) >= 3 and seen_div > 0, (seen_depth, seen_div)


# ------------------------------------------------------------------ 2. one iteration with a real likelihood
def test_one_iteration_with_a_likelihood_matches_the_restatement():
    C, depth, seed = 3, 4, 11
    m = _model(16, 2)
    s = _sampler(m, _data(m, B=2, T=5, sigma=0.2), C, depth, seed, noise_sigma=0.2, solver="rk4", dtype=torch.float64)
    D = s.D
    s.log_eps.copy_(torch.log(torch.tensor([0.004, 0.015, 0.05], dtype=torch.float64, device=DEV)))
    z0 = s.z.clone()
    minv = np.ones(D)

    def u_grad_of(c):
        def u_grad(z):
            zz = z0.clone()
            zz[c, :D] = torch.as_tensor(z, device=DEV)
            U, g = _torch_U_grad(s, zz)
            return float(U[c]), g[c].cpu().numpy(), False
        return u_grad

    s.transition(0)
    eps = s.eps.cpu().numpy()
    stats = torch.zeros(C, 1, 6, dtype=torch.float64, device=DEV)
    s.finish(False, 0.8, None, stats, 1, 0)
    st = stats[:, 0].cpu().numpy()
    for c in range(C):
        u_grad = u_grad_of(c)
        U, g, _ = u_grad(z0[c, :D].cpu().numpy())
        r = ref.transition(z0[c, :D].cpu().numpy(), ref.momentum(seed, c, 0, minv), g, U, float(eps[c]), minv, u_grad,
                           ref.philox_uniform(seed, c, 0), depth)
        assert (int(st[c, 4]), int(st[c, 5]), bool(st[c, 2])) == (r["tree_depth"], r["n_leapfrog"], r["divergent"]), (c, st[c], r)
        np.testing.assert_allclose(s.z[c, :D].cpu().numpy(), r["z"], rtol=0, atol=1e-10)
    assert s.solved == s.N * int(st[:, 5].sum())


# ------------------------------------------------------------------ 3. prior only
def test_prior_only_run_recovers_the_prior():
    from inference.hmc import REFERENCE_PRIORS
    from inference.nuts import run_nuts
    m = _model()
    r = run_nuts(m, None, num_samples=300, num_warmup=200, n_chains=64, seed=3)
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
    assert r.stats["tree_depth"].dtype == np.int64 and r.stats["tree_depth"].shape == (64, 300)


# ------------------------------------------------------------------ 4. posterior against quadrature
def test_posterior_matches_quadrature():
    from inference.nuts import run_nuts
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
    r = run_nuts(m, data, num_samples=200, num_warmup=150, n_chains=256, noise_sigma=sig, ode_priors=pri, sample_nn=False, seed=5)
    x = r.draws.double().reshape(-1, 2)
    mcse = x.std(0) / r.ess(kind="mean").sqrt()
    got_m, got_s = x.mean(0), x.std(0)
    assert abs(float(got_m[0]) - ma) < 4 * float(mcse[0]) and abs(float(got_m[1]) - mk) < 4 * float(mcse[1]), (got_m, ma, mk, mcse)
    assert abs(float(got_s[0]) / sa - 1) < 0.1 and abs(float(got_s[1]) / sk - 1) < 0.1, (got_s, sa, sk)


# ------------------------------------------------------------------ 5. determinism and chain independence
def test_same_seed_same_draws():
    from inference.nuts import run_nuts
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    kw = dict(num_samples=10, num_warmup=20, n_chains=32, noise_sigma=0.5, seed=9, max_tree_depth=6)
    a, b = run_nuts(m, data, **kw), run_nuts(m, data, **kw)
    assert torch.equal(a.draws, b.draws)
    for k in ("accept_prob", "log_posterior", "divergent", "failed_solve", "tree_depth", "n_leapfrog", "step_size", "inv_mass",
              "trajectories_solved"):
        assert np.array_equal(a.stats[k], b.stats[k]), k


def test_chains_do_not_depend_on_the_chain_count():
    from inference.nuts import run_nuts
    m = _model(16, 2)
    data = _data(m, B=3, T=9, sigma=0.3)
    # num_warmup < 20: per-chain step-size adaptation only (no pooled mass matrix), so every chain is on its own
    kw = dict(num_samples=12, num_warmup=10, noise_sigma=0.3, seed=4, max_tree_depth=5, dtype=torch.float64)
    r16, r8 = run_nuts(m, data, n_chains=16, **kw), run_nuts(m, data, n_chains=8, **kw)
    assert np.array_equal(r16.stats["tree_depth"][:8], r8.stats["tree_depth"])
    assert np.array_equal(r16.stats["n_leapfrog"][:8], r8.stats["n_leapfrog"])
    torch.testing.assert_close(r16.draws[:8], r8.draws, rtol=0, atol=1e-10)
    assert len(set(r16.stats["n_leapfrog"].reshape(-1).tolist())) > 1          # trees of different sizes: the active sets differed


# ------------------------------------------------------------------ 6. failed solves
def test_failed_solves_are_counted_and_a_divergent_first_leaf_keeps_the_state():
    from inference.nuts import run_nuts
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    # K_m ~ N(7, 20^2) reaches K_m + G ~ 0: the GLP-1 production term blows up, the solve reports status 2 / 3
    pri = {"K_m": (7.0, 20.0), "k_L": (0.02, 0.005)}
    r = run_nuts(m, data, num_samples=40, num_warmup=0, n_chains=16, noise_sigma=0.5, ode_priors=pri, sample_nn=False, seed=1,
                 max_tree_depth=6)
    st = r.stats
    assert int(st["failed_solve"].sum()) > 0 and int(st["divergent"].sum()) > 0
    assert bool(st["divergent"][st["failed_solve"]].all())
    assert bool(torch.isfinite(r.draws).all()) and np.isfinite(st["log_posterior"]).all()
    # a first leaf that diverges (step 50 prior sd in K_m): the tree ends at once, the chain keeps its state
    s = _sampler(m, data, 4, 6, 7, noise_sigma=0.5, ode_priors=pri, sample_nn=False)
    s.log_eps.fill_(math.log(50.0))
    z0, U0 = s.z.clone(), s.U.clone()
    s.transition(0)
    stats = torch.zeros(4, 1, 6, dtype=torch.float64, device=DEV)
    s.finish(False, 0.8, None, stats, 1, 0)
    st1 = stats[:, 0].cpu()
    assert bool((st1[:, 2] == 1).all() and (st1[:, 4] == 1).all() and (st1[:, 5] == 1).all()), st1
    assert torch.equal(s.z, z0) and torch.equal(s.U, U0)


# ------------------------------------------------------------------ 7. limits and compaction
def test_tree_limits_and_compacted_solves():
    from inference.nuts import run_nuts
    m = _model(16, 2)
    data = _data(m, B=3, T=9, sigma=0.3)
    N, C = 3, 12
    kw = dict(num_samples=8, num_warmup=0, n_chains=C, noise_sigma=0.3, seed=6)
    r = run_nuts(m, data, max_tree_depth=4, **kw)
    nl, td = r.stats["n_leapfrog"], r.stats["tree_depth"]
    assert nl.min() >= 1 and nl.max() <= 2 ** 4 - 1 and td.min() >= 1 and td.max() <= 4
    assert bool((nl <= 2 ** td - 1).all() and (nl >= 2 ** (td - 1)).all())
    solved = r.stats["trajectories_solved"]
    np.testing.assert_array_equal(solved, N * nl.sum(0))                      # N x sum_c leaves_c per iteration ...
    assert solved.sum() < N * C * nl.max(0).sum()                            # ... not N x C x max_c leaves_c
    r1 = run_nuts(m, data, max_tree_depth=1, **kw)
    assert bool((r1.stats["n_leapfrog"] == 1).all() and (r1.stats["tree_depth"] == 1).all())
    np.testing.assert_array_equal(r1.stats["trajectories_solved"], N * C)


# ------------------------------------------------------------------ 8. end to end on the 4GI batch
def test_run_nuts_end_to_end_on_4gi_batch():
    from hode.datagen import FourGIModel, GlucoseDataset
    from inference.nuts import run_nuts
    gen = torch.Generator(device=DEV).manual_seed(0)
    table, status = FourGIModel("T2DM").generate_cohort(32, duration_hours=5, sampling_interval_min=5, meal_times=(0.5, 2.5),
                                                        meal_sizes=(75, 50), noise_cv=0.1, generator=gen)
    ds = GlucoseDataset(table, sequence_length=61, stride=61)
    batch = ds.batch(torch.arange(32))
    m = _model()
    r = run_nuts(m, batch, 4, 4, 0.8, 3, None, n_chains=8, seed=2)
    s = r.samples
    names = [n for n, _ in m.nn_residual.named_parameters()]
    assert list(s) == [f"ode.{k}" for k in ("a_GI", "k_I", "rho", "E_max", "V_max", "K_m", "k_L")] + [f"nn.{n}" for n in names]
    for n, p in m.nn_residual.named_parameters():
        assert s[f"nn.{n}"].shape == (8, 4) + tuple(p.shape)
    assert r.flat()["ode.k_L"].shape == (32,)
    assert r.stats["accept_prob"].shape == (8, 4) and r.stats["step_size"].shape == (8,)
    assert r.stats["tree_depth"].shape == (8, 4) and r.stats["n_leapfrog"].shape == (8, 4)
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
