"""The observation model on the GPU (csrc/hode_obs.hip, inference/observation.py): the kernel against a torch-fp64 restatement
of the two likelihoods (fixed per-state sigma; sigma^2 ~ InvGamma integrated out), its agreement with hode_mse_sets on complete
data, the samplers on masked data (U and grad U, pieces, a posterior against quadrature with the noise inferred, failed solves,
a glucose-only 4GI batch) and HybridODENN.data_nll.

The oracle is the restatement below (`_restate`): with d = y - obs on the observed entries (0 elsewhere), S_k = sum d^2 of state k,
    fixed     nll = sum_k S_k / (2 sigma_k^2),                          gy = d / sigma_k^2
    marginal  nll = sum_{n_k > 0} (a_k + n_k/2) log(b_k + S_k/2),       gy = (a_k + n_k/2) / (b_k + S_k/2) d"""
import math

import numpy as np
import pytest
import torch

import hode
from test_hmc_gpu import _data, _model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = dict(dtype=torch.float64, device=DEV)


def _restate(y, obs, seen, marginal, w=None, a=None, b=None):
    """(sse [S, 6], nll [S], terms [S] = sum of |nll terms|, gy [S, len], n [6]); y [S, len], obs / seen [len]; element i is state
    i % 6.  The residual is formed in the input precision (as the kernel forms it), everything after it in fp64."""
    S, n_el = y.shape
    d = torch.where(seen, y - torch.where(seen, obs, torch.zeros_like(obs)), torch.zeros_like(y))
    k_of = torch.arange(n_el, device=y.device) % 6
    sse = torch.stack([(d[:, k_of == k].double() ** 2).sum(1) for k in range(6)], 1)
    n = torch.stack([seen[k_of == k].sum() for k in range(6)]).double()
    if not marginal:
        wt = torch.as_tensor(w, **F64)
        terms = 0.5 * wt * sse
        coef = wt.expand(S, 6)
    else:
        at, bt = torch.as_tensor(a, **F64), torch.as_tensor(b, **F64)
        on = n > 0
        terms = torch.where(on, (at + 0.5 * n) * torch.log(bt + 0.5 * sse), torch.zeros_like(sse))
        coef = torch.where(on, (at + 0.5 * n) / (bt + 0.5 * sse), torch.zeros_like(sse))
    gy = coef.to(y.dtype)[:, k_of] * d
    return sse, terms.sum(1), terms.abs().sum(1), gy, n


def _case(dt, n_el, S, off, gen):
    """y [S, n_el], obs [n_el] and an explicit mask: ~30 % NaN, state 2 missing entirely, ~10 % masked entries holding garbage
    (huge, inf, NaN).  off = 1: every pointer one element off a 16-byte boundary."""
    ybuf = torch.randn(S * n_el + off, dtype=dt, device=DEV, generator=gen)
    y = ybuf[off:].view(S, n_el)
    obuf = torch.randn(n_el + 4 + off, dtype=dt, device=DEV, generator=gen)
    obs = obuf[4 + off:]
    u = torch.rand(n_el, device=DEV, generator=gen)
    idx = torch.arange(n_el, device=DEV)
    obs[u < 0.3] = float("nan")
    obs[idx % 6 == 2] = float("nan")
    masked = (u > 0.9)
    obs[masked & (idx % 3 == 0)] = 1e30
    obs[masked & (idx % 3 == 1)] = float("inf")
    obs[masked & (idx % 3 == 2)] = float("nan")
    mbuf = torch.ones(n_el + 4 + off, dtype=torch.uint8, device=DEV)
    mask = mbuf[4 + off:]
    mask[masked] = 0
    seen = torch.isfinite(obs) & (mask != 0)
    return y, obs, mask, seen


def _close(got, want, rtol):
    assert got.shape == want.shape
    err = (got.double() - want.double()).abs()
    assert bool((err <= rtol * want.double().abs()).all()), float((err / want.double().abs().clamp_min(1e-300)).max())


# ------------------------------------------------------------------ 1. the kernel against the restatement
# (unaligned, 1001: the row-by-row path), (aligned, 1000 = 83 x 12 + 4: wide groups + a tail), (aligned, 32 x 61 x 6: wide only)
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("marginal", [False, True])
@pytest.mark.parametrize("n_el,off", [(1001, 1), (1000, 0), (32 * 61 * 6, 0), (1002, 0)])
@pytest.mark.parametrize("S", [1, 5])
def test_kernel_against_restatement(dt, marginal, n_el, off, S):
    cap = hode.capi
    gen = torch.Generator(device=DEV).manual_seed(1000 * S + n_el)
    y, obs, mask, seen = _case(dt, n_el, S, off, gen)
    sig = np.array([0.7, 1.3, 2.0, 0.5, 1.1, 0.9])
    a, b = np.array([2.0, 2.5, 2.0, 3.0, 2.0, 4.0]), np.array([0.5, 1.0, 1.5, 2.0, 0.25, 3.0])
    w = 1.0 / sig ** 2
    sse_w, nll_w, mag_w, gy_w, n = _restate(y, obs, seen, marginal, w, a, b)
    assert int(n[2]) == 0 and int(n.sum()) > 0.3 * n_el
    kw = dict(a=a, b=b, n=n.cpu().numpy()) if marginal else dict(w=w)
    mode = cap.OBS_MARGINAL if marginal else cap.OBS_FIXED

    def run(flags=0, sse=None, ls=None, yy=y, oo=obs, mm=mask):
        sse = torch.zeros(S, 6, **F64) if sse is None else sse
        ls = torch.zeros(S, **F64) if ls is None else ls
        gy = cap.obs_nll_sets(yy, oo, mm, mode, sse, ls, flags=flags, **kw)
        return sse, ls, gy

    sse, ls, gy = run()
    print(f"\n{dt} marginal={marginal} len={n_el} S={S}: sse rel err {float(((sse - sse_w).abs() / sse_w.clamp_min(1e-300)).max()):.2e}, "
          f"nll err / |terms| {float(((ls - nll_w).abs() / mag_w).max()):.2e}, "
          f"gy rel err {float(((gy.double() - gy_w.double()).abs() / gy_w.double().abs().clamp_min(1e-300))[gy_w != 0].max()):.2e}")
    _close(sse, sse_w, 1e-13)
    assert bool((sse[:, 2] == 0).all())                                  # the state that is missing entirely: exactly 0
    assert bool(((ls - nll_w).abs() <= 1e-13 * mag_w).all())
    # fixed: the tolerances of test_mse_sets_against_torch; marginal: the coefficient carries one fp64 division and one rounding
    # to the input precision more, so 4x those
    tol = (1e-6 if dt == torch.float32 else 1e-15) * (4 if marginal else 1)
    _close(gy, gy_w, tol)
    assert bool((gy[:, ~seen] == 0).all()) and bool(torch.isfinite(gy).all())
    # the same call gives the same bits
    sse2, ls2, gy2 = run()
    assert torch.equal(sse, sse2) and torch.equal(ls, ls2) and torch.equal(gy, gy2)
    # finiteness only (NULL mask) on observations whose masked entries were made NaN: the same observed set, the same bits
    obs_nan = torch.where(seen, obs, torch.full_like(obs, float("nan")))
    sse3, ls3, gy3 = run(oo=obs_nan, mm=None)
    assert torch.equal(sse, sse3) and torch.equal(ls, ls3) and torch.equal(gy, gy3)
    # sums only, then the cotangent from the finished sums = the fused call, bit for bit
    sse4 = torch.zeros(S, 6, **F64)
    ls4 = torch.zeros(S, **F64)
    assert run(cap.OBS_SUMS_ONLY, sse4, ls4)[2] is None and float(ls4.abs().max()) == 0.0
    _, _, gy4 = run(cap.OBS_FROM_SSE, sse4, ls4)
    assert torch.equal(sse, sse4) and torch.equal(ls, ls4) and torch.equal(gy, gy4)
    # sums only in two slices (cut at a row of six), then the cotangent of each slice from the whole set's sums
    cut = 6 * (n_el // 14)
    sse5, ls5 = torch.zeros(S, 6, **F64), torch.zeros(S, **F64)
    parts = [(y[:, :cut].contiguous(), obs[:cut].contiguous(), mask[:cut].contiguous()),
             (y[:, cut:].contiguous(), obs[cut:].contiguous(), mask[cut:].contiguous())]
    for yy, oo, mm in parts:
        run(cap.OBS_SUMS_ONLY, sse5, None, yy, oo, mm)
    assert float(((sse5 - sse).abs() / sse.clamp_min(1e-300)).max()) <= 1e-15
    g5 = [cap.obs_nll_sets(yy, oo, mm, mode, sse5, ls5 if i == 0 else None, flags=cap.OBS_FROM_SSE, **kw)
          for i, (yy, oo, mm) in enumerate(parts)]
    _close(torch.cat(g5, 1), gy_w, tol)
    assert bool(((ls5 - nll_w).abs() <= 1e-13 * mag_w).all())


def test_nonfinite_trajectory_reaches_the_loss():
    cap = hode.capi
    gen = torch.Generator(device=DEV).manual_seed(3)
    y, obs, mask, seen = _case(torch.float32, 1200, 3, 0, gen)
    first = int(torch.nonzero(seen)[0])
    y[1, first] = float("nan")
    y[2, int(torch.nonzero(~seen)[0])] = float("inf")              # under the mask: selected away
    for mode, kw in ((cap.OBS_FIXED, dict(w=np.ones(6))), (cap.OBS_MARGINAL, dict(a=np.full(6, 2.0), b=np.ones(6), n=np.full(6, 100.0)))):
        sse, ls = torch.zeros(3, 6, **F64), torch.zeros(3, **F64)
        cap.obs_nll_sets(y, obs, mask, mode, sse, ls, **kw)
        assert bool(torch.isfinite(ls[0])) and not bool(torch.isfinite(ls[1])) and bool(torch.isfinite(ls[2]))


# ------------------------------------------------------------------ 2. complete data: hode_mse_sets, and the samplers stay on it
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_fixed_mode_reproduces_mse_sets_on_complete_data(dt):
    gen = torch.Generator(device=DEV).manual_seed(0)
    S, n_el, sig = 5, 32 * 61 * 6, 0.37
    y, obs = torch.randn(S, n_el, dtype=dt, device=DEV, generator=gen), torch.randn(n_el, dtype=dt, device=DEV, generator=gen)
    scale = 0.5 / sig ** 2
    ls0 = torch.zeros(S, **F64)
    gy0 = hode.capi.mse_sets(y, obs, scale, ls0)
    sse, ls = torch.zeros(S, 6, **F64), torch.zeros(S, **F64)
    gy = hode.capi.obs_nll_sets(y, obs, None, hode.capi.OBS_FIXED, sse, ls, w=np.full(6, 1.0 / sig ** 2))
    _close(ls, scale * ls0, 1e-13)
    _close(sse.sum(1), ls0, 1e-13)
    _close(gy, gy0, 1e-6 if dt == torch.float32 else 1e-15)


def test_samplers_stay_on_mse_sets_for_complete_data_and_one_sigma(monkeypatch):
    from inference.hmc import run_hmc
    from inference.nuts import run_nuts
    calls = {"mse": 0, "obs": 0}
    mse, obs = hode.capi.mse_sets, hode.capi.obs_nll_sets

    def count(key, fn):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(hode.capi, "mse_sets", count("mse", mse))
    monkeypatch.setattr(hode.capi, "obs_nll_sets", count("obs", obs))
    m = _model(16, 2)
    data = _data(m, B=4, T=13, sigma=0.5)
    run_hmc(m, data, num_samples=3, num_warmup=3, n_chains=4, n_leapfrog=2, noise_sigma=0.5, seed=1)
    assert calls["mse"] > 0 and calls["obs"] == 0, calls
    calls["mse"] = 0
    run_nuts(m, data, 3, 3, 0.8, 3, None, n_chains=4, noise_sigma=0.5, seed=1)
    assert calls["mse"] > 0 and calls["obs"] == 0, calls
    # ... and leave it when they must: one missing entry
    d2 = dict(data, observations=data["observations"].clone())
    d2["observations"][0, 1, 0] = float("nan")
    calls["mse"] = 0
    run_hmc(m, d2, num_samples=2, num_warmup=0, n_chains=4, n_leapfrog=2, noise_sigma=0.5, seed=1)
    assert calls["mse"] == 0 and calls["obs"] > 0, calls


# ------------------------------------------------------------------ 3. U and grad U of the sampler on masked data
SIG6 = [0.2, 2.0, 2.0, 0.3, 0.05, 0.1]


def _masked(data, seed=4, garbage=float("nan")):
    """~30 % of the entries masked out (explicit mask, `garbage` underneath), state 5 NaN everywhere."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs = data["observations"].clone()
    mask = torch.rand(obs.shape, device=DEV, generator=g) > 0.3
    obs[~mask] = garbage
    obs[..., 5] = float("nan")
    return dict(data, observations=obs, observation_mask=mask)


def _obs_sampler(C=3, marginal=False, dtype=torch.float64, solver="rk4", garbage=float("nan"), B=2, T=5, **kw):
    from inference.hmc import _Sampler
    m = _model(16, 2)
    data = _masked(_data(m, B=B, T=T, sigma=0.2), garbage=garbage)
    s = _Sampler(m, data, C, noise_sigma=SIG6, noise="marginal" if marginal else "fixed", seed=11, solver=solver, dtype=dtype,
                 jitter=0.0, **kw)             # (kw may hold target=: another posterior over the same observation model)
    s.initial_jitter()
    s.gradient()
    return s, data


def _torch_U_grad_obs(s, z):
    """test_hmc_gpu._torch_U_grad with the restated observation model in place of the sum of squares."""
    from models.ode_core import ODE_PARAM_NAMES
    C, P, N = s.C, s.P, s.N
    zd = z[:, :s.D].double()
    ode = s.ode_base.double().reshape(1, 17).repeat(C, 1)
    idx = [ODE_PARAM_NAMES.index(n) for n in s.ode_names]
    ode[:, idx] = s.mu + s.sd * zd[:, :s.n_ode]
    nn = zd[:, s.n_ode:]
    sol = hode.solve_fwd(s.x0.repeat(C, 1), s.t.repeat(C, 1) if s.t.dim() == 2 else s.t, None, None, None, ode.reshape(-1),
                         nn.reshape(-1), s.H, s.L, method=hode.METHOD_RK4, n_sets=C, want_tape=True)
    om = s.om
    seen = (om.mask.reshape(-1) != 0) if om.mask is not None else torch.ones(om.obs.numel(), dtype=torch.bool, device=DEV)
    _, nll, _, gy, _ = _restate(sol.y.reshape(C, -1), om.obs.reshape(-1), seen, om.marginal, om.w, om.a, om.b)
    _, gnn, gode = hode.solve_bwd(sol, gy.view_as(sol.y), want_gnn=True, want_gode=True)
    grad = torch.cat([gode.view(C, 17)[:, idx] * s.sd, gnn.view(C, P)], 1) + zd
    return nll + 0.5 * (zd ** 2).sum(1), grad


@pytest.mark.parametrize("marginal", [False, True])
def test_sampler_U_and_gradient_on_masked_data(marginal):
    s, _ = _obs_sampler(marginal=marginal)
    assert s.obs_kernel and s.lik_scale == 1.0
    s.log_eps.fill_(math.log(0.02))
    s.refresh(5)
    U0, g0 = _torch_U_grad_obs(s, s.z.clone())
    torch.testing.assert_close(s.U, U0, rtol=1e-12, atol=0)
    torch.testing.assert_close(s.g[:, :s.D], g0, rtol=1e-12, atol=1e-12)
    s.trajectory(3)
    U1, g1 = _torch_U_grad_obs(s, s.z.clone())
    torch.testing.assert_close(s.U, U1, rtol=1e-12, atol=0)
    torch.testing.assert_close(s.g[:, :s.D], g1, rtol=1e-12, atol=1e-12)
    # the values under the mask change no bit
    s2, _ = _obs_sampler(marginal=marginal, garbage=1e30)
    s2.log_eps.fill_(math.log(0.02))
    s2.refresh(5)
    s2.trajectory(3)
    assert torch.equal(s.U, s2.U) and torch.equal(s.g, s2.g) and torch.equal(s.z, s2.z)


@pytest.mark.parametrize("marginal", [False, True])
def test_values_under_the_mask_change_no_bit_of_a_run(marginal):
    from inference.hmc import run_hmc
    from inference.nuts import run_nuts
    m = _model(16, 2)
    base = _data(m, B=4, T=13, sigma=0.2)
    kw = dict(noise_sigma=SIG6, noise="marginal" if marginal else "fixed", seed=3)
    da, db = _masked(base, garbage=float("nan")), _masked(base, garbage=-7e20)
    a, b = (run_hmc(m, d, num_samples=4, num_warmup=6, n_chains=8, n_leapfrog=3, **kw) for d in (da, db))
    assert torch.equal(a.draws, b.draws) and np.array_equal(a.stats["log_posterior"], b.stats["log_posterior"])
    a, b = (run_nuts(m, d, 4, 6, 0.8, 3, None, n_chains=8, **kw) for d in (da, db))
    assert torch.equal(a.draws, b.draws) and np.array_equal(a.stats["log_posterior"], b.stats["log_posterior"])


# ------------------------------------------------------------------ 4. a set cut into pieces (marginal mode: the forward pre-pass)
@pytest.mark.parametrize("dtype,solver,tol", [(torch.float64, "rk4", 1e-10), (torch.float32, "dopri5", 2e-6)])
def test_pieces_inside_a_set_reproduce_the_whole_set(monkeypatch, dtype, solver, tol):
    import models.hybrid_ode_nn as HN
    s, _ = _obs_sampler(C=3, marginal=True, dtype=dtype, solver=solver, B=4, T=7)
    U1, g1 = s.U.clone(), s.g.clone()
    elem = s.x0.element_size()
    steps = HN._small_tape_steps(s.C * s.N, s.T, s.method, elem, s.L, s.H, s.model.tape_steps) or HN._tape_steps(s.T, s.method, s.model.tape_steps)
    per = hode.capi.tape_nbytes(1, steps, elem, s.L, s.H)
    monkeypatch.setattr(HN, "TAPE_BUDGET_BYTES", 3 * per)            # 3 of a set's 4 trajectories per piece
    cap = max(1, HN._tape_budget(s.dev, s.C * s.N * per) // per)
    assert cap == 3 and len(HN._pieces(s.C, s.N, cap)) == 2 * s.C
    flags_seen, kernel = [], hode.capi.obs_nll_sets

    def spy(*a, **k):
        flags_seen.append(k.get("flags", 0))
        return kernel(*a, **k)
    monkeypatch.setattr(hode.capi, "obs_nll_sets", spy)
    s.gradient()
    # the forward-only pre-pass (sums only) over the six pieces, then their cotangents from the finished sums
    assert flags_seen == [hode.capi.OBS_SUMS_ONLY] * 6 + [hode.capi.OBS_FROM_SSE] * 6
    rel = lambda x, y: float((x - y).double().norm() / y.double().norm())           # noqa: E731
    print(f"\npieces {dtype}: U rel {rel(s.U, U1):.2e}, grad rel norm {rel(s.g, g1):.2e}")
    assert rel(s.U, U1) < tol and rel(s.g, g1) < tol
    # whole sets per piece (the fused call per piece): 4 trajectories = one set
    monkeypatch.setattr(HN, "TAPE_BUDGET_BYTES", 5 * per)
    del flags_seen[:]
    s.gradient()
    assert flags_seen == [0] * 3
    assert rel(s.U, U1) < tol and rel(s.g, g1) < tol


# ------------------------------------------------------------------ 5. posterior against quadrature, noise inferred
TRUE_SIG = [0.05, 0.5, 0.4, 0.1, 0.01, 0.02]


@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
def test_marginal_posterior_matches_quadrature(sampler):
    from inference.hmc import run_hmc
    from inference.nuts import run_nuts
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.0, seed=2, ode={"a_GI": 0.0110, "k_I": 0.022})
    g = torch.Generator(device=DEV).manual_seed(7)
    clean = data["observations"]
    obs = clean + torch.tensor(TRUE_SIG, device=DEV) * torch.randn(clean.shape, device=DEV, generator=g)
    obs[torch.rand(obs.shape, device=DEV, generator=g) < 0.25] = float("nan")           # ~25 % missing
    obs[..., 4:] = float("nan")                                                         # two states unobserved
    data = dict(data, observations=obs)
    guess = [0.1, 1.0, 1.0, 0.2, 0.05, 0.05]                                            # prior mean of sigma_k^2 = guess_k^2
    pri = {"a_GI": (0.0104, 0.002), "k_I": (0.025, 0.005)}
    x0, t = data["initial_state"], data["time_points"]
    seen = torch.isfinite(obs)
    obs0 = torch.where(seen, obs, torch.zeros_like(obs)).double()
    n = seen.sum((0, 1)).double()
    a0, b0 = torch.full((6,), 2.0, **F64), torch.tensor(guess, **F64) ** 2
    on = n > 0
    assert on.tolist() == [True] * 4 + [False] * 2

    def sse_of(a, k):
        y = m.forward_ode_sets({"a_GI": a, "k_I": k}, x0, t).double()
        return (torch.where(seen, y - obs0, torch.zeros_like(y)) ** 2).sum((1, 2))      # [S, 6]

    def logpost(a, k):
        sse = sse_of(a, k)
        nll = torch.where(on, (a0 + 0.5 * n) * torch.log(b0 + 0.5 * sse), torch.zeros_like(sse)).sum(1)
        za, zk = (a.double() - pri["a_GI"][0]) / pri["a_GI"][1], (k.double() - pri["k_I"][0]) / pri["k_I"][1]
        return -nll - 0.5 * (za ** 2 + zk ** 2), sse

    def moments(ca, wa, ck, wk, npts):
        ga = torch.linspace(ca - wa, ca + wa, npts, **F64)
        gk = torch.linspace(ck - wk, ck + wk, npts, **F64)
        A, K = torch.meshgrid(ga, gk, indexing="ij")
        lp, sse = logpost(A.reshape(-1).float(), K.reshape(-1).float())
        w = torch.exp(lp - lp.max())
        w = w / w.sum()
        a, k = A.reshape(-1), K.reshape(-1)
        ma, mk = float((w * a).sum()), float((w * k).sum())
        # E[sigma | theta] of sigma^2 ~ InvGamma(alpha, beta): sqrt(beta) Gamma(alpha - 1/2) / Gamma(alpha)
        al, be = a0 + 0.5 * n, b0 + 0.5 * sse
        e_sig = (w.unsqueeze(1) * be.sqrt() * torch.exp(torch.lgamma(al - 0.5) - torch.lgamma(al))).sum(0)
        return ma, mk, float((w * (a - ma) ** 2).sum().sqrt()), float((w * (k - mk) ** 2).sum().sqrt()), e_sig

    ma, mk, sa, sk, _ = moments(pri["a_GI"][0], 5 * pri["a_GI"][1], pri["k_I"][0], 5 * pri["k_I"][1], 128)
    ma, mk, sa, sk, _ = moments(ma, 6 * sa, mk, 6 * sk, 128)
    ma, mk, sa, sk, e_sig = moments(ma, 6 * sa, mk, 6 * sk, 160)
    kw = dict(num_samples=200, num_warmup=150, n_chains=256, noise_sigma=guess, noise="marginal", ode_priors=pri, sample_nn=False, seed=5)
    r = run_hmc(m, data, n_leapfrog=8, **kw) if sampler == "hmc" else run_nuts(m, data, **kw)
    x = r.draws.double().reshape(-1, 2)
    ess = r.ess(kind="mean")
    mcse = x.std(0) / ess.sqrt()
    got_m, got_s = x.mean(0), x.std(0)
    print(f"\n{sampler}: mean {got_m.tolist()} vs quadrature {[ma, mk]} (mcse {mcse.tolist()}); sd {got_s.tolist()} vs {[sa, sk]}")
    assert abs(float(got_m[0]) - ma) < 4 * float(mcse[0]) and abs(float(got_m[1]) - mk) < 4 * float(mcse[1]), (got_m, ma, mk, mcse)
    assert abs(float(got_s[0]) / sa - 1) < 0.1 and abs(float(got_s[1]) / sk - 1) < 0.1, (got_s, sa, sk)
    # the noise: the mean of the sigma_k draws against E_theta[E[sigma_k | theta]]; standard error from the spread of the draws
    # over the smaller effective sample size of the two sampled constants (the inner draws themselves are independent)
    sig = r.noise_sigma(data)
    assert tuple(sig.shape) == (256 * 200, 6) and bool(torch.isfinite(sig).all()) and bool((sig > 0).all())
    se = sig.std(0) / float(ess.min()) ** 0.5
    print(f"{sampler}: sigma recovered {sig.mean(0).tolist()}\n      quadrature {e_sig.tolist()}\n      true {TRUE_SIG} (se {se.tolist()})")
    for k in range(4):
        assert abs(float(sig[:, k].mean()) - float(e_sig[k])) < 5 * float(se[k]), (k, float(sig[:, k].mean()), float(e_sig[k]), float(se[k]))
    # the unobserved states are drawn from their prior InvGamma(2, guess^2): E[sigma] = guess Gamma(1.5) / Gamma(2)
    # (5 standard errors of the mean of independent draws: sd / mean of sigma is sqrt(1 / Gamma(1.5)^2 - 1) under that prior)
    for k in (4, 5):
        want = guess[k] * math.gamma(1.5)
        assert abs(float(sig[:, k].mean()) / want - 1) < 5 * math.sqrt(1 / math.gamma(1.5) ** 2 - 1) / math.sqrt(sig.shape[0])


# ------------------------------------------------------------------ 6. data_nll
def test_data_nll_matches_the_restatement_and_fills_gradients():
    from inference.observation import ObservationModel
    from models.hybrid_ode_nn import _SOLVERS, _SolveFn, _compute_device
    m = _model(16, 2)
    batch = _masked(_data(m, B=3, T=9, sigma=0.2))
    for marginal in (False, True):
        om = ObservationModel(SIG6, "marginal" if marginal else "fixed")
        # fp64: the module's forward() is fp32 only, so the restatement is applied to the same solve (_SolveFn) in fp64
        m.zero_grad()
        nll = m.data_nll(batch, om, dtype=torch.float64)
        assert nll.dtype == torch.float64 and nll.dim() == 0
        nll.backward()
        got = torch.cat([p.grad.flatten().double() for p in m.nn_residual.parameters()])
        m.zero_grad()
        dev = _compute_device()
        x0, t, ins = m._prep_inputs(batch["initial_state"], batch["time_points"], batch["external_inputs"], dev)
        nn_flat, ode_vec = m._params_on(dev)
        nl = m.nn_residual
        y = _SolveFn.apply(x0.double(), nn_flat.double(), ode_vec.double(), t.double(), None, None, None, nl.hidden_dim, nl.hip_layers,
                           _SOLVERS["dopri5"], 1e-6, 1e-8, 1, {}, m.tape_steps)
        seen = torch.isfinite(batch["observations"]) & batch["observation_mask"]
        obs = torch.where(seen, batch["observations"], torch.zeros_like(batch["observations"])).double()
        sse = (torch.where(seen, y - obs, torch.zeros_like(y)) ** 2).sum((0, 1))
        n = seen.sum((0, 1)).double()
        if marginal:
            a, b = torch.as_tensor(om.a, **F64), torch.as_tensor(om.b, **F64)
            want = torch.where(n > 0, (a + 0.5 * n) * torch.log(b + 0.5 * sse), torch.zeros_like(sse)).sum()
        else:
            want = (0.5 * sse / torch.tensor(SIG6, **F64) ** 2).sum()
        want.backward()
        ref = torch.cat([p.grad.flatten().double() for p in m.nn_residual.parameters()])
        rel = float((got - ref).norm() / ref.norm())
        print(f"\ndata_nll marginal={marginal}: value {float(nll):.12g} vs {float(want):.12g}, grad rel norm {rel:.2e}")
        assert abs(float(nll) - float(want)) <= 1e-8 * abs(float(want)) and float(ref.norm()) > 0 and rel < 1e-8
        # fp32 (the default): against the restatement on model.forward, to fp32 accuracy of the solve
        m.zero_grad()
        nll32 = m.data_nll(batch, om)
        nll32.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.nn_residual.parameters())
        assert sum(float(p.grad.abs().sum()) for p in m.nn_residual.parameters()) > 0
        with torch.no_grad():
            y32 = m.forward(batch["initial_state"], batch["time_points"], batch["external_inputs"]).double()
        sse32 = (torch.where(seen, y32 - obs, torch.zeros_like(y32)) ** 2).sum((0, 1))
        t32 = (torch.where(n > 0, (a + 0.5 * n) * torch.log(b + 0.5 * sse32), torch.zeros_like(sse32)) if marginal
               else 0.5 * sse32 / torch.tensor(SIG6, **F64) ** 2)
        assert abs(float(nll32) - float(t32.sum())) <= 1e-6 * float(t32.abs().sum())


# ------------------------------------------------------------------ 7. CGM: glucose only, noise inferred
def test_run_nuts_on_a_glucose_only_4gi_batch():
    from hode.datagen import FourGIModel, GlucoseDataset
    from inference.nuts import run_nuts
    gen = torch.Generator(device=DEV).manual_seed(0)
    table, status = FourGIModel("T2DM").generate_cohort(32, duration_hours=5, sampling_interval_min=5, meal_times=(0.5, 2.5),
                                                        meal_sizes=(75, 50), noise_cv=0.1, generator=gen)
    ds = GlucoseDataset(table, sequence_length=61, stride=61)
    batch = ds.batch(torch.arange(32))
    m = _model()
    full = run_nuts(m, batch, 4, 4, 0.8, 3, None, n_chains=8, seed=2)                  # the complete-data run of test_nuts_gpu
    cgm = dict(batch, observations=batch["observations"].clone())
    cgm["observations"][..., 1:] = float("nan")
    r = run_nuts(m, cgm, 4, 4, 0.8, 3, None, n_chains=8, seed=2, noise="marginal")
    assert r.observation.n.tolist() == [32 * 61.0, 0, 0, 0, 0, 0]
    assert bool(torch.isfinite(r.draws).all()) and np.isfinite(r.stats["log_posterior"]).all()
    # test_run_nuts_end_to_end_on_4gi_batch puts no bound on the failed solves of its run, only on what becomes of them: the
    # draws stay finite.  With one state observed and its noise inferred the posterior is far wider than the complete-data
    # one, so a proposal may leave the solvable region; it must then be rejected and counted like any other.
    fs = r.stats["failed_solve"]
    print(f"\nfailed solves: glucose only {int(fs.sum())}, complete data {int(full.stats['failed_solve'].sum())} of {fs.size} draws")
    assert bool(r.stats["divergent"][fs].all())
    sig = r.noise_sigma(cgm)
    assert tuple(sig.shape) == (32, 6) and bool(torch.isfinite(sig).all()) and bool((sig > 0).all())
    assert torch.equal(sig, r.noise_sigma())                                           # the run's batch is the default
    pred = r.predict(batch["initial_state"], batch["time_points"], batch["external_inputs"], observation_noise=True)
    clean = r.predict(batch["initial_state"], batch["time_points"], batch["external_inputs"])
    assert tuple(pred.shape) == (32, 32, 61, 6) and bool(torch.isfinite(pred).all()) and not torch.equal(pred, clean)
    # fixed mode: the fixed values repeated
    fx = run_nuts(m, cgm, 2, 2, 0.8, 2, None, n_chains=4, seed=2, noise_sigma=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert fx.noise_sigma().tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]] * 8


# ------------------------------------------------------------------ 8. failed solves on the new path
def test_failed_solves_are_rejected_and_counted_on_the_observation_path():
    """The recipe of test_hmc_gpu.test_failed_solves_are_rejected_and_counted (K_m ~ N(., 20^2) reaches K_m + G ~ 0: the GLP-1
    production term blows up, the solve reports status 2 / 3) with missing observations.  The model's own K_m is -3 here: with
    the noise inferred the chains take smaller steps and do not reach the pole from K_m = 7 within 40 iterations."""
    from inference.hmc import run_hmc
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN(ode_params={"K_m": -3.0}, nn_hidden=64, nn_layers=4, device=DEV)
    data = _data(m, B=4, T=13, sigma=0.5)
    data["observations"][:, ::3, 1] = float("nan")
    kw = dict(num_samples=40, num_warmup=0, n_leapfrog=4, noise_sigma=0.5, ode_priors={"K_m": (-3.0, 20.0), "k_L": (0.02, 0.005)},
              sample_nn=False, seed=1)
    for noise in ("fixed", "marginal"):
        r = run_hmc(m, data, n_chains=16, noise=noise, **kw)
        st = r.stats
        assert int(st["failed_solve"].sum()) > 0, noise
        assert bool(st["divergent"][st["failed_solve"]].all()) and float(np.abs(st["accept_prob"][st["failed_solve"]]).max()) == 0.0
        assert bool(torch.isfinite(r.draws).all()) and np.isfinite(st["log_posterior"]).all()
