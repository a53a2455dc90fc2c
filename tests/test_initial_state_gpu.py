"""Latent initial states on the GPU (inference/initial_state.py, csrc/hode_x0.hip): the two kernels against the numpy restatement
(tests/_initial_state_restatement.py), the transpose on the device, one x0 row per trajectory through
models.hybrid_ode_nn._run_sets(own_x0=True) against the oracle, U and grad U end to end against a torch restatement, the prior,
a joint posterior of a constant and an initial state against 2-D quadrature, incomplete records, and the properties of a run."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _initial_state_restatement as XR
import hode

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NCPU = max(1, min(os.cpu_count() or 1, 16))
X0_TYPICAL = [8.0, 90.0, 80.0, 10.0, 0.0, 0.5]
MEAN = [8.0, 90.0, 80.0, 10.0, 0.5, 0.5]


def _model(H=64, L=4, seed=0):
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(seed)
    return HybridODENN(nn_hidden=H, nn_layers=L, device=DEV)


def _data(model, B=4, T=13, sigma=0.05, seed=1, a_GI=0.0104):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.tensor(X0_TYPICAL, device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
    t = torch.linspace(0.0, 2.0, T, device=DEV)
    with torch.no_grad():
        y = model.forward_ode_sets({"a_GI": torch.tensor([a_GI])}, x0, t)[0]
    obs = y + sigma * torch.randn(y.shape, device=DEV, generator=g)
    return {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {}}


def _prior(states, link="identity", rel=0.1, B=None):
    from inference import InitialStatePrior
    m = np.array(MEAN) if B is None else np.tile(MEAN, (B, 1))
    sd = np.full_like(m, rel) if link == "log" else rel * np.abs(m) + 0.01          # (the log link's sd is that of log x0)
    return InitialStatePrior(m, sd, states=states, link=link)


# ------------------------------------------------------------------ 1. the kernels against the restatement
SHAPES = [(1, 1, 0, 1, 0), (3, 3, 7, 6, 7), (2, 257, 0, 4, 0), (2, 5, 2, 2, 14), (2, 5, 0, 6, 49)]


def _kernel_case(A, B, K, n_lat, off, dt, aligned, link, seed=0):
    rng = np.random.default_rng(seed + 1000 * A + 10 * B + K + 100 * n_lat + off + 7 * link)
    D = off + B * n_lat
    ld = (D + 3) // 4 * 4 if aligned else D
    lat = sorted(int(j) for j in rng.choice(6, n_lat, replace=False))
    idx = sorted(int(j) for j in rng.choice(17, K, replace=False))
    with_ode = K > 0 or off == 0                                  # (the population offset carries no constants block)
    m = np.array(MEAN) * (1 + 0.1 * rng.standard_normal((B, 6)))
    s = 0.1 * np.abs(m) + 0.01
    mu, sd = rng.uniform(0.01, 10.0, max(K, 1)), rng.uniform(0.01, 1.0, max(K, 1))
    f64 = dict(dtype=torch.float64, device=DEV)
    x0_base = rng.uniform(0.5, 2.0, (B, 6))
    x0_base[:, lat] = np.nan                                      # latent entries of the batch may be missing: never read
    c = dict(A=A, B=B, K=K, n_lat=n_lat, off=off, D=D, ld=ld, lat=lat, idx=idx, link=link, with_ode=with_ode, m=m, s=s, mu=mu, sd=sd,
             lat_mask=sum(1 << j for j in lat), ode_mask=sum(1 << j for j in idx), m_d=torch.tensor(m, **f64), s_d=torch.tensor(s, **f64),
             mu_d=torch.tensor(mu, **f64), sd_d=torch.tensor(sd, **f64))
    c["coords"] = torch.as_tensor(rng.standard_normal((A, ld)), dtype=dt, device=DEV)          # the pad holds values, too: never read
    c["x0_base"] = torch.as_tensor(x0_base, dtype=dt, device=DEV)
    c["ode_base"] = torch.as_tensor(rng.uniform(0.5, 2.0, 17), dtype=dt, device=DEV)
    c["gx0"] = torch.as_tensor(rng.standard_normal((A * B, 6)), dtype=dt, device=DEV)
    c["gode"] = torch.as_tensor(rng.standard_normal((A, 17)), dtype=dt, device=DEV)
    return c


def _params(c, coords=None):
    coords = c["coords"] if coords is None else coords
    x0 = torch.full((c["A"] * c["B"], 6), float("nan"), dtype=coords.dtype, device=DEV)
    ode = torch.full((c["A"], 17), float("nan"), dtype=coords.dtype, device=DEV)
    w = c["with_ode"]
    hode.capi.x0_params(c["A"], c["B"], c["n_lat"], c["ld"], c["off"], coords, c["lat_mask"], c["link"], c["m_d"], c["s_d"], c["x0_base"], x0,
                        c["K"] if w else 0, c["ode_mask"] if w else 0, c["mu_d"] if w else None, c["sd_d"] if w else None,
                        c["ode_base"] if w else None, ode if w else None)
    return x0, ode


def _grad(c, gx0=None):
    gx0 = c["gx0"] if gx0 is None else gx0
    out = torch.full((c["A"], c["ld"]), float("nan"), dtype=gx0.dtype, device=DEV)
    w = c["with_ode"]
    hode.capi.x0_grad(c["A"], c["B"], c["n_lat"], c["ld"], c["off"], c["coords"], c["lat_mask"], c["link"], c["m_d"], c["s_d"], gx0, out,
                      c["K"] if w else 0, c["ode_mask"] if w else 0, c["sd_d"] if w else None, c["gode"] if w else None)
    return out


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("link", [0, 1])
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("A,B,K,n_lat,off", SHAPES)
def test_x0_params_against_the_restatement(A, B, K, n_lat, off, aligned, link, dt):
    """fp64: within 1e-15 of the summed magnitudes of the terms (|m| + |s w|; |x0| (1 + |s w|) for the log link, where an ulp of
    exp's argument is that much of x0); fp32 adds one rounding, 2^-23 |want|, of the fp64 value computed from the same fp32
    inputs.  Fixed entries and unsampled constants are copied bit for bit; the outputs were NaN before the call and every entry
    is finite after it (the batch's latent entries ARE NaN: they are never read); a buffer that is not handed over stays NaN;
    two calls give the same bits."""
    c = _kernel_case(A, B, K, n_lat, off, dt, aligned, link)
    x0, ode = _params(c)
    got = x0.view(A, B, 6).double().cpu().numpy()
    cn = c["coords"].double().cpu().numpy()
    base = c["x0_base"].double().cpu().numpy()
    want, mag = XR.x0_params(cn, off, B, c["lat"], link, c["m"], c["s"], base)
    r32 = 2.0 ** -23 if dt == torch.float32 else 0.0
    err, bound = np.abs(got - want)[..., c["lat"]], 1e-15 * mag + r32 * np.abs(want[..., c["lat"]])
    print(f"\nx0_params {(A, B, K, n_lat, off)} {dt} aligned={aligned} link={link}: worst err / bound {float((err / bound).max()):.3f}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    fixed = [j for j in range(6) if j not in c["lat"]]
    assert np.array_equal(got[..., fixed], np.broadcast_to(base[:, fixed], (A, B, len(fixed))))
    if c["with_ode"]:
        go = ode.double().cpu().numpy()
        ob = c["ode_base"].double().cpu().numpy()
        wo, mo = XR.ode_params(cn, c["idx"], c["mu"], c["sd"], ob)
        assert np.all(np.isfinite(go)) and np.all(np.abs(go - wo)[:, c["idx"]] <= 1e-15 * mo + r32 * np.abs(wo[:, c["idx"]]))
        rest = [j for j in range(17) if j not in c["idx"]]
        assert np.array_equal(go[:, rest], np.broadcast_to(ob[rest], (A, len(rest))))
    else:
        assert bool(ode.isnan().all())
    x0b, odeb = _params(c)
    assert torch.equal(x0, x0b) and (torch.equal(ode, odeb) if c["with_ode"] else True)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("link", [0, 1])
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("A,B,K,n_lat,off", SHAPES)
def test_x0_grad_against_the_restatement(A, B, K, n_lat, off, aligned, link, dt):
    """Every entry is one product: the bound of x0_params, 1e-15 (fp64; plus 2^-23 for fp32's one rounding) of |g| (1 + |s w|)
    for the log link (exp's argument again) and of |g| for the identity link and the constants.  Values are written, not
    accumulated, and nothing else is touched: the buffer was NaN before the call, the entries the layer owns (w, and the K
    constants when gode is given) are finite afterwards, and every other entry -- the columns between the constants and off, which
    belong to another layer, and the pad D..ld -- is still NaN.  Two calls give the same bits."""
    c = _kernel_case(A, B, K, n_lat, off, dt, aligned, link)
    out = _grad(c)
    got = out.double().cpu().numpy()
    cn = c["coords"].double().cpu().numpy()
    want, mag = XR.x0_transpose(cn, off, B, c["lat"], link, c["m"], c["s"], c["gx0"].double().cpu().numpy().reshape(A, B, 6))
    sw = np.abs(c["s"][:, c["lat"]] * XR.split(cn, off, B, n_lat)).reshape(A, -1)
    r32 = 2.0 ** -23 if dt == torch.float32 else 0.0
    err, bound = np.abs(got[:, off:c["D"]] - want), (1e-15 * (1 + (sw if link else 0.0)) + r32) * mag
    print(f"\nx0_grad {(A, B, K, n_lat, off)} {dt} aligned={aligned} link={link}: worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound)
    owned = np.zeros(c["ld"], dtype=bool)
    owned[off:c["D"]] = True
    if c["with_ode"]:
        owned[:K] = True
        wo = XR.ode_transpose(c["gode"].double().cpu().numpy(), c["idx"], c["sd"])
        assert np.all(np.abs(got[:, :K] - wo) <= (1e-15 + r32) * np.abs(wo))
    assert np.all(np.isfinite(got[:, owned])) and np.all(np.isnan(got[:, ~owned]))
    assert torch.equal(out[:, torch.as_tensor(owned, device=DEV)], _grad(c)[:, torch.as_tensor(owned, device=DEV)])


# ------------------------------------------------------------------ 2. the transpose on the device
@pytest.mark.parametrize("link", [0, 1])
@pytest.mark.parametrize("A,B,K,n_lat,off", SHAPES)
def test_x0_grad_is_the_transpose_of_x0_params(A, B, K, n_lat, off, link):
    """fp64: <gx0, dx0/dw v> + <gode, d ode / dz v> against <hode_x0_grad(gx0, gode), v>, relative to the summed magnitudes of the
    terms: 5e-9, the population test's bound.  The map's derivative along v comes from central differences of hode_x0_params
    (identity link and the constants: h = 1e-6, no truncation, rounding eps |x0| / h relative to s |v| with |x0| / s <= 10: 2.2e-9
    per term, summed in quadrature) and, for the log link, from the restatement's closed form."""
    c = _kernel_case(A, B, K, n_lat, off, torch.float64, False, link, seed=3)
    rng = np.random.default_rng(17)
    h, D = 1e-6, c["D"]
    v = torch.as_tensor(rng.standard_normal((A, c["ld"])), dtype=torch.float64, device=DEV)
    xp, op = _params(c, c["coords"] + h * v)
    xm, om = _params(c, c["coords"] - h * v)
    lat = c["lat"]
    if link:
        d = XR.dx0_dw(c["coords"].cpu().numpy(), off, B, lat, link, c["m"], c["s"])
        Jx = torch.as_tensor(d, device=DEV) * v[:, off:D].view(A, B, n_lat)
    else:
        Jx = ((xp - xm) / (2 * h)).view(A, B, 6)[..., lat]
    lhs = (Jx * c["gx0"].view(A, B, 6)[..., lat]).reshape(A, -1).sum(1)
    g = _grad(c)
    rhs = (v[:, off:D] * g[:, off:D]).sum(1)
    scale = (v[:, off:D] * g[:, off:D]).abs().sum(1)
    if c["with_ode"] and K:
        lhs = lhs + (((op - om) / (2 * h)) * c["gode"])[:, c["idx"]].sum(1)
        rhs = rhs + (v[:, :K] * g[:, :K]).sum(1)
        scale = scale + (v[:, :K] * g[:, :K]).abs().sum(1)
    err = (lhs - rhs).abs()
    print(f"\ntranspose {(A, B, K, n_lat, off)} link={link}: worst err / scale {float((err / scale).max()):.2e}")
    assert bool((err <= 5e-9 * scale).all())


# ------------------------------------------------------------------ 3. one x0 row per trajectory through _run_sets
_ROWS = {}


def _rows_case():
    """C = 3 sets x B = 5 patients, T = 5, every (set, patient) with its own x0; the oracle's gx0 of every trajectory alone."""
    if not _ROWS:
        from oracle import oracle as O   # checker only
        from inference.hmc import REFERENCE_PRIORS
        from models.ode_core import ODE_PARAM_NAMES
        C, B, T = 3, 5, 5
        m = _model()
        rng = np.random.default_rng(2)
        x0 = (np.array(X0_TYPICAL) * (1 + 0.1 * rng.standard_normal((C * B, 6)))).astype(np.float32).astype(np.float64)
        t = np.linspace(0.0, 2.0, T).astype(np.float32).astype(np.float64)
        with torch.no_grad():
            nn, ode = m._params_on(DEV)
        nn, ode = nn.double().cpu().numpy(), ode.double().cpu().numpy()
        rows = np.tile(ode, (C, 1))
        for n in REFERENCE_PRIORS:
            j = ODE_PARAM_NAMES.index(n)
            rows[:, j] = (rows[:, j] * (1 + 0.1 * rng.standard_normal(C))).astype(np.float32)
        cot = rng.standard_normal((C * B, T, 6)).astype(np.float32).astype(np.float64)

        def work(i):
            sol = O.solve(x0[i:i + 1], t, None, None, None, rows[i // B], nn, 64, 4, rtol=1e-10, atol=1e-12, dtype=np.float64, want_tape=True)
            return O.solve_bwd(sol, cot[i:i + 1], want_gnn=False, want_gode=False)[0][0]
        with ThreadPoolExecutor(NCPU) as ex:
            ref = np.stack(list(ex.map(work, range(C * B))))
        _ROWS.update(C=C, B=B, T=T, m=m, x0=x0, t=t, nn=nn, rows=rows, cot=cot, ref=ref)
    return _ROWS


@pytest.mark.parametrize("own_sets", [False, True])
@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_own_x0_through_run_sets_vs_oracle(dt, own_sets):
    """gx0 of every (set, patient) row through _run_sets(own_x0=True) against the oracle's adjoint of that trajectory alone (fp64,
    1e-10 / 1e-12), each against the row's largest entry, to 1e-4 (test_per_patient_sets_through_run_sets_vs_oracle's bound);
    the statuses are 0 and two calls give the same bits.  own_sets=True: the same rows with one set of constants per trajectory."""
    import models.hybrid_ode_nn as HN
    c = _rows_case()
    C, B, T = c["C"], c["B"], c["T"]
    R = dict(dtype=dt, device=DEV)
    x0, t = torch.as_tensor(c["x0"], **R), torch.as_tensor(c["t"], **R)
    nn1 = torch.as_tensor(c["nn"], **R)
    if own_sets:
        ode_vec, nn = torch.as_tensor(np.repeat(c["rows"], B, axis=0), **R).reshape(-1), nn1
    else:
        ode_vec, nn = torch.as_tensor(c["rows"], **R).reshape(-1), nn1.repeat(C)
    cot = torch.as_tensor(c["cot"], **R).view(C, B, T, 6)
    plan = HN._plan_sets(DEV, C, B, T, hode.METHOD_DP54, x0.element_size(), 4, 64, None, max_traj=HN.OWN_SETS_MAX if own_sets else None)
    assert plan[1] == [(0, C, 0, B)]
    stat = []

    def cotangent(sol, s0, s1, lo, hi):
        stat.append(sol.status)
        assert sol.y.shape[0] == (s1 - s0) * (hi - lo)
        return cot[s0:s1, lo:hi].reshape(sol.y.shape).contiguous()

    def run():
        return HN._run_sets(plan, cotangent, (True, False, False), x0, t, None, None, None, ode_vec, nn, 64, 4, hode.METHOD_DP54, 1e-6, 1e-8,
                            own_sets=own_sets, own_x0=True)[0]
    gx0 = run()
    assert int(stat[0].max()) == 0 and tuple(gx0.shape) == (C * B, 6)
    got, ref = gx0.double().cpu().numpy(), c["ref"]
    worst = float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())
    print(f"\nown x0 {dt} own_sets={own_sets}: worst gx0 error against the oracle {worst:.2e}")
    assert worst < 1e-4
    assert torch.equal(gx0, run())


def _latent_sampler(m, data, C, pop=False, **kw):
    from inference.hmc import _Sampler
    from inference.initial_state import _LatentTarget
    from inference.population import _PopulationTarget
    t = _LatentTarget(kw.pop("initial_state"), data, ode_priors=kw.pop("ode_priors", None), inner=_PopulationTarget(data) if pop else None)
    return _Sampler(m, data, C, target=t, **kw)


@pytest.mark.parametrize("own_sets", [False, True])
@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_chains_cut_into_patient_slices_reproduce_the_uncut_run(monkeypatch, dt, own_sets):
    """A tape budget of 24 trajectories cuts every chain's 64 patients into three slices: gx0, y and the statuses bit for bit,
    loss_sum to 1e-15 relative.  own_sets=True: the population row in front of the initial states."""
    import models.hybrid_ode_nn as HN
    m = _model()
    C, B, T = 5, 64, 5
    data = _data(m, B=B, T=T, sigma=0.2)
    s = _latent_sampler(m, data, C, pop=own_sets, noise_sigma=0.2, seed=3, dtype=dt, initial_state=_prior(("G", "I", "FFA")))
    s.initial_jitter()
    s.leapfrog(hode.capi.HMC_PARAMS)
    Y = torch.full((C, B, T, 6), float("nan"), dtype=dt, device=DEV)
    real = s._mse_piece

    def spy(stat, sol, s0, s1, lo, hi):
        Y[s0:s1, lo:hi] = sol.y.view(s1 - s0, hi - lo, T, 6)
        return real(stat, sol, s0, s1, lo, hi)
    s._mse_piece = spy
    s.evaluate()
    loss, gx0, glik, status, y = s.loss_sum.clone(), s.gx0_rows.clone(), s.glik.clone(), s.status.clone(), Y.clone()
    assert int(status.max()) == 0 and tuple(status.shape) == (C, B) and tuple(gx0.shape) == (C * B, 6) and bool(torch.isfinite(y).all())
    assert not torch.equal(y[0, :, 0], y[1, :, 0])                       # every chain starts from its own initial states
    elem = s.x0.element_size()
    steps = HN._small_tape_steps(s.C * s.N, s.T, s.method, elem, s.L, s.H, s.model.tape_steps) or HN._tape_steps(s.T, s.method, s.model.tape_steps)
    per = hode.capi.tape_nbytes(1, steps, elem, s.L, s.H)
    monkeypatch.setattr(HN, "TAPE_BUDGET_BYTES", 24 * per)
    plan = HN._plan_sets(s.dev, s.C, s.N, s.T, s.method, elem, s.L, s.H, s.model.tape_steps, max_traj=HN.OWN_SETS_MAX if own_sets else None)
    assert plan[1] == [(c, c + 1, a, min(a + 24, 64)) for c in range(5) for a in (0, 24, 48)]
    Y.fill_(float("nan"))
    s.evaluate()
    rel = float(((s.loss_sum - loss).abs() / loss).max())
    print(f"\ncut chains {dt} own_sets={own_sets}: loss_sum rel {rel:.2e}")
    assert rel <= 1e-15
    assert torch.equal(s.gx0_rows, gx0) and torch.equal(Y, y) and torch.equal(s.status, status)
    assert torch.equal(s.glik[:, s.target.off:], glik[:, s.target.off:])               # (a chain's gode is summed over its slices: not bitwise)
    if own_sets:
        assert torch.equal(s.glik, glik)                                 # one gode row per trajectory: nothing is summed across slices


# ------------------------------------------------------------------ 4. U and grad U end to end
def _small_sampler(kind, link, C=3):
    m = _model(16, 2)
    data = _data(m, B=3, T=5, sigma=0.2)
    kw = dict(noise_sigma=0.2, seed=11, solver="rk4", dtype=torch.float64, jitter=0.0, initial_state=_prior(("G", "I", "GLP1"), link, B=3))
    if kind == "K0":
        kw["ode_priors"] = {}
    s = _latent_sampler(m, data, C, pop=kind == "pop", **kw)
    s.initial_jitter()
    s.gradient()
    return s


def _torch_U_grad(s, z):
    """U and grad U by ONE fp64 solve of the mapped rows, the residuals, the adjoint, and the map and its transpose in torch."""
    from models.ode_core import ODE_PARAM_NAMES
    t, pop = s.target, s.target.inner
    C, B, lat, off = s.C, t.lat.B, t.lat, t.off
    zd = z[:, :s.D].double()
    w = zd[:, off:].reshape(C, B, lat.n_lat)
    ml, sl = lat.m[:, lat.states].to(DEV), lat.s[:, lat.states].to(DEV)
    xl = ml * torch.exp(sl * w) if lat.link_code else ml + sl * w
    x0 = s.x0.double().unsqueeze(0).repeat(C, 1, 1)
    x0[..., lat.states] = xl
    if pop is not None:
        K, om = pop.K, pop.omega
        m_, s_, zz = zd[:, :K], zd[:, K:2 * K], zd[:, 2 * K:off].reshape(C, B, K)
        mu, tau = pop.mu0 + pop.sd0 * m_, pop.tau0 * torch.exp(om * s_)
        idx = [ODE_PARAM_NAMES.index(n) for n in pop.pop_names]
        ode = s.ode_base.double().reshape(1, 17).repeat(C * B, 1)
        ode[:, idx] = (mu.unsqueeze(1) + tau.unsqueeze(1) * zz).reshape(C * B, K)
        n_sets = C * B
    else:
        K = t.g_K
        idx = [ODE_PARAM_NAMES.index(n) for n in t.g_names]
        ode = s.ode_base.double().reshape(1, 17).repeat(C, 1)
        if K:
            ode[:, idx] = t.g_mu + t.g_sd * zd[:, :K]
        n_sets = C
    sol = hode.solve_fwd(x0.reshape(C * B, 6).contiguous(), s.t, None, None, None, ode.reshape(-1), s.nn_base.double().repeat(n_sets), s.H, s.L,
                         method=hode.METHOD_RK4, n_sets=n_sets, want_tape=True)
    r = sol.y.view(C, B, -1) - s.obs.view(1, B, -1)
    ss = (r ** 2).sum((1, 2))
    gx0, _, gode = hode.solve_bwd(sol, (2 * s.lik_scale * r).view_as(sol.y), want_gnn=False, want_gode=K > 0)
    gw = (gx0.view(C, B, 6)[..., lat.states] * (sl * xl if lat.link_code else sl)).reshape(C, -1)
    if pop is not None:
        G = gode.view(C, B, 17)[:, :, idx]
        parts = [pop.sd0 * G.sum(1), om * tau * (G * zz).sum(1), (tau.unsqueeze(1) * G).reshape(C, B * K), gw]
    else:
        parts = ([t.g_sd * gode.view(C, 17)[:, idx]] if K else []) + [gw]
    return s.lik_scale * ss + 0.5 * (zd ** 2).sum(1), torch.cat(parts, 1) + zd


@pytest.mark.parametrize("link", ["identity", "log"])
@pytest.mark.parametrize("kind", ["K7", "K0", "pop"])
def test_one_trajectory_matches_torch_fp64_and_is_reversible(kind, link):
    """sampler.gradient() against the torch recomputation to rtol 1e-12 for the row [ z_ode (7) | w ], for pure state estimation
    (ode_priors = {}: K = 0) and for the population row [ m | s | z | w ]; then 4 leapfrog steps against the torch leapfrog to
    1e-12, reversed to 1e-10."""
    s = _small_sampler(kind, link)
    n_w = 3 * 3
    assert (s.target.off, s.D) == {"K7": (7, 7 + n_w), "K0": (0, n_w), "pop": (35, 35 + n_w)}[kind] and s.ld == (s.D + 3) // 4 * 4
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


# ------------------------------------------------------------------ 5. prior only
@pytest.mark.parametrize("link", ["identity", "log"])
@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
def test_prior_only_run_recovers_the_prior(sampler, link):
    """data=None: every x0 coordinate is N(m, s^2) (identity link) or log-normal, log x0 ~ N(log m, s^2) (log link), and the
    constants N(mu, sd^2): means within 5 MCSE, sds within 10 %, no divergence (test_population_gpu's numbers)."""
    from inference.hmc import REFERENCE_PRIORS, _ess, _split, run_hmc
    from inference.nuts import run_nuts
    prior = _prior(None, link)
    kw = dict(num_samples=300, num_warmup=200, n_chains=64, seed=3, sample_nn=False, initial_state=prior, n_patients=5)
    r = run_hmc(_model(), None, n_leapfrog=8, **kw) if sampler == "hmc" else run_nuts(_model(), None, **kw)
    assert tuple(r.draws.shape) == (64, 300, 7 + 5 * 6) and r.samples["x0"].shape == (64, 300, 5, 6)
    x = r.draws.double().clone()
    m, s = prior.mean.to(x.device).repeat(5), prior.sd.to(x.device).repeat(5)
    if link == "log":
        x[..., 7:] = x[..., 7:].log()
        m = m.log()
    want_m = torch.cat([torch.tensor([REFERENCE_PRIORS[n][0] for n in r.ode_names], dtype=torch.float64, device=x.device), m])
    want_s = torch.cat([torch.tensor([REFERENCE_PRIORS[n][1] for n in r.ode_names], dtype=torch.float64, device=x.device), s])
    flat = x.reshape(-1, x.shape[2])
    mean, psd = flat.mean(0), flat.std(0)
    mcse = psd / _ess(_split(x)).sqrt()
    print(f"\nprior {sampler} {link}: worst |mean - mu| / mcse {float(((mean - want_m).abs() / mcse).max()):.2f}, "
          f"worst |sd ratio - 1| {float((psd / want_s - 1).abs().max()):.3f}")
    assert float(((mean - want_m).abs() / mcse).max()) < 5
    assert float((psd / want_s - 1).abs().max()) < 0.10
    assert int(r.stats["divergent"].sum()) == 0
    assert bool(r.initial_states().isnan().logical_not().all())          # all six are latent: nothing is left to the batch


# ------------------------------------------------------------------ 6. joint posterior against 2-D quadrature
def test_joint_posterior_of_a_constant_and_an_initial_state_matches_quadrature():
    """a_GI and x0_I of one patient, T = 13, sigma = 0.015, the prior of x0_I off by 0.3 s from the truth (s = 0.015).  The exact
    moments come from a 96 x 96 grid over a_GI +- 5 sd0 and x0_I +- 6 s (one forward_ode_sets launch).  A CPU check with the C
    oracle gave posterior sd / prior sd 0.749 (a_GI) and 0.377 (x0_I), correlation -0.69, edge mass 1e-10 (this quadrature: 0.749,
    0.377, -0.688, 1.4e-10); the test first asserts on its own quadrature that both ratios lie in (0.3, 0.8) and |rho| >= 0.4: the
    data, both priors and their coupling all matter.  HMC: both means within 4 MCSE (ess("mean")), both sds within 10 %, the
    correlation within 4 (1 - rho^2) / sqrt(ESS_min) -- four standard errors of a sample correlation.

    ESS_min is the smallest effective sample size of the series the sample correlation is an average of, the standardised squares
    and cross product z_1^2, z_2^2, z_1 z_2 (z_i = (x_i - mean_i) / sd_i with the quadrature's moments), NOT that of the means.
    At n_leapfrog = 8 the trajectory of this two-coordinate posterior is about half a period long: a transition nearly reflects
    the chain about the mean, so the means are antithetic (ess("mean") 1.0e5 to 1.5e5 from 51 200 draws) while x^2 and x_1 x_2
    barely move from one draw to the next (ESS 1 000 to 2 100, measured).  With the ESS of the means the formula is not the
    standard error of anything the test looks at: over the seeds 5..10 the sample correlation was -0.675, -0.691, -0.694, -0.685,
    -0.675, -0.701 (mean -0.687 against the quadrature's -0.688, spread 0.010 where 4 (1 - rho^2) / sqrt(1.0e5) = 0.0066), and
    -0.685 from 1 000 draws per chain, -0.691 / -0.689 at n_leapfrog = 5 / 13 (second-moment ESS 36 000 / 31 000), -0.693 in fp64."""
    from inference import InitialStatePrior
    from inference.hmc import _ess, _split, run_hmc
    m = _model()
    sig, s0, (mu0, sd0), nq = 0.015, 0.015, (0.0104, 0.002), 96
    rng = np.random.default_rng(7)
    x0 = torch.as_tensor(np.array(X0_TYPICAL) * (1 + 0.1 * rng.standard_normal((1, 6))), dtype=torch.float32, device=DEV)
    t = torch.linspace(0.0, 2.0, 13, device=DEV)
    with torch.no_grad():
        y = m.forward_ode_sets({"a_GI": torch.tensor([0.0090])}, x0, t)[0]
    obs = y + torch.as_tensor(0.015 * rng.standard_normal(tuple(y.shape)), dtype=torch.float32, device=DEV)
    data = {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {}}
    x0_I = float(x0[0, 1])
    mean = np.array(MEAN)
    mean[1] = x0_I + 0.3 * s0
    prior = InitialStatePrior(mean, np.full(6, s0), states=("I",))
    # ---- quadrature
    f64 = dict(dtype=torch.float64, device=DEV)
    ga = torch.linspace(mu0 - 5 * sd0, mu0 + 5 * sd0, nq, **f64).float().double()              # the values the solve sees
    gx = torch.linspace(x0_I - 6 * s0, x0_I + 6 * s0, nq, **f64).float().double()
    xs = x0.repeat(nq, 1)
    xs[:, 1] = gx.float()
    with torch.no_grad():
        yq = m.forward_ode_sets({"a_GI": ga.float()}, xs, t).double()                          # [a, x, T, 6]
    lp = (-((yq - obs.double().view(1, 1, 13, 6)) ** 2).sum((2, 3)) / (2 * sig ** 2) - 0.5 * ((ga.view(-1, 1) - mu0) / sd0) ** 2
          - 0.5 * ((gx.view(1, -1) - mean[1]) / s0) ** 2)
    wgt = torch.exp(lp - lp.max())
    wgt = wgt / wgt.sum()
    edge = float(wgt[0].sum() + wgt[-1].sum() + wgt[:, 0].sum() + wgt[:, -1].sum())
    A, X = ga.view(-1, 1).expand_as(wgt), gx.view(1, -1).expand_as(wgt)
    qm = [float((wgt * A).sum()), float((wgt * X).sum())]
    qs = [math.sqrt(float((wgt * (A - qm[0]) ** 2).sum())), math.sqrt(float((wgt * (X - qm[1]) ** 2).sum()))]
    rho = float((wgt * (A - qm[0]) * (X - qm[1])).sum()) / (qs[0] * qs[1])
    print(f"\nquadrature: means {qm}, sds {qs}, sd ratios {qs[0] / sd0:.3f} {qs[1] / s0:.3f}, rho {rho:.3f}, edge mass {edge:.1e}")
    assert 0.3 < qs[0] / sd0 < 0.8 and 0.3 < qs[1] / s0 < 0.8 and abs(rho) >= 0.4 and edge < 1e-6
    # ---- sampler
    r = run_hmc(m, data, num_samples=200, num_warmup=150, n_chains=256, n_leapfrog=8, noise_sigma=sig, ode_priors={"a_GI": (mu0, sd0)},
                sample_nn=False, initial_state=prior, seed=5)
    x = r.draws.double()
    assert tuple(x.shape) == (256, 200, 2) and int(r.stats["failed_solve"].sum()) == 0
    ess = r.ess("mean")
    flat = x.reshape(-1, 2)
    got_m, got_s = flat.mean(0), flat.std(0)
    mcse = got_s / ess.sqrt()
    got_rho = float(torch.corrcoef(flat.T)[0, 1])
    print(f"hmc: means {got_m.tolist()}, sds {got_s.tolist()}, mcse {mcse.tolist()}, rho {got_rho:.3f}, ess {ess.tolist()}")
    for i in range(2):
        assert abs(float(got_m[i]) - qm[i]) < 4 * float(mcse[i]), (i, got_m, qm, mcse)
        assert abs(float(got_s[i]) / qs[i] - 1) < 0.1, (i, got_s, qs)
    zq = (x - torch.tensor(qm, dtype=torch.float64, device=x.device)) / torch.tensor(qs, dtype=torch.float64, device=x.device)
    ess2 = _ess(_split(torch.stack([zq[..., 0] ** 2, zq[..., 1] ** 2, zq[..., 0] * zq[..., 1]], 2)))
    bound = 4 * (1 - rho ** 2) / math.sqrt(float(ess2.min()))
    print(f"correlation: {got_rho:.4f} against {rho:.4f}, ESS of the second moments {ess2.tolist()}, four standard errors {bound:.4f}")
    assert abs(got_rho - rho) < bound, (got_rho, rho, ess2)


# ------------------------------------------------------------------ 7. incomplete records
def test_incomplete_records_are_sampled():
    """B = 4, T = 13; GE is observed nowhere, insulin not at patient 0, and the same entries of initial_state are NaN: without
    the prior over (I, GE) no chain could solve these records.  The untrained model's output layer is zero (asserted), so nothing
    depends on GE: x0_GE of every patient recovers its prior (mean within 5 MCSE, sd within 10 %).  x0_I of the patients whose
    insulin is observed is narrower than its prior."""
    from inference import InitialStatePrior
    from inference.hmc import _ess, _split, run_hmc
    m = _model()
    last = [mod for mod in m.nn_residual.modules() if isinstance(mod, torch.nn.Linear)][-1]
    assert float(last.weight.abs().max()) == 0.0 and float(last.bias.abs().max()) == 0.0
    B, T = 4, 13
    data = _data(m, B=B, T=T, sigma=0.05)
    obs, x0 = data["observations"].clone(), data["initial_state"].clone()
    obs[:, :, 4] = float("nan")
    obs[0, :, 1] = float("nan")
    x0[:, 4] = float("nan")
    x0[0, 1] = float("nan")
    data = dict(data, observations=obs, initial_state=x0)
    mean, sd = np.array(MEAN), np.array([1.0, 5.0, 8.0, 1.0, 0.1, 0.05])
    prior = InitialStatePrior(mean, sd, states=("I", "GE"))
    r = run_hmc(m, data, num_samples=200, num_warmup=150, n_chains=64, n_leapfrog=8, noise_sigma=0.05, ode_priors={"a_GI": (0.0104, 0.002)},
                sample_nn=False, initial_state=prior, seed=4)
    assert int(r.stats["failed_solve"].sum()) == 0 and int(r.stats["divergent"].sum()) == 0
    xs = r.initial_states()
    assert tuple(xs.shape) == (64, 200, B, 6) and bool(torch.isfinite(xs).all())
    ge = xs[..., 4]
    flat = ge.reshape(-1, B)
    mcse = flat.std(0) / _ess(_split(ge)).sqrt()
    print(f"\nx0_GE: mean {flat.mean(0).tolist()}, sd {flat.std(0).tolist()}, mcse {mcse.tolist()}; x0_I sd {xs[..., 1].reshape(-1, B).std(0).tolist()}")
    assert float(((flat.mean(0) - mean[4]).abs() / mcse).max()) < 5
    assert float((flat.std(0) / sd[4] - 1).abs().max()) < 0.10
    assert bool((xs[..., 1].reshape(-1, B).std(0)[1:] < sd[1]).all())
    summ = r.summary()
    assert list(summ) == ["ode.a_GI", "x0.I", "x0.GE"] and summ["x0.GE"]["mean"].shape == (B,) and summ["ode.a_GI"]["q975"].shape == ()
    assert all(np.all(np.isfinite(v)) for d in summ.values() for v in d.values())
    t2 = torch.linspace(0.0, 4.0, 2 * T - 1, device=DEV)
    pred = r.predict(t_span=t2, thin=10)
    assert tuple(pred.shape) == (64 * 20, B, 2 * T - 1, 6) and bool(torch.isfinite(pred).all())
    # every draw starts from its own x0
    torch.testing.assert_close(pred[:, :, 0].double().cpu(), xs[:, ::10].reshape(-1, B, 6).cpu(), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------ 8. run properties
def _run(sampler, m, data, **kw):
    from inference.hmc import run_hmc
    from inference.nuts import run_nuts
    if sampler == "hmc":
        kw.pop("max_tree_depth", None)
        return run_hmc(m, data, sample_nn=False, **kw)
    kw.pop("n_leapfrog", None)
    return run_nuts(m, data, sample_nn=False, **kw)


@pytest.mark.parametrize("sampler", ["hmc", "nuts"])
def test_same_seed_same_draws(sampler):
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    kw = dict(num_samples=10, num_warmup=20, n_chains=32, n_leapfrog=4, max_tree_depth=6, noise_sigma=0.5, seed=9,
              initial_state=_prior(("G", "I"), "log"))
    a, b = _run(sampler, m, data, **kw), _run(sampler, m, data, **kw)
    assert torch.equal(a.draws, b.draws) and torch.equal(a.raw, b.raw) and tuple(a.draws.shape) == (32, 10, 7 + 4 * 2)
    keys = ["accept_prob", "log_posterior", "divergent", "failed_solve", "step_size", "inv_mass"]
    keys += ["tree_depth", "n_leapfrog", "trajectories_solved"] if sampler == "nuts" else []
    for k in keys:
        assert np.array_equal(a.stats[k], b.stats[k]), k


def test_hmc_chains_do_not_depend_on_the_chain_count():
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    kw = dict(num_samples=20, num_warmup=0, n_leapfrog=4, noise_sigma=0.5, seed=1, initial_state=_prior(("G", "I")))
    r8, r4 = _run("hmc", m, data, n_chains=8, **kw), _run("hmc", m, data, n_chains=4, **kw)
    torch.testing.assert_close(r4.raw, r8.raw[:4], rtol=1e-5, atol=1e-6)
    assert np.array_equal(r4.stats["failed_solve"], r8.stats["failed_solve"][:4])


def test_nuts_chains_do_not_depend_on_the_chain_count():
    """tests/test_nuts_gpu.py's setting: fp64, num_warmup < 20 (per-chain step-size adaptation only, no pooled mass matrix), so
    every chain is on its own; trees of different sizes make the compacted active sets differ between the two runs."""
    m = _model(16, 2)
    data = _data(m, B=3, T=9, sigma=0.3)
    # a prior about as wide as what the data say (sd 0.1 around the batch's values, sigma = 0.3 on 9 points): the coordinates are
    # of order one without a mass matrix, so the trees end at different depths
    from inference import InitialStatePrior
    prior = InitialStatePrior(data["initial_state"].cpu().double(), torch.full((3, 6), 0.1, dtype=torch.float64), states=("G", "I"))
    kw = dict(num_samples=12, num_warmup=10, noise_sigma=0.3, seed=4, max_tree_depth=5, dtype=torch.float64, initial_state=prior,
              ode_priors={})                 # the states alone: constants that the data pin would need a mass matrix
    r16, r8 = _run("nuts", m, data, n_chains=16, **kw), _run("nuts", m, data, n_chains=8, **kw)
    assert np.array_equal(r16.stats["tree_depth"][:8], r8.stats["tree_depth"])
    assert np.array_equal(r16.stats["n_leapfrog"][:8], r8.stats["n_leapfrog"])
    torch.testing.assert_close(r16.raw[:8], r8.raw, rtol=0, atol=1e-10)
    assert len(set(r16.stats["n_leapfrog"].reshape(-1).tolist())) > 1


def test_a_prior_that_reaches_a_pole_is_rejected_and_counted():
    from inference import InitialStatePrior
    from inference.hmc import run_hmc
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    # G(0) ~ N(8, 20^2) reaches the pole of the GLP-1 production V_max G / (K_m + G) at G = -K_m = -7: dG/dt is about -0.23 per
    # minute there (I ~ 90), so a trajectory that starts in (-7, -6.5) crosses the pole inside the window of 2 minutes and the
    # solve reports status 2 / 3.  noise_sigma = 100 lets the prior dominate (13 points of G: the likelihood alone has sd 28), so
    # the posterior density of G(0) at -7 is about 0.016 per unit: about 3 % of the evaluations of a chain (4 patients) fail
    prior = InitialStatePrior(MEAN, [20.0, 9.0, 8.0, 1.0, 0.1, 0.05], states=("G",))
    r = run_hmc(m, data, num_samples=40, num_warmup=0, n_chains=16, n_leapfrog=4, noise_sigma=100.0, ode_priors={}, sample_nn=False,
                initial_state=prior, seed=1)
    st = r.stats
    print(f"\nfailed solves: {int(st['failed_solve'].sum())} of {st['failed_solve'].size}")
    assert int(st["failed_solve"].sum()) > 0
    assert bool(st["divergent"][st["failed_solve"]].all()) and float(np.abs(st["accept_prob"][st["failed_solve"]]).max()) == 0.0
    assert bool(torch.isfinite(r.draws).all()) and np.isfinite(st["log_posterior"]).all()


def _fold_by_hand(pred, batch):
    from inference import predictive as PR
    B, T = pred.shape[1], pred.shape[2]
    acc = PR.PredictiveAccumulator(B, T, batch.get("observations"), batch.get("observation_mask"), torch.float32)
    acc.fold(pred.to(DEV).contiguous())
    return acc.finish(10)


def _same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def test_predictive_summary_equals_folding_predict_by_hand():
    m = _model()
    data = _data(m, B=4, T=13, sigma=0.5)
    r = _run("hmc", m, data, num_samples=6, num_warmup=4, n_chains=4, n_leapfrog=2, noise_sigma=0.5, seed=2, initial_state=_prior(("G", "I")))
    pred = r.predict()
    assert tuple(pred.shape) == (24, 4, 13, 6)
    assert not torch.equal(pred[0, :, 0], pred[1, :, 0])                 # the draws' own initial states, not the batch's
    for kw in (dict(), dict(max_bytes=5 * 4 * 13 * 6 * 4)):
        got, want = r.predictive_summary(observation_noise=False, **kw), _fold_by_hand(pred, data)
        assert torch.equal(got.mean, want.mean) and _same(got.std, want.std) and _same(got.pit, want.pit)
    # another batch: the current path, the batch's initial states under every draw
    other = dict(data, initial_state=data["initial_state"] * 1.01)
    got = r.predictive_summary(other, observation_noise=False)
    want = _fold_by_hand(r.predict(other["initial_state"], other["time_points"]), other)
    assert torch.equal(got.mean, want.mean)


def test_run_population_with_initial_states_end_to_end_on_4gi_batch():
    from hode.datagen import FourGIModel, GlucoseDataset
    from inference import InitialStatePrior
    from inference.population import run_population
    gen = torch.Generator(device=DEV).manual_seed(0)
    table, status = FourGIModel("T2DM").generate_cohort(32, duration_hours=5, sampling_interval_min=5, meal_times=(0.5, 2.5),
                                                        meal_sizes=(75, 50), noise_cv=0.1, generator=gen)
    ds = GlucoseDataset(table, sequence_length=61, stride=61)
    batch = ds.batch(torch.arange(32))
    prior = InitialStatePrior.from_batch(batch, states=("G", "I"), inflate=2.0)
    m = _model()
    for sampler in ("hmc", "nuts"):
        r = run_population(m, batch, num_samples=4, num_warmup=4, n_chains=4, n_leapfrog=2, max_tree_depth=3, seed=2, sampler=sampler,
                           initial_state=prior)
        names = ["a_GI", "k_I", "rho", "E_max", "V_max", "K_m", "k_L"]
        assert r.names == names and tuple(r.draws.shape) == (4, 4, 7 * 34 + 32 * 2)
        xs = r.initial_states()
        assert tuple(xs.shape) == (4, 4, 32, 6) and bool(torch.isfinite(xs).all())
        assert torch.equal(xs[..., [2, 3, 4, 5]], batch["initial_state"].double()[:, [2, 3, 4, 5]].expand(4, 4, 32, 4))
        s, summ = r.samples, r.summary()
        assert list(s)[-2:] == ["x0.G", "x0.I"] and s["x0.I"].shape == (4, 4, 32) and list(summ) == list(s)
        assert all(np.all(np.isfinite(v)) for d in summ.values() for v in d.values())
        assert int(r.stats["failed_solve"].sum()) == 0
    pred = r.predict()
    assert tuple(pred.shape) == (16, 32, 61, 6) and bool(torch.isfinite(pred).all())
    torch.testing.assert_close(pred[:, :, 0].double().cpu(), xs.reshape(16, 32, 6).cpu(), rtol=1e-6, atol=1e-6)
    whole, want = r.predictive_summary(), _fold_by_hand(pred, batch)
    assert torch.equal(whole.mean, want.mean)
    cut = r.predictive_summary(max_bytes=3 * 32 * 61 * 6 * 4)
    assert torch.equal(cut.mean, whole.mean) and _same(cut.std, whole.std)
