"""The unscented Kalman filter's step kernel (csrc/hode_ukf.hip) and inference.run_ukf on the GPU, held to the numpy restatement
of tests/_ukf_reference.py.  `-m gpu`.

Tolerances against the restatement, per patient:
  mean, cov, stats   within 64 n c 2^-52 of the largest magnitude in the same array, c the larger condition number of the case's
                     P- (on its non-zero columns) and S from the restatement (tests/test_ukf_host.py keeps c <= 1e6);
  x_out, aux_out     fp64: the same bound, relative, entry by entry; fp32: one ulp of fp32 (another libm's exp may flip the one
                     rounding); carried columns bit for bit;
  a lost patient     exact flags and NaN / -inf pattern, its rows copied bit for bit.
Every comparison prints `UKF_FRACTION <what> <worst error / bound>`."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

import _ukf_cases as UC  # noqa: E402
import _ukf_reference as UR  # noqa: E402

DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}
bits = lambda v: np.ascontiguousarray(v).view(np.uint8)                                 # noqa: E731  (NaN and -0 included)


def _bound(n, cond):
    return 64 * n * cond * 2.0 ** -52


def _run_case(c, dtype, sel=None):
    """The kernel on the case `c` (all patients, or patient `sel` alone) -> dict of numpy arrays."""
    pick = (lambda a: a) if sel is None else (lambda a: a[sel:sel + 1])
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(pick(a)), dtype=dt, device=DEV)  # noqa: E731
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)                     # noqa: E731
    alive, mean, cov = dev(c["alive"], torch.int32), dev(c["mean"], torch.float64), dev(c["cov"], torch.float64)
    x_out, aux_out, stats = hode.capi.ukf_step(
        dev(c["x_in"], dtype), dev(c["aux_in"], dtype), c["mode"], dev(c["obs"], dtype), f64(c["sigma"]), f64(c["q"]), f64(c["walk"]),
        f64(pick(c["dt"])), alive, mean, cov, c["w"], predict=bool(c["predict"]), link=c["link"], status=dev(c["status"], torch.int32),
        mask=dev(c["mask"], torch.uint8))
    torch.cuda.synchronize()
    return {"x_out": x_out.cpu().numpy(), "aux_out": aux_out.cpu().numpy(), "stats": stats.cpu().numpy(), "alive": alive.cpu().numpy(),
            "mean": mean.cpu().numpy(), "cov": cov.cpu().numpy()}


def _check_patient(got, b, ref, c, dtype, what):
    """One patient of a kernel result against the restatement; returns the worst error / bound."""
    n = c["n"]
    assert int(got["alive"][b]) == ref["alive"], what
    if not ref["alive"]:
        st = got["stats"][b]
        assert st[0] == -math.inf and st[2] == ref["stats"][2] and st[3] == 0 and np.isnan(st[[1] + list(range(4, 16))]).all(), what
        assert np.isnan(got["mean"][b]).all() and np.isnan(got["cov"][b]).all(), what
        assert np.array_equal(bits(got["x_out"][b]), bits(c["x_in"][b].astype(NP[dtype]))), what + ": x_out is not x_in"
        assert np.array_equal(bits(got["aux_out"][b]), bits(c["aux_in"][b].astype(NP[dtype]))), what + ": aux_out is not aux_in"
        return 0.0
    bound = _bound(n, ref["cond"])
    worst = 0.0
    for name in ("mean", "cov", "stats"):
        err = np.abs(got[name][b] - ref[name]).max() / np.abs(ref[name]).max() if np.abs(ref[name]).max() > 0 else np.abs(got[name][b]).max()
        worst = max(worst, err / bound)
        assert err <= bound, f"{what} {name}: {err:.3e} > {bound:.3e}"
    assert got["stats"][b][2] == ref["stats"][2] and got["stats"][b][3] == 1.0, what
    cols, _ = UR.columns(c["mode"])
    carried = [j for j in range(17) if j not in cols]
    assert np.array_equal(got["aux_out"][b][:, carried], np.tile(c["aux_in"][b][0, carried], (c["K"], 1)).astype(NP[dtype])), what + " carried"
    for name, g, r in (("x_out", got["x_out"][b], ref["x_out"]), ("aux_out", got["aux_out"][b][:, cols], ref["aux_out"][:, cols])):
        if dtype == torch.float64:
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.where(r == g, 0.0, np.abs(g - r) / np.abs(r)).max() if r.size else 0.0
            worst = max(worst, err / bound)
            assert err <= bound, f"{what} {name}: {err:.3e} > {bound:.3e}"
        else:
            want = r.astype(np.float32)
            assert (np.abs(g.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), f"{what} {name}"
    return worst


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", range(len(UC.SPECS)), ids=[UC.case_id(s) for s in UC.SPECS])
def test_step_kernel_against_the_restatement(idx, dtype):
    c, refs = UC.case(idx), UC.reference(idx)
    got = _run_case(c, dtype)
    worst = 0.0
    for b, ref in enumerate(refs):
        worst = max(worst, _check_patient(got, b, ref, c, dtype, f"case {UC.case_id(UC.SPECS[idx])} patient {b}"))
        if ref["alive"] and ref["stats"][2] == 0:                        # nothing seen: exactly no evidence
            assert got["stats"][b][0] == 0.0 and got["stats"][b][1] == 0.0
            if not c["predict"]:                                         # and the given moments come back bit for bit
                assert np.array_equal(bits(got["mean"][b]), bits(c["mean"][b])) and np.array_equal(bits(got["cov"][b]), bits(c["cov"][b]))
    print(f"UKF_FRACTION kernel-{UC.case_id(UC.SPECS[idx])}-{NP[dtype].__name__} {worst:.4f}")
    edge = UC.SPECS[idx].get("edge")
    if edge == "zero_cov":
        assert (got["x_out"] == got["x_out"][:, :1]).all() and (got["aux_out"] == got["aux_out"][:, :1]).all() and not got["cov"].any()
    if edge == "zero_state":
        assert (got["x_out"][:, :, 2] == 1.0).all() and not got["cov"][:, 2].any() and not got["cov"][:, :, 2].any()
    if edge == "zero_given":
        assert (got["x_out"][:, :, 2] == got["x_out"][:, :1, 2]).all() and not got["cov"][:, 2].any()


_DET = [i for i, s in enumerate(UC.SPECS) if s["B"] == 3 and (s["P"] == 17 or s.get("edge") in ("lost_status", "zero_given")
                                                              or (s["P"] == 2 and s["mask"] in ("mixed", "none")))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", _DET, ids=[UC.case_id(UC.SPECS[i]) for i in _DET])
def test_step_kernel_is_deterministic_and_independent_of_the_batch(idx, dtype):
    """The same call twice gives the same bits; patient 2 of B = 3 gives the bits of that patient alone."""
    c = UC.case(idx)
    a, b = _run_case(c, dtype), _run_case(c, dtype)
    alone = _run_case(c, dtype, sel=2)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
        assert np.array_equal(bits(a[k][2:3]), bits(alone[k])), k


def test_capi_rejects_what_the_kernel_cannot_take():
    c = UC.case(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=DEV)                                                     # noqa: E731
    base = dict(x_in=t(c["x_in"], torch.float32), aux_in=t(c["aux_in"], torch.float32), mode=c["mode"], obs=t(c["obs"], torch.float32),
                sigma=t(c["sigma"], torch.float64), q=t(c["q"], torch.float64), walk=t(c["walk"], torch.float64),
                dt=t(c["dt"], torch.float64), alive=t(c["alive"], torch.int32), mean=t(c["mean"], torch.float64),
                cov=t(c["cov"], torch.float64), weights=c["w"])
    bad_mode = c["mode"].copy()
    bad_mode[5] = 3
    for change in (dict(x_in=base["x_in"][:, :-1].contiguous()), dict(aux_in=base["aux_in"].double()), dict(mode=bad_mode),
                   dict(mode=UC.mode_of(1)), dict(sigma=base["sigma"].float()), dict(walk=base["walk"][:6].contiguous()),
                   dict(alive=base["alive"].long()), dict(mean=base["mean"][:, :5].contiguous()), dict(cov=base["cov"].cpu()),
                   dict(out=(base["x_in"], torch.empty_like(base["aux_in"]), torch.empty(1, 16, dtype=torch.float64, device=DEV)))):
        with pytest.raises(hode.capi.HodeError):
            hode.capi.ukf_step(**dict(base, **change))


# ------------------------------------------------------------------ 2. a linear model on the device is a Kalman filter
@pytest.mark.parametrize("which", [1, 2])
def test_identity_link_on_the_device_reproduces_the_kalman_filter(which):
    """x_in = A chi_x + Bm chi_theta formed in torch (fp64) from the kernel's own x_out / aux_out, step after step."""
    M = UC.linear_model(which)
    w = hode.capi.ukf_weights(M["n"])
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)                     # noqa: E731
    A, Bm, sigma, q, walk = f64(M["A"]), f64(M["Bm"]), f64(M["sigma"]), f64(M["q"]), f64(M["walk"])
    K, cols = 2 * M["n"] + 1, M["cols"]
    x, aux = torch.zeros(1, K, 6, dtype=torch.float64, device=DEV), torch.ones(1, K, 17, dtype=torch.float64, device=DEV)
    mean, cov, alive = f64(M["m0"][None]), f64(M["P0"][None]), torch.ones(1, dtype=torch.int32, device=DEV)
    worst = [0.0, 0.0, 0.0]
    for s, (e0, m0, P0) in enumerate(UC.kalman(M)):
        if s > 0:
            x = (x @ A.T + aux[:, :, cols] @ Bm.T).contiguous()
        x, aux, stats = hode.capi.ukf_step(x, aux, M["mode"], f64(M["ys"][s][None]), sigma, q, walk, f64(M["dts"][s:s + 1]), alive, mean, cov,
                                           w, predict=s > 0, link=0)
        worst = [max(worst[0], abs(e0 - float(stats[0, 0]))), max(worst[1], np.abs(m0 - mean[0].cpu().numpy()).max()),
                 max(worst[2], np.abs(P0 - cov[0].cpu().numpy()).max())]
        assert int(alive[0]) == 1 and (not np.isfinite(M["ys"][s]).any()) == (float(stats[0, 0]) == 0.0)
    print(f"model {which} on the device: evidence {worst[0]:.2e}, mean {worst[1]:.2e}, covariance {worst[2]:.2e}")
    assert max(worst) <= 1e-10


# ------------------------------------------------------------------ 3. run_ukf end to end
B, T = 3, 13
X0 = [8.0, 90.0, 80.0, 10.0, 0.3, 0.5]                              # (every state positive: the log link has no zero)
LINKS = {"relu64x4": "log", "tanh32x2": "additive"}


def _model(kind):
    import models as M
    torch.manual_seed(3)
    if kind == "relu64x4":
        m = M.HybridODENN(nn_hidden=64, nn_layers=4, device=DEV)
    else:
        m = M.HybridODENN(nn_hidden=32, nn_layers=2, device=DEV)
        m.nn_residual = M.NNResidual(9, 32, 6, 2, activation="tanh").cuda()
    with torch.no_grad():
        for p in m.nn_residual.parameters():
            p.normal_(0.0, 0.05)                                   # (the output layer starts at zero: make the network matter)
    return m


def _data(model, x0=X0, sigma_rel=0.05, seed=1, missing=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.tensor(x0, device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
    t = torch.linspace(0.0, 2.0, T, device=DEV)
    meal = torch.zeros(B, T, device=DEV)
    meal[:, 2:5] = torch.tensor([20.0, 40.0, 10.0], device=DEV)
    with torch.no_grad():
        y = model.forward(x0, t, {"meal": meal})
    scale = y.abs().mean((0, 1)) + 0.1
    obs = y + sigma_rel * scale * torch.randn(y.shape, device=DEV, generator=g)
    if missing:
        obs[:, 3] = float("nan")                                   # a grid point nobody observes: no filter step there
        obs[1, 5, :] = float("nan")                                # one patient unobserved at a step
        obs[:, 7, 0] = float("nan")                                # one state seen (the second)
        obs[:, 7, 2:] = float("nan")
    return {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {"meal": meal}}, (sigma_rel * scale).double().cpu().numpy(), y


@pytest.fixture(scope="module", params=["relu64x4", "tanh32x2"])
def setup(request):
    m = _model(request.param)
    data, sigma, truth = _data(m)
    scale = (truth.abs().mean((0, 1)) + 0.1).double().cpu().numpy()
    link = LINKS[request.param]
    rel = 1.0 if link == "log" else scale                              # additive noise in the states' own units
    return m, data, sigma, link, rel


def test_run_ukf_equals_a_loop_of_segment_solves_and_restated_steps(setup):
    """Every step of run_ukf against model.forward over the segment from the sigma points the step before emitted (run_ukf's own,
    store_history=True) plus the restatement's step -- each step is held to the kernel tolerances, not to their compound."""
    from inference import run_ukf
    model, data, sigma, link, rel = setup
    q, q0 = 0.04 * rel * np.ones(6), 0.1 * rel * np.ones(6)
    res = run_ukf(model, data, process_noise=q, initial_spread=q0, noise_sigma=sigma, noise_link=link, store_history=True)
    idxs = res.step_index.tolist()
    assert idxs == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12]          # row 3 is unobserved: no step there
    assert res.alive.all() and torch.isfinite(res.log_evidence()).all()
    t, meal, obs = data["time_points"], data["external_inputs"]["meal"], data["observations"].cpu().numpy().astype(np.float64)
    w, mode, K, lk = hode.capi.ukf_weights(6), np.zeros(17, dtype=np.int32), 13, UR.LINK[link]
    x0 = data["initial_state"].double().cpu().numpy()
    ode = model.ode_core.param_vector().float().cpu().numpy().astype(np.float64)
    hist, odeh = res.history.cpu().numpy(), res.ode_history.cpu().numpy()
    meanh, covh = res.mean_history.cpu().numpy(), res.cov_history.cpu().numpy()
    stats = np.concatenate([torch.stack([res.log_evidence_steps, res.nis, res.n_seen.double(), res.alive.double()], 2).cpu().numpy(),
                            res.mean.cpu().numpy(), res.std.cpu().numpy() ** 2], 2)                        # [B, S, 16]
    worst = 0.0
    for s, g in enumerate(idxs):
        if s == 0:
            x_in, status, dt = np.repeat(x0[:, None], K, 1), np.zeros((B, K), np.int32), np.ones(B)
            mean, cov = np.log(x0) - 0.5 * q0 * q0 if lk else x0, np.tile(np.diag(q0 * q0), (B, 1, 1))
            aux_in = np.tile(ode, (B, K, 1))
        else:
            p = idxs[s - 1]
            with torch.no_grad():
                y = model.forward(res.history[s - 1].reshape(B * K, 6), t[p:g + 1], {"meal": meal[:, p:g + 1].repeat_interleave(K, 0)})
            x_in = y[:, -1].reshape(B, K, 6).cpu().numpy().astype(np.float64)
            status = model.last_solve_info["status"].view(B, K).cpu().numpy()
            dt = np.full(B, float(t[g].double() - t[p].double()))
            mean, cov, aux_in = meanh[s - 1], covh[s - 1], odeh[s - 1].astype(np.float64)
        c = {"n": 6, "K": K, "mode": mode, "x_in": x_in, "aux_in": aux_in}
        # (the result holds the standard deviation: its square carries the roundings of the root and of the square, far inside
        # the bound, which is at least 64 * 6 * 2^-52)
        got = {"alive": res.alive[:, s].int().cpu().numpy(), "mean": meanh[s], "cov": covh[s], "x_out": hist[s], "aux_out": odeh[s],
               "stats": stats[:, s]}
        for b in range(B):
            ref = UR.step(x_in[b], aux_in[b], mode, obs[b, g], sigma, q, np.zeros(17), dt[b], 1, mean[b], cov[b], w, predict=s > 0, link=lk,
                          status=status[b])
            worst = max(worst, _check_patient(got, b, ref, c, torch.float32, f"step {s} (grid {g}) patient {b}"))
    print(f"UKF_FRACTION run_ukf-{link} {worst:.4f}")
    assert torch.equal(res.times, t[res.step_index]) and res.sigma_points.shape == (B, K, 6) and res.ode_p.shape == (B, K, 17)
    assert torch.equal(res.sigma_points, res.history[-1]) and torch.equal(res.ode_p, res.ode_history[-1])
    assert torch.equal(res.state_mean, res.mean_history[-1]) and torch.equal(res.state_cov, res.cov_history[-1])
    assert res.learned is None and res.n_seen[1, idxs.index(5)] == 0 and res.log_evidence_steps[1, idxs.index(5)] == 0
    assert (res.n_seen[:, idxs.index(7)] == 1).all()
    plain = run_ukf(model, data, process_noise=q, initial_spread=q0, noise_sigma=sigma, noise_link=link)
    assert plain.history is None and torch.equal(plain.sigma_points, res.sigma_points) and torch.equal(plain.state_cov, res.state_cov)


def test_without_noise_the_evidence_is_the_gaussian_log_likelihood(setup):
    """process_noise = 0 and initial_spread = 0: the covariance is zero throughout, all K sigma points are the deterministic
    trajectory, S = diag(sigma^2), and the evidence is the Gaussian log-likelihood of the segment solves, -(sum z^2 +
    sum log sigma^2 + d log 2 pi) / 2 -- to 8 * 2^-52 = 1.8e-15 relative per step.
    The additive link with kappa = 2: n + kappa = 8 makes the weights 1/4 and 1/16, so the unscented mean of K equal fp32 values
    is that value exactly.  (Under the log link the mean of K equal points is exp(sum w log x), which is x only up to the
    rounding of the logarithm, some ulps of x; against a residual of a few per cent of x that alone is tens of ulps of z^2.)"""
    from inference import run_ukf
    model, data, sigma, _, _ = setup
    res = run_ukf(model, data, process_noise=0.0, initial_spread=0.0, noise_sigma=sigma, noise_link="additive", kappa=2.0)
    assert res.alive.all() and (res.sigma_points == res.sigma_points[:, :1]).all() and (res.std == 0).all() and not res.state_cov.any()
    t, meal, obs = data["time_points"], data["external_inputs"]["meal"], data["observations"].double().cpu().numpy()
    idxs = res.step_index.tolist()
    x = data["initial_state"]
    want = np.zeros((B, len(idxs)))
    for s, g in enumerate(idxs):
        if s > 0:
            p = idxs[s - 1]
            with torch.no_grad():
                x = model.forward(x, t[p:g + 1], {"meal": meal[:, p:g + 1]})[:, -1]
        xs = x.double().cpu().numpy()
        for b in range(B):
            nis, ld, d = 0.0, 0.0, 0
            for j in range(6):
                if math.isfinite(obs[b, g, j]):
                    z = (obs[b, g, j] - xs[b, j]) / sigma[j]
                    nis, ld, d = nis + z * z, ld + math.log(sigma[j]), d + 1
            want[b, s] = -0.5 * ((nis + 2.0 * ld) + d * UR.LOG_2PI) if d else 0.0
    assert torch.equal(res.sigma_points[:, 0], x)
    got = res.log_evidence_steps.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want == got, 0.0, np.abs(got - want) / np.abs(want))
    print("max relative |evidence - log-likelihood| per step", rel.max(), "in units of 2^-52:", rel.max() * 2.0 ** 52)
    np.testing.assert_allclose(got, want, rtol=8 * 2.0 ** -52, atol=0.0)
    np.testing.assert_allclose(res.log_evidence().cpu().numpy(), want.sum(1), rtol=8 * 2.0 ** -52, atol=0.0)


def test_forecast_equals_a_run_with_trailing_nan_rows(setup):
    """Bit for bit, a learned constant that walks included."""
    from inference import ParameterLearning, run_ukf
    model, data, sigma, link, rel = setup
    cut = 9
    obs = data["observations"].clone()
    obs[:, cut:] = float("nan")
    kw = dict(process_noise=0.04 * rel, initial_spread=0.1 * rel, noise_sigma=sigma, noise_link=link,
              learn=ParameterLearning(["k_I", "a_GI"], walk=[0.1, 0.0], initial_spread=0.2))
    full = run_ukf(model, dict(data, observations=obs), **kw)
    meal = data["external_inputs"]["meal"]
    head = run_ukf(model, dict(data, observations=obs[:, :cut], time_points=data["time_points"][:cut],
                               external_inputs={"meal": meal[:, :cut]}), **kw)
    tail = head.forecast(data["time_points"][cut - 1:], {"meal": meal[:, cut - 1:]})
    assert full.step_index.tolist() == head.step_index.tolist() + [T - 1] and tail.step_index.tolist() == [T - cut]
    assert full.alive.all()
    tb = lambda v: v.cpu().numpy().tobytes()                                                                # noqa: E731
    for name in ("sigma_points", "ode_p", "state_mean", "state_cov"):
        assert tb(getattr(full, name)) == tb(getattr(tail, name)), name
    for name in ("mean", "std", "nis", "n_seen", "log_evidence_steps", "alive"):
        assert tb(getattr(full, name)[:, -1:]) == tb(getattr(tail, name)), name
        assert tb(getattr(full, name)[:, :-1]) == tb(getattr(head, name)), name
    for name in ("location", "scale"):
        assert tb(getattr(full.learned, name)[:, -1:]) == tb(getattr(tail.learned, name)), name
    assert (tail.log_evidence_steps == 0).all()                     # nothing observed: no evidence
    # names keep the caller's order (k_I's column is not the smaller one): the walking constant's band widens, the other's does not
    assert full.learned.names == ["k_I", "a_GI"]
    assert (tail.learned.scale[:, -1, 0] > 1.01 * head.learned.scale[:, -1, 0]).all()
    np.testing.assert_allclose(tail.learned.scale[:, -1, 1].cpu().numpy(), head.learned.scale[:, -1, 1].cpu().numpy(), rtol=1e-6)
    rank = np.argsort(np.argsort(kw["learn"].columns))
    assert torch.equal(full.learned.location[:, -1], full.state_mean[:, torch.as_tensor(6 + rank, device=DEV)])
    assert full.sigma_points.shape == (B, 17, 6) and full.state_mean.shape == (B, 8)


def test_run_ukf_fp64_and_per_patient_grids_agree_with_fp32_shared(setup):
    """The fp64 path and a per-patient [B, T] grid run the same loop.  The same grid per patient gives the shared grid's numbers
    up to the solver's treatment of the grid (1e-5, as for run_filter); fp64 against fp32 differs by the fp32 solve: adaptive
    steps taken at rtol 1e-6 in another arithmetic, some 1e-5 relative over twelve segments, contracted by the updates --
    2e-4 relative, and as much of the observation noise for states near zero."""
    from inference import run_ukf
    model, data, sigma, link, rel = setup
    kw = dict(process_noise=0.04 * rel, initial_spread=0.1 * rel, noise_sigma=sigma, noise_link=link)
    a = run_ukf(model, data, **kw)
    b = run_ukf(model, dict(data, time_points=data["time_points"].expand(B, T).contiguous()), **kw)
    c = run_ukf(model, data, dtype=torch.float64, **kw)
    assert b.times.shape == (B, len(a.step_index))
    np.testing.assert_allclose(b.mean.cpu().numpy(), a.mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(c.mean.cpu().numpy(), a.mean.cpu().numpy(), rtol=2e-4, atol=2e-4 * float(sigma.max()))
    assert c.sigma_points.dtype == torch.float64 and torch.isfinite(c.log_evidence()).all() and c.alive.all()


# ------------------------------------------------------------------ 4. what it is for
def test_a_wrong_constant_is_learned_from_the_record():
    """Records simulated by the model with V_max (the GLP-1 secretion capacity) at 1.25 times the model's value -- the model's is
    20 % off --, all six states observed, T = 25.  `learn` on V_max starts from the model's value with an initial spread of 0.5
    in the logarithm: the final 90 % interval contains the generating value in all 3 patients, and its scale has shrunk."""
    from inference import ParameterLearning, run_ukf
    model = _model("relu64x4")
    g = torch.Generator(device=DEV).manual_seed(4)
    Tn, name, factor, spread = 25, "V_max", 1.25, 0.5
    x0 = torch.tensor([8.0, 90.0, 80.0, 10.0, 0.0, 0.5], device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
    t = torch.linspace(0.0, 4.0, Tn, device=DEV)
    meal = torch.zeros(B, Tn, device=DEV)
    meal[:, 2:5] = torch.tensor([20.0, 40.0, 10.0], device=DEV)
    start = float(getattr(model.ode_core, name))
    with torch.no_grad():
        y = model.forward_ode_sets({name: torch.tensor([factor * start])}, x0, t, {"meal": meal})[0]
    scale = y.abs().mean((0, 1)) + 0.1
    sigma = (0.02 * scale).double().cpu().numpy()
    obs = y + 0.02 * scale * torch.randn(y.shape, device=DEV, generator=g)
    data = {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {"meal": meal}}
    noise = 0.02 * scale.double().cpu().numpy()                       # additive (state 4 starts at exactly 0), in the states' own units
    res = run_ukf(model, data, process_noise=noise, initial_spread=noise, noise_sigma=sigma, noise_link="additive",
                  learn=ParameterLearning([name], initial_spread=spread))
    assert res.alive.all()
    lo, hi = res.learned.interval(0.9)
    med = res.learned.median()[:, -1, 0].cpu().numpy()
    print(f"{name}: truth {factor * start:.5f}, start {start:.5f}, final medians {med}, intervals "
          f"{lo[:, -1, 0].cpu().numpy()} .. {hi[:, -1, 0].cpu().numpy()}, scale {res.learned.scale[:, -1, 0].cpu().numpy()}")
    assert ((lo[:, -1, 0] <= factor * start) & (factor * start <= hi[:, -1, 0])).all()
    assert (res.learned.scale[:, -1, 0] < spread).all()
    assert res.learned.location.shape == (B, Tn, 1) and res.state_mean.shape == (B, 7)
    assert torch.equal(res.learned.location[:, -1, 0], res.state_mean[:, 6])


def test_the_filter_tracks_a_patient_whose_initial_glucose_is_wrong():
    """The data of the particle filter's tracking case (tests/test_filter_gpu.py): records from the model itself, 2 % noise, only
    glucose observed; the filter starts from a glucose x0 that is 30 % off.  Over the second half of the grid its filtered
    glucose mean is closer to the truth than the open-loop solve from that x0, and closer than the observation noise
    (sigma = 0.31).  The record's fifth state starts at exactly 0, which a Gaussian on the logarithm cannot hold, so the noise is
    additive here, 5 % of every state's typical size (none on the fifth)."""
    from inference import run_ukf
    model = _model("relu64x4")
    data, _, truth = _data(model, x0=[8.0, 90.0, 80.0, 10.0, 0.0, 0.5], missing=False)
    g = torch.Generator(device=DEV).manual_seed(9)
    sigma = np.full(6, 1.0)
    sigma[0] = 0.02 * float(truth[..., 0].mean())
    obs = torch.full_like(truth, float("nan"))
    obs[..., 0] = truth[..., 0] + sigma[0] * torch.randn(B, T, device=DEV, generator=g)
    wrong = data["initial_state"].clone()
    wrong[:, 0] *= 1.3
    with torch.no_grad():
        open_loop = model.forward(wrong, data["time_points"], data["external_inputs"])
    size = (truth.abs().mean((0, 1)) + 0.1).double().cpu().numpy()
    res = run_ukf(model, dict(data, initial_state=wrong, observations=obs), process_noise=0.05 * size * np.array([1, 1, 1, 1, 0, 1.0]),
                  initial_spread=np.array([0.3, 0.05, 0.05, 0.05, 0.0, 0.05]) * size, noise_sigma=sigma, noise_link="additive")
    assert res.step_index.tolist() == list(range(T)) and res.alive.all()
    half = slice(T // 2, T)
    rmse = lambda a: float(((a[:, half] - truth[:, half, 0].double()) ** 2).mean().sqrt())                 # noqa: E731
    e_filter, e_open = rmse(res.mean[..., 0]), rmse(open_loop[..., 0].double())
    print(f"glucose RMSE over the second half: filter {e_filter:.4f}, open loop {e_open:.4f}, sigma {sigma[0]:.4f}")
    assert torch.isfinite(res.log_evidence()).all()
    assert e_filter < e_open and e_filter < sigma[0]
