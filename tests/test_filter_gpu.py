"""The particle-filter step kernel (csrc/hode_filter.hip) and inference.run_filter on the GPU, held to the numpy restatement of
tests/_filter_reference.py.  `-m gpu`.

Tolerances against the restatement:
  anc          exactly equal: tests/test_filter_host.py shows that no case has a pointer within 8 summation errors of a boundary;
  stats, lw    rtol (N + 16) * 2^-52 against the restatement's math.fsum values: the worst-case bound of a positive fp64 sum of N
               terms plus the handful of roundings and libm calls around it;
  states       fp64 rtol 1e-14; fp32 one ulp of fp32 (the last bit of the double from another libm may flip the one rounding);
               a state without noise (q = 0) bit for bit."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

import _filter_cases as FC  # noqa: E402
import _filter_reference as FR  # noqa: E402

DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _rtol(N):
    return (N + 16) * 2.0 ** -52


def _run_case(d, dtype, sel=None, id0=None):
    """The kernel on case inputs `d` (all patients, or patient `sel` alone) -> dict of numpy arrays."""
    pick = (lambda a: a) if sel is None else (lambda a: a[sel:sel + 1])
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(pick(a)), dtype=dt, device=DEV)  # noqa: E731
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)                     # noqa: E731
    lw = dev(d["lw"], torch.float64)
    x_out, anc, stats, aux_out = hode.capi.pf_step(
        dev(d["x_in"], dtype), dev(d["obs"], dtype), f64(d["sigma"]), f64(d["q"]), f64(pick(d["dt"])), lw, d["step"], seed=d["seed"],
        id0=d["id0"] if id0 is None else id0, link=FR.LINK[d["link"]], ess_frac=d["ess_frac"], status=dev(d["status"], torch.int32),
        mask=dev(d["mask"], torch.uint8), aux_in=dev(d["aux"], dtype))
    torch.cuda.synchronize()
    return {"x_out": x_out.cpu().numpy(), "anc": anc.cpu().numpy(), "stats": stats.cpu().numpy(), "lw": lw.cpu().numpy(),
            "aux_out": None if aux_out is None else aux_out.cpu().numpy()}


def _check_states(got, want64, dtype, what):
    want = want64.astype(NP[dtype])
    if dtype == torch.float64:
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0.0, err_msg=what)
    else:
        ulp = np.spacing(np.abs(want))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), what


def _check_patient(got, b, ref, d, dtype, what):
    N = d["N"]
    assert np.array_equal(got["anc"][b], ref["anc"]), (what, np.nonzero(got["anc"][b] != ref["anc"])[0][:8])
    with np.errstate(invalid="ignore"):
        err = np.abs(got["stats"][b] - ref["stats"]) / np.abs(ref["stats"])
    print(what, "stats max rel err / bound", np.nanmax(np.where(np.isfinite(err), err, 0.0)) / _rtol(N))
    np.testing.assert_allclose(got["stats"][b], ref["stats"], rtol=_rtol(N), atol=0.0, equal_nan=True, err_msg=what + " stats")
    np.testing.assert_allclose(got["lw"][b], ref["lw"], rtol=_rtol(N), atol=0.0, err_msg=what + " lw")
    _check_states(got["x_out"][b], ref["x_out"], dtype, what + " states")
    quiet = np.nonzero(~(np.asarray(d["q"]) > 0))[0]                    # no noise: the input's bits, gathered
    assert np.array_equal(got["x_out"][b][:, quiet], d["x_in"][b][ref["anc"]][:, quiet].astype(NP[dtype])), what + " q = 0 states"
    if d["aux"] is not None:
        assert np.array_equal(got["aux_out"][b], ref["aux_out"].astype(NP[dtype])), what + " payload"


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", range(len(FC.CASES)), ids=[FC.case_id(c) for c in FC.CASES])
def test_step_kernel_against_the_restatement(idx, dtype):
    d, refs = FC.inputs(idx), FC.reference(idx)
    got = _run_case(d, dtype)
    for b, ref in enumerate(refs):
        _check_patient(got, b, ref, d, dtype, f"case {FC.case_id(d)} patient {b}")
    c = FC.CASES[idx]
    if c["edge"] == "patient_dead":                                # the dead patient: nothing resampled, its neighbours untouched
        assert got["stats"][1][0] == -np.inf and got["stats"][1][1] == 0 and np.isnan(got["stats"][1][4:]).all()
        assert np.isneginf(got["lw"][1]).all() and np.array_equal(got["anc"][1], np.arange(c["N"]))
    if c["edge"] == "one_heavy":
        assert (got["stats"][:, 1] == 1.0).all() and (got["anc"] == (2 * c["N"]) // 3).all()
    if c["mask"] == "patient_missing" and c["ess_frac"] == 0.0:   # an unobserved patient keeps its weights
        assert np.array_equal(got["lw"][c["B"] - 2], d["lw"][c["B"] - 2]) and got["stats"][c["B"] - 2][0] == 0.0


_DET = [c["idx"] for c in FC.CASES if c["B"] == 3 and c["N"] in (65, 257, 4096) and c["mask"] == "complete"][:10]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", _DET, ids=[FC.case_id(FC.CASES[i]) for i in _DET])
def test_step_kernel_is_deterministic_and_independent_of_the_batch(idx, dtype):
    """The same call twice gives the same bits; patient 2 of B = 3 gives the bits of that patient alone with id0 + 2."""
    d = FC.inputs(idx)
    a, b = _run_case(d, dtype), _run_case(d, dtype)
    alone = _run_case(d, dtype, sel=2, id0=d["id0"] + 2)
    for k in ("x_out", "anc", "stats", "lw", "aux_out"):
        if a[k] is None:
            continue
        bits = lambda v: np.ascontiguousarray(v).view(np.uint8)                        # noqa: E731  (NaN and -0 included)
        assert np.array_equal(bits(a[k]), bits(b[k])), k
        assert np.array_equal(bits(a[k][2:3]), bits(alone[k])), k


# ------------------------------------------------------------------ 2. run_filter end to end
B, N, T = 3, 128, 13
X0 = [8.0, 90.0, 80.0, 10.0, 0.0, 0.5]


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


def _data(model, sigma_rel=0.05, seed=1, missing=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.tensor(X0, device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
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
        obs[:, 7, 1:] = float("nan")                               # one state seen
    return {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {"meal": meal}}, (sigma_rel * scale).double().cpu().numpy(), y


@pytest.fixture(scope="module", params=["relu64x4", "tanh32x2"])
def setup(request):
    m = _model(request.param)
    data, sigma, truth = _data(m)
    return m, data, sigma, truth


def test_run_filter_equals_a_loop_of_segment_solves_and_restated_steps(setup):
    """(a) every step of run_filter against model.forward over the segment plus the restatement's step, fed with run_filter's own
    particles of the step before (so that each step is held to the kernel tolerances, not to their compound)."""
    from inference import run_filter
    model, data, sigma, _ = setup
    q, q0, seed = 0.04, 0.1, 5
    res = run_filter(model, data, n_particles=N, process_noise=q, initial_spread=q0, noise_sigma=sigma, ess_threshold=0.5, seed=seed,
                     store_particles=True)
    idxs = res.step_index.tolist()
    assert idxs == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12]          # row 3 is unobserved: no step there
    t, meal, obs = data["time_points"], data["external_inputs"]["meal"], data["observations"].cpu().numpy().astype(np.float64)
    hist, ancs, stats = res.history.cpu().numpy(), res.ancestors.cpu().numpy(), None
    lw = np.zeros((B, N))
    x_prev = data["initial_state"].reshape(B, 1, 6).repeat(1, N, 1)
    resampled = 0
    for s, g in enumerate(idxs):
        if s == 0:
            x_in, status, dt, qs = x_prev.cpu().numpy().astype(np.float64), np.zeros((B, N), np.int32), np.ones(B), np.full(6, q0)
        else:
            p = idxs[s - 1]
            with torch.no_grad():
                y = model.forward(x_prev.reshape(B * N, 6), t[p:g + 1], {"meal": meal[:, p:g + 1].repeat_interleave(N, 0)})
            x_in = y[:, -1].reshape(B, N, 6).cpu().numpy().astype(np.float64)
            status = model.last_solve_info["status"].view(B, N).cpu().numpy()
            dt, qs = np.full(B, float(t[g].double() - t[p].double())), np.full(6, q)
        for b in range(B):
            ref = FR.step(x_in[b], obs[b, g], sigma, qs, dt[b], lw[b], s, seed=seed, key=b, link=1, ess_frac=0.5, status=status[b])
            assert ref["tie"] > N * 2.0 ** -50, (s, b, ref["tie"])
            what = f"step {s} (grid {g}) patient {b}"
            assert np.array_equal(ancs[s, b], ref["anc"]), what
            _check_states(hist[s, b], ref["x_out"], torch.float32, what)
            got = np.concatenate([[float(res.log_evidence_steps[b, s]), float(res.ess[b, s]), float(res.resampled[b, s]), float(res.alive[b, s])],
                                  res.mean[b, s].cpu().numpy()])
            np.testing.assert_allclose(got, ref["stats"][:10], rtol=_rtol(N), atol=0.0, err_msg=what)
            # (the result holds the standard deviation: its square carries the roundings of the root and of the square, < 4 * 2^-52)
            np.testing.assert_allclose(res.std[b, s].cpu().numpy() ** 2, ref["stats"][10:], rtol=_rtol(N) + 4 * 2.0 ** -52, atol=0.0, err_msg=what)
            lw[b] = ref["lw"]
            resampled += int(ref["stats"][2])
        x_prev = res.history[s]
    assert 0 < resampled < B * len(idxs)                            # both branches were taken
    np.testing.assert_allclose(res.log_weights.cpu().numpy(), lw, rtol=_rtol(N), atol=0.0)
    assert torch.equal(res.particles, res.history[-1]) and torch.equal(res.times, t[res.step_index])
    np.testing.assert_allclose(res.weights().sum(1).cpu().numpy(), 1.0, rtol=1e-12)
    sm, ss = res.smoothed()
    assert sm.shape == (B, len(idxs), 6) and torch.isfinite(sm).all() and torch.isfinite(ss).all()
    keep = ~res.resampled[:, -1]                                    # (a resampling at the last step redraws the cloud)
    np.testing.assert_allclose(sm[keep, -1].cpu().numpy(), res.mean[keep, -1].cpu().numpy(), rtol=1e-6)   # (from the fp32 particles)
    assert ((sm[:, -1] - res.mean[:, -1]).abs() <= res.std[:, -1] + 1e-6).all()


def test_without_noise_the_evidence_is_the_gaussian_log_likelihood(setup):
    """(b) process_noise = 0, initial_spread = 0, ess_threshold = 0: every particle is the same trajectory."""
    from inference import run_filter
    model, data, sigma, _ = setup
    n = 16
    res = run_filter(model, data, n_particles=n, process_noise=0.0, initial_spread=0.0, noise_sigma=sigma, ess_threshold=0.0)
    assert not res.resampled.any() and (res.alive == n).all()
    assert (res.particles == res.particles[:, :1]).all() and (res.std == 0).all()
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
            for j in range(6):
                if math.isfinite(obs[b, g, j]):
                    z = (obs[b, g, j] - xs[b, j]) / sigma[j]
                    want[b, s] += (-0.5 * (z * z) - math.log(sigma[j])) - FR.HALF_LOG_2PI
    assert torch.equal(res.particles[:, 0], x)
    got = res.log_evidence_steps.cpu().numpy()
    print("max |evidence - log-likelihood| per step", np.abs(got - want).max())
    # the kernel's increment is the difference of two numbers of the size of the accumulated log-weight + log n, each rounded a few
    # times: an absolute error of some ulps of THAT size, on top of the relative bound of the kernel tests
    big = np.abs(np.cumsum(want, 1)).max() + math.log(n)
    np.testing.assert_allclose(got, want, rtol=_rtol(n), atol=8 * 2.0 ** -53 * big)
    np.testing.assert_allclose(res.log_evidence().cpu().numpy(), want.sum(1), rtol=_rtol(n), atol=len(idxs) * 8 * 2.0 ** -53 * big)


def test_the_filter_tracks_a_patient_whose_initial_glucose_is_wrong():
    """(c) data from the model itself, 2 % noise, only glucose observed; the filter starts from a glucose x0 that is 30 % off.
    Over the second half of the grid its filtered glucose mean is closer to the truth than the open-loop solve from that x0."""
    from inference import run_filter
    model = _model("relu64x4")
    data, _, truth = _data(model, missing=False)
    g = torch.Generator(device=DEV).manual_seed(9)
    sigma = np.full(6, 1.0)
    sigma[0] = 0.02 * float(truth[..., 0].mean())
    obs = torch.full_like(truth, float("nan"))
    obs[..., 0] = truth[..., 0] + sigma[0] * torch.randn(B, T, device=DEV, generator=g)
    wrong = data["initial_state"].clone()
    wrong[:, 0] *= 1.3
    with torch.no_grad():
        open_loop = model.forward(wrong, data["time_points"], data["external_inputs"])
    res = run_filter(model, dict(data, initial_state=wrong, observations=obs), n_particles=N, process_noise=0.05,
                     initial_spread=[0.3, 0.05, 0.05, 0.05, 0.0, 0.05], noise_sigma=sigma, seed=2)
    assert res.step_index.tolist() == list(range(T))
    half = slice(T // 2, T)
    rmse = lambda a: float(((a[:, half] - truth[:, half, 0].double()) ** 2).mean().sqrt())                 # noqa: E731
    e_filter, e_open = rmse(res.mean[..., 0]), rmse(open_loop[..., 0].double())
    print(f"glucose RMSE over the second half: filter {e_filter:.4f}, open loop {e_open:.4f}, sigma {sigma[0]:.4f}")
    assert torch.isfinite(res.log_evidence()).all()
    assert e_filter < e_open


def test_forecast_equals_a_run_with_trailing_nan_rows(setup):
    """(d) bit for bit."""
    from inference import run_filter
    model, data, sigma, _ = setup
    cut = 9
    obs = data["observations"].clone()
    obs[:, cut:] = float("nan")
    kw = dict(n_particles=N, process_noise=0.04, noise_sigma=sigma, seed=11, ode_sets={"a_GI": torch.linspace(0.009, 0.012, N)})
    full = run_filter(model, dict(data, observations=obs), **kw)
    meal = data["external_inputs"]["meal"]
    head = run_filter(model, dict(data, observations=obs[:, :cut], time_points=data["time_points"][:cut],
                                  external_inputs={"meal": meal[:, :cut]}), **kw)
    tail = head.forecast(data["time_points"][cut - 1:], {"meal": meal[:, cut - 1:]})
    assert full.step_index.tolist() == head.step_index.tolist() + [T - 1] and tail.step_index.tolist() == [T - cut]
    bits = lambda v: v.cpu().numpy().tobytes()                                                              # noqa: E731
    for name in ("particles", "log_weights", "ode_p"):
        assert bits(getattr(full, name)) == bits(getattr(tail, name)), name
    for name in ("mean", "std", "ess", "log_evidence_steps", "alive", "resampled"):
        assert bits(getattr(full, name)[:, -1:]) == bits(getattr(tail, name)), name
        assert bits(getattr(full, name)[:, :-1]) == bits(getattr(head, name)), name
    assert (tail.log_evidence_steps == 0).all()                     # nothing observed: no evidence


def test_ode_sets_rows_follow_their_particles(setup):
    """(e) after forced resampling ode_p[i] is the input row of the particle's ancestor."""
    from inference import run_filter
    from models.ode_core import ODE_PARAM_NAMES
    model, data, sigma, _ = setup
    a = torch.linspace(0.008, 0.013, N)
    k = (0.05 + 0.01 * torch.arange(B * N).reshape(B, N) / (B * N))
    res = run_filter(model, data, n_particles=N, noise_sigma=sigma, ess_threshold=1.0, seed=4, ode_sets={"a_GI": a, "ode_k_I": k},
                     store_particles=True)
    assert res.resampled.float().mean() > 0.5                       # (an unobserved patient right after a resampling keeps ESS = N)
    idx = torch.arange(N, device=DEV).expand(B, N)
    for s in range(res.ancestors.shape[0] - 1, -1, -1):
        idx = res.ancestors[s].long().gather(1, idx)
    assert (idx != torch.arange(N, device=DEV)).any()
    ja, jk = ODE_PARAM_NAMES.index("a_GI"), ODE_PARAM_NAMES.index("k_I")
    assert torch.equal(res.ode_p[:, :, ja], a.to(DEV)[idx]) and torch.equal(res.ode_p[:, :, jk], k.to(DEV).gather(1, idx))
    base = model.ode_core.param_vector().to(DEV)
    others = [j for j in range(17) if j not in (ja, jk)]
    assert (res.ode_p[:, :, others] == base[others]).all()


def test_run_filter_fp64_and_per_patient_grids_agree_with_fp32_shared(setup):
    """The fp64 path and a per-patient [B, T] grid run the same loop: filtered means close to the fp32 / shared-grid run."""
    from inference import run_filter
    model, data, sigma, _ = setup
    kw = dict(n_particles=N, process_noise=0.04, noise_sigma=sigma, seed=6, ess_threshold=0.0)
    a = run_filter(model, data, **kw)
    b = run_filter(model, dict(data, time_points=data["time_points"].expand(B, T).contiguous()), **kw)
    c = run_filter(model, data, dtype=torch.float64, **kw)
    assert b.times.shape == (B, len(a.step_index))
    np.testing.assert_allclose(b.mean.cpu().numpy(), a.mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(c.mean.cpu().numpy(), a.mean.cpu().numpy(), rtol=2e-3, atol=1e-3)
    assert c.particles.dtype == torch.float64 and torch.isfinite(c.log_evidence()).all()
