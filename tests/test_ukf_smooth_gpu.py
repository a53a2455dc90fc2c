"""The unscented RTS smoother's kernels (csrc/hode_ukf_smooth.hip) and UKFResult.smooth on the GPU, held to the numpy restatement
of tests/_ukf_smooth_reference.py.  `-m gpu`.

Tolerances against the restatement.  Every pair of steps and every step of the recursion is compared on
its own: the restatement of step s is fed the device's own values of step s + 1, so no bound is a compound.  The orders of all
sums are the restatement's; what differs is the device's log and exp.
  pred_mean, pred_cov, gain, mean_s   within 64 n c 2^-52 of the largest magnitude in the same array, c the condition number of
                     that pair's P- (on its non-zero columns) from the restatement (tests/test_ukf_smooth_host.py keeps c <= 1e6);
  cov_s              within the same factor of max(max |P_s|, the largest entry of |G| |D| |G^T|): the size its terms reach;
  moments            the same factor of the largest magnitude, c of the pair that starts at the step (the last live pair for the
                     terminal step; for a patient with one live step, of the covariance itself);
  a dead step        NaN in every output, the gain into it included; the terminal step a copy, bit for bit.
Every comparison prints `UKF_FRACTION smooth-<what> <worst error / bound>`."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

import _ukf_cases as UC  # noqa: E402
import _ukf_reference as UR  # noqa: E402
import _ukf_smooth_cases as SC  # noqa: E402
import _ukf_smooth_reference as SR  # noqa: E402

DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}
NAMES = ("mean_s", "cov_s", "gain", "pred_mean", "pred_cov", "moments")
bits = lambda v: np.ascontiguousarray(v).view(np.uint8)                                 # noqa: E731  (NaN and -0 included)


def _bound(n, cond):
    return 64 * n * cond * 2.0 ** -52


def _args(c, dtype, sel=None):
    pick = (lambda a: a) if sel is None else (lambda a: a[:, sel:sel + 1])
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(pick(a)), dtype=dt, device=DEV)                      # noqa: E731
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)                     # noqa: E731
    return dict(history=dev(c["hist"], dtype), ode_history=dev(c["ode"], dtype), propagated=dev(c["prop"], dtype),
                mean=dev(c["mean_f"], torch.float64), cov=dev(c["cov_f"], torch.float64), alive=dev(c["alive"], torch.int32),
                mode=c["mode"], q=f64(c["q"]), walk=f64(c["walk"]), dt=dev(c["dt"], torch.float64), weights=c["w"], link=c["link"])


def _run_case(c, dtype, sel=None):
    """The three kernels on the case `c` (all patients, or patient `sel` alone) -> dict of numpy arrays, step-major."""
    out = hode.capi.ukf_smooth(**_args(c, dtype, sel))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(NAMES, out)}


def _rel(got, ref, scale=None):
    scale = np.abs(ref).max() if scale is None else scale
    err = np.abs(got - ref).max()
    return err / scale if scale > 0 else err


def _check_patient(got, b, ref, c, what):
    """One patient of a device result against the restatement; returns the worst error / bound."""
    S, n = c["S"], c["n"]
    mean_f, cov_f = c["mean_f"][:, b], c["cov_f"][:, b]
    term = ref["terminal"]
    worst = 0.0

    def hold(name, err, bound):
        nonlocal worst
        worst = max(worst, err / bound)
        assert err <= bound, f"{what} {name}: {err:.3e} > {bound:.3e}"

    # the pairs: functions of the inputs alone
    for s in range(S - 1):
        if not c["alive"][s + 1, b]:
            assert all(np.isnan(got[k][s, b]).all() for k in ("gain", "pred_mean", "pred_cov")), f"{what} pair {s} into a dead step"
            continue
        for name in ("pred_mean", "pred_cov", "gain"):
            hold(f"{name}[{s}]", _rel(got[name][s, b], ref[name][s]), _bound(n, ref["cond"][s]))
    # the recursion, fed the device's own step s + 1
    for s in range(S):
        if s > term:
            assert all(np.isnan(got[k][s, b]).all() for k in ("mean_s", "cov_s", "moments")), f"{what} step {s} is dead"
            continue
        if s == term:
            assert np.array_equal(bits(got["mean_s"][s, b]), bits(mean_f[s])) and np.array_equal(bits(got["cov_s"][s, b]), bits(cov_f[s])), what
            continue
        ms, Ps, scale = SR.back(mean_f[s], cov_f[s], got["gain"][s, b], got["pred_mean"][s, b], got["pred_cov"][s, b],
                                got["mean_s"][s + 1, b], got["cov_s"][s + 1, b])
        bound = _bound(n, ref["cond"][s])
        hold(f"mean_s[{s}]", _rel(got["mean_s"][s, b], ms), bound)
        hold(f"cov_s[{s}]", _rel(got["cov_s"][s, b], Ps, max(np.abs(cov_f[s]).max(), scale)), bound)
    # the natural-space moments of the device's own smoothed moments
    for s in range(term + 1):
        if term > 0:
            cond = ref["cond"][min(s, term - 1)]
        else:
            _, zero, _ = UR.cholesky(cov_f[s])
            keep = [j for j in range(n) if j not in zero]
            cond = UR._cond(cov_f[s][np.ix_(keep, keep)])
        mo = SR.moments(got["mean_s"][s, b], got["cov_s"][s, b], c["mode"], c["w"], c["link"])
        hold(f"moments[{s}]", _rel(got["moments"][s, b], mo), _bound(n, cond))
    return worst


# ------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", range(len(SC.SPECS)), ids=[SC.case_id(s) for s in SC.SPECS])
def test_smoother_kernels_against_the_restatement(idx, dtype):
    spec, c, refs = SC.SPECS[idx], SC.case(idx), SC.reference(idx)
    got = _run_case(c, dtype)
    assert got["gain"].shape == (c["S"] - 1, c["B"], c["n"], c["n"]) and got["moments"].shape == (c["S"], c["B"], 12)
    worst = 0.0
    for b, ref in enumerate(refs):
        worst = max(worst, _check_patient(got, b, ref, c, f"case {SC.case_id(spec)} patient {b}"))
    print(f"UKF_FRACTION smooth-{SC.case_id(spec)}-{NP[dtype].__name__} {worst:.4f}")
    if spec.get("edge") == "lost":
        assert refs[1]["terminal"] == 1 and np.isnan(got["mean_s"][2:, 1]).all() and np.isfinite(got["mean_s"][:2, 1]).all()
        assert np.isfinite(got["mean_s"][:, [0, 2, 3, 4]]).all()
    if spec.get("edge") == "zero_state":                                # exactly zero: a held coordinate takes and gives nothing
        assert not got["gain"][:, :, 2, :].any() and not got["gain"][:, :, :, 2].any()
        assert not got["cov_s"][:, :, 2, :].any() and not got["cov_s"][:, :, :, 2].any()
        assert np.array_equal(bits(got["mean_s"][:, :, 2]), bits(c["mean_f"][:, :, 2]))


# ------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", [0, 4], ids=[SC.case_id(SC.SPECS[i]) for i in (0, 4)])
def test_smoother_is_deterministic_and_independent_of_the_batch(idx, dtype):
    """The same call twice gives the same bits; patient 2 of B = 3 gives the bits of that patient alone (n = 6 and n = 23)."""
    c = SC.case(idx)
    assert c["B"] == 3 and c["n"] == (6, 23)[idx == 4]
    a, b = _run_case(c, dtype), _run_case(c, dtype)
    alone = _run_case(c, dtype, sel=2)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
        assert np.array_equal(bits(a[k][:, 2:3]), bits(alone[k])), k


# ------------------------------------------------------------------ 3. what the binding refuses
def test_capi_rejects_what_the_kernels_cannot_take():
    c = SC.case(0)
    base = _args(c, torch.float32)
    S, B, n = c["S"], c["B"], c["n"]
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=DEV)                                      # noqa: E731
    outs = lambda: [f64(S, B, n), f64(S, B, n, n), f64(S - 1, B, n, n), f64(S - 1, B, n), f64(S - 1, B, n, n), f64(S, B, 12)]  # noqa: E731
    aliased = outs()
    aliased[1] = base["cov"]
    twice = outs()
    twice[4] = twice[2]
    for change in (dict(history=base["history"][:, :, :-1].contiguous()),                 # a wrong K
                   dict(mode=UC.mode_of(1)),                                              # (K from another n)
                   dict(ode_history=base["ode_history"].double()),                        # a dtype mismatch
                   dict(propagated=base["propagated"].double()),
                   dict(mean=base["mean"].float()),
                   dict(cov=base["cov"].cpu()),                                           # a host tensor
                   dict(dt=base["dt"][:-1].contiguous()),                                 # a short dt
                   dict(alive=base["alive"].long()),
                   dict(out=tuple(aliased)),                                              # an output that is an input
                   dict(out=tuple(twice)),
                   dict(out=tuple(outs()[:5]))):
        with pytest.raises(hode.capi.HodeError):
            hode.capi.ukf_smooth(**dict(base, **change))
    with pytest.raises(hode.capi.HodeError):
        hode.capi.ukf_smooth(**dict(base, history=base["history"].cpu()))


# ------------------------------------------------------------------ 4. a linear model on the device is the Kalman RTS smoother
@pytest.mark.parametrize("which", [1, 2])
def test_identity_link_on_the_device_reproduces_the_kalman_rts_smoother(which):
    """The filter as tests/test_ukf_gpu.py runs it -- x_in = A chi_x + Bm chi_theta formed in torch (fp64) from the kernel's own
    x_out / aux_out --, everything the smoother reads kept, then one call."""
    M = UC.linear_model(which)
    w = hode.capi.ukf_weights(M["n"])
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)                     # noqa: E731
    A, Bm, sigma, q, walk = f64(M["A"]), f64(M["Bm"]), f64(M["sigma"]), f64(M["q"]), f64(M["walk"])
    n, K, cols, S = M["n"], 2 * M["n"] + 1, M["cols"], M["S"]
    x, aux = torch.zeros(1, K, 6, dtype=torch.float64, device=DEV), torch.ones(1, K, 17, dtype=torch.float64, device=DEV)
    mean, cov, alive = f64(M["m0"][None]), f64(M["P0"][None]), torch.ones(1, dtype=torch.int32, device=DEV)
    hist, odeh, prop, meanh, covh, aliveh = [], [], [], [], [], []
    for s in range(S):
        if s > 0:
            x = (x @ A.T + aux[:, :, cols] @ Bm.T).contiguous()
        prop.append(x)
        x, aux, _ = hode.capi.ukf_step(x, aux, M["mode"], f64(M["ys"][s][None]), sigma, q, walk, f64(M["dts"][s:s + 1]), alive, mean, cov, w,
                                       predict=s > 0, link=0)
        hist.append(x), odeh.append(aux), meanh.append(mean.clone()), covh.append(cov.clone()), aliveh.append(alive.clone())
    st = lambda v: torch.stack(v).contiguous()                                                                     # noqa: E731
    mean_s, cov_s, gain, pm, pc, mo = hode.capi.ukf_smooth(st(hist), st(odeh), st(prop), st(meanh), st(covh), st(aliveh), M["mode"], q, walk,
                                                           f64(M["dts"][:, None]), w, link=0)
    assert bool(st(aliveh).all())
    want = SC.kalman_rts(M)
    em = max(np.abs(want[s][0] - mean_s[s, 0].cpu().numpy()).max() for s in range(S))
    eP = max(np.abs(want[s][1] - cov_s[s, 0].cpu().numpy()).max() for s in range(S))
    print(f"model {which} on the device: smoothed mean {em:.2e}, covariance {eP:.2e}")
    assert max(em, eP) <= 1e-10
    assert torch.equal(mean_s[-1], meanh[-1]) and torch.equal(cov_s[-1], covh[-1])
    np.testing.assert_allclose(mo[:, 0, :6].cpu().numpy(), mean_s[:, 0, :6].cpu().numpy(), rtol=0, atol=1e-12)   # (identity link)


# ------------------------------------------------------------------ 5. UKFResult.smooth end to end
from test_ukf_gpu import B, LINKS, T, _data, _model  # noqa: E402  (the fixtures of the filter's own end-to-end tests)


@pytest.fixture(scope="module", params=["relu64x4", "tanh32x2"])
def setup(request):
    from inference import ParameterLearning
    m = _model(request.param)
    data, sigma, truth = _data(m)
    scale = (truth.abs().mean((0, 1)) + 0.1).double().cpu().numpy()
    link = LINKS[request.param]
    rel = 1.0 if link == "log" else scale
    learn = ParameterLearning(["k_I", "a_GI"], walk=[0.1, 0.0], initial_spread=0.2) if request.param == "relu64x4" else None
    kw = dict(process_noise=0.04 * rel, initial_spread=0.1 * rel, noise_sigma=sigma, noise_link=link, learn=learn)
    return m, data, kw


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_smooth_of_a_run(setup):
    from inference import UKFSmoothResult, run_ukf
    model, data, kw = setup
    plain = run_ukf(model, data, **kw)
    res = run_ukf(model, data, store_history=True, **kw)
    # storing changes nothing the filter reports
    for name in ("mean", "std", "nis", "n_seen", "log_evidence_steps", "alive", "step_index", "times", "sigma_points", "ode_p", "state_mean",
                 "state_cov"):
        assert _eq(getattr(plain, name), getattr(res, name)), name
    if kw["learn"] is not None:
        assert _eq(plain.learned.location, res.learned.location) and _eq(plain.learned.scale, res.learned.scale)
    S, n, K = len(res.step_index), res.state_mean.shape[1], res.sigma_points.shape[1]
    assert res.propagated_history.shape == (S, B, K, 6) and res.propagated_history.dtype == res.history.dtype
    assert res.dt_history.shape == (S, B) and res.dt_history.dtype == torch.float64
    tt = res.times.double()
    assert torch.equal(res.dt_history[1:], (tt[1:] - tt[:-1])[:, None].expand(S - 1, B)) and plain.propagated_history is None
    assert torch.equal(res.propagated_history[0], data["initial_state"][:, None].expand(B, K, 6))

    sm = res.smooth()
    assert isinstance(sm, UKFSmoothResult) and res.alive.all()
    assert sm.mean.shape == (B, S, 6) and sm.std.shape == (B, S, 6) and sm.state_mean.shape == (B, S, n) and sm.state_cov.shape == (B, S, n, n)
    assert sm.gain.shape == (B, S - 1, n, n) and sm.pred_mean.shape == (B, S - 1, n) and sm.pred_cov.shape == (B, S - 1, n, n)
    assert sm.alive is res.alive and sm.step_index is res.step_index and sm.times is res.times
    assert all(bool(torch.isfinite(getattr(sm, k)).all()) for k in ("mean", "std", "state_mean", "state_cov", "gain", "pred_mean", "pred_cov"))
    # the last step is the filter's, bit for bit
    assert _eq(sm.mean[:, -1], res.mean[:, -1]) and _eq(sm.std[:, -1] ** 2, res.std[:, -1] ** 2)
    assert _eq(sm.state_mean[:, -1], res.state_mean) and _eq(sm.state_cov[:, -1], res.state_cov)
    # hindsight narrows: no link-space variance above the filtered one
    var_s, var_f = sm.state_cov.diagonal(dim1=2, dim2=3), res.cov_history.diagonal(dim1=2, dim2=3).transpose(0, 1)
    assert (var_s <= var_f * (1 + 64 * n * 2.0 ** -52)).all(), float((var_s / var_f).max())
    assert (var_s < var_f).any() and not torch.equal(sm.state_mean[:, :-1], res.mean_history.transpose(0, 1)[:, :-1])
    # the predicted moments are what the filter's next step started from: without an update there, they are its moments
    unseen = [(b, s) for b in range(B) for s in range(1, S) if int(res.n_seen[b, s]) == 0]
    assert unseen
    for b, s in unseen:
        assert _eq(sm.pred_mean[b, s - 1], res.mean_history[s, b]) and _eq(sm.pred_cov[b, s - 1], res.cov_history[s, b]), (b, s)
    if kw["learn"] is None:
        assert sm.learned is None
    else:
        assert sm.learned.names == ["k_I", "a_GI"] == res.learned.names
        rank = np.argsort(np.argsort(kw["learn"].columns))
        at = torch.as_tensor(6 + rank, device=DEV)
        assert torch.equal(sm.learned.location, sm.state_mean[..., at]) and sm.learned.location.shape == (B, S, 2)
        assert _eq(sm.learned.location[:, -1], res.learned.location[:, -1]) and _eq(sm.learned.scale[:, -1], res.learned.scale[:, -1])
        assert (sm.learned.scale <= res.learned.scale * (1 + 64 * n * 2.0 ** -52)).all()
    # refusals
    with pytest.raises(ValueError, match="store_history"):
        plain.smooth()
    meal = data["external_inputs"]["meal"]
    tail = res.forecast(torch.cat([data["time_points"][-1:], data["time_points"][-1:] + 0.5]), {"meal": meal[:, -2:] * 0})
    with pytest.raises(ValueError, match="forecast"):
        tail.smooth()


def test_after_the_last_observation_smoothed_is_filtered(setup):
    """Observations cut to NaN after row 9: from the last step that saw anything on, delta and D are exactly zero."""
    from inference import run_ukf
    model, data, kw = setup
    obs = data["observations"].clone()
    obs[:, 9:] = float("nan")
    res = run_ukf(model, dict(data, observations=obs), store_history=True, **kw)
    sm = res.smooth()
    idxs = res.step_index.tolist()
    assert idxs[-2:] == [8, T - 1] and res.alive.all()
    s0 = idxs.index(8)
    assert _eq(sm.state_mean[:, s0:], res.mean_history.transpose(0, 1)[:, s0:]) and _eq(sm.state_cov[:, s0:], res.cov_history.transpose(0, 1)[:, s0:])
    assert _eq(sm.mean[:, s0:], res.mean[:, s0:]) and _eq(sm.std[:, s0:], res.std[:, s0:])
    assert not torch.equal(sm.state_mean[:, s0 - 1], res.mean_history[s0 - 1])


# ------------------------------------------------------------------ 6. what it is for
def test_hindsight_tracks_the_early_record_better_than_the_filter():
    """The data of test_the_filter_tracks_a_patient_whose_initial_glucose_is_wrong (tests/test_ukf_gpu.py): records from the model
    itself, only glucose observed at 2 % noise, the filter started from a glucose x0 that is 30 % off.  The filter needs the first
    observations to find the patient; the smoother also knows what came after.  Over the first half of the grid the smoothed
    glucose is closer to the truth than the filtered one."""
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
    size = (truth.abs().mean((0, 1)) + 0.1).double().cpu().numpy()
    res = run_ukf(model, dict(data, initial_state=wrong, observations=obs), process_noise=0.05 * size * np.array([1, 1, 1, 1, 0, 1.0]),
                  initial_spread=np.array([0.3, 0.05, 0.05, 0.05, 0.0, 0.05]) * size, noise_sigma=sigma, noise_link="additive",
                  store_history=True)
    sm = res.smooth()
    assert res.step_index.tolist() == list(range(T)) and res.alive.all()
    half = slice(0, T // 2)
    rmse = lambda a: float(((a[:, half] - truth[:, half, 0].double()) ** 2).mean().sqrt())                 # noqa: E731
    e_smooth, e_filter = rmse(sm.mean[..., 0]), rmse(res.mean[..., 0])
    print(f"glucose RMSE over the first half: smoothed {e_smooth:.4f}, filtered {e_filter:.4f}, sigma {sigma[0]:.4f}")
    assert e_smooth < e_filter
