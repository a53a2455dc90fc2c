"""The particle-smoother kernel (csrc/hode_smooth.hip) and FilterResult.smooth on the GPU, held to the numpy restatement of
tests/_smooth_reference.py.  `-m gpu`.

`idx` is compared exactly and `paths` bit for bit (a gather of `hist`).  Exact indices need every pointer u c_{N-1} further from
every boundary c_k than the kernel's and the restatement's c_k / c_{N-1} can differ.  Both take the same fp64 operations in the
same order with contraction off (the running sum included: a lane's sum IS the sequential one), so they differ only through
libm, and the bound on that difference has three parts:
  the sum    c_k is a sum of up to N non-negative terms; were the order to differ, each partial sum would carry half an ulp,
             N * 2^-53 of c_{N-1} in all (it does not differ here; the term is kept as the issue of this feature sets it);
  exp        w_i = exp(l_i - mx): one ulp of the library (2^-52 relative), and the argument's own rounding and the difference of
             the two mx, each <= 2^-53 |l_i - mx| absolute in the argument, i.e. relative in w_i: 2^-52 (2 + spread) with
             spread = max |l_i - mx| over the candidates alive, counting generously;
  log        under the log link one ulp in log p_j (and in log x~_j) moves z_j by 2^-52 |log v| r_j and tau_j = -z_j^2 / 2 by
             |z_j| times that: 2^-52 logamp per logarithm, logamp = max |log v| |z_j| r_j, 12 logarithms per pair.
A relative error e in every w_i moves c_k / c_{N-1} by at most 2 e (numerator and denominator):
  bound = N 2^-53 + 2 (2^-52 (2 + spread) + 12 * 2^-52 logamp)            (_smooth_reference.tie_bound).
Every case keeps tie >= 100 * bound; tests/test_smooth_host.py shows that on the CPU, and the tests here assert it again."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

import _smooth_cases as SC  # noqa: E402
import _smooth_reference as SR  # noqa: E402

DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}
bits = lambda v: np.ascontiguousarray(v).view(np.uint8)                                    # noqa: E731  (NaN included)


def _run(d, dtype, M=None, sel=None, id0=None):
    """The kernel on case inputs `d` (all patients, or patient `sel` alone) -> (idx [S, B, M], paths [S, B, M, 6]) as numpy."""
    pick = (lambda a: a) if sel is None else (lambda a: a[:, sel:sel + 1])
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(pick(a)), dtype=dt, device=DEV)                    # noqa: E731
    idx, paths = hode.capi.pf_smooth(dev(d["hist"], dtype), dev(d["lwh"], torch.float64), dev(d["pred"], dtype),
                                     torch.as_tensor(d["q"], dtype=torch.float64, device=DEV), dev(d["dt"], torch.float64),
                                     d["M"] if M is None else M, seed=d["seed"], id0=d["id0"] if id0 is None else id0,
                                     link=SC.LINK[d["link"]])
    torch.cuda.synchronize()
    return idx.cpu().numpy(), paths.cpu().numpy()


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("i", range(len(SC.CASES)), ids=[SC.case_id(c) for c in SC.CASES])
def test_smooth_kernel_against_the_restatement(i, dtype):
    d, refs = SC.inputs(i), SC.reference(i)
    idx, paths = _run(d, dtype)
    assert idx.shape == (d["S"], d["B"], d["M"]) and paths.shape == (d["S"], d["B"], d["M"], 6) and paths.dtype == NP[dtype]
    for b, ref in enumerate(refs):
        what = f"case {SC.case_id(d)} patient {b}"
        bound = SR.tie_bound(d["N"], ref["spread"], ref["logamp"])
        print(what, f"tie {ref['tie']:.3e} = {ref['tie'] / bound:.3g} x bound")
        assert ref["tie"] >= 100 * bound, what
        assert np.array_equal(idx[:, b], ref["idx"]), (what, np.argwhere(idx[:, b] != ref["idx"])[:8])
        assert np.array_equal(bits(paths[:, b]), bits(ref["paths"].astype(NP[dtype]))), what
    c = SC.CASES[i]
    if c["edge"] == "patient_dead":                                 # lost from the dead step back, the neighbours untouched
        s0 = min(2, c["S"] - 1)
        assert (idx[:s0 + 1, 1] == -1).all() and np.isnan(paths[:s0 + 1, 1]).all() and (idx[s0 + 1:, 1] >= 0).all()
        assert (idx[:, 0] >= 0).all() and (idx[:, 2] >= 0).all()
    if c["edge"] == "dead" and c["N"] > 1:
        assert not (idx[0] == c["N"] // 2).any()                    # the dead candidate of step 0
        assert not (idx[:-1] == c["N"] // 3).any()                  # the slot whose pred row is NaN
    if c["edge"] == "q0" and c["S"] > 1:                            # the point mass: the noiseless state never changes along a path
        assert (paths[..., 2] == paths[-1:, ..., 2]).all()


_DET = [c["idx"] for c in SC.CASES if c["B"] == 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("i", _DET, ids=[SC.case_id(SC.CASES[i]) for i in _DET])
def test_smooth_kernel_is_reproducible_and_independent_of_the_launch(i, dtype):
    """The same call twice gives the same bits; trajectory m of an M = 300 call is trajectory m of an M = 65 call; patient 2 of
    B = 3 gives the bits of that patient alone with id0 + 2."""
    d = SC.inputs(i)
    a, b = _run(d, dtype, M=300), _run(d, dtype, M=300)
    few = _run(d, dtype, M=65)
    alone = _run(d, dtype, M=300, sel=2, id0=d["id0"] + 2)
    for k in range(2):
        assert np.array_equal(bits(a[k]), bits(b[k]))
        assert np.array_equal(bits(a[k][:, :, :65]), bits(few[k]))
        assert np.array_equal(bits(a[k][:, 2:3]), bits(alone[k]))
    if d["N"] > 2:                                                  # (and the trajectories are not all the same one)
        assert (a[0] >= 0).any() and not np.array_equal(a[0][:, :, :65], a[0][:, :, 65:130])


# ------------------------------------------------------------------ 2. run_filter(..., store_particles=True).smooth()
B, N, T = 3, 128, 13
X0 = [8.0, 90.0, 80.0, 10.0, 0.3, 0.5]       # (every state positive: under the log link a state at 0 has no transition density)


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
            p.normal_(0.0, 0.05)
    return m


def _data(model, n_points=T, sigma_rel=0.05, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x0 = torch.tensor(X0, device=DEV) * (1 + 0.1 * torch.randn(B, 6, device=DEV, generator=g))
    t = torch.linspace(0.0, 2.0 * (n_points - 1) / (T - 1), n_points, device=DEV)
    meal = torch.zeros(B, n_points, device=DEV)
    meal[:, 2:5] = torch.tensor([20.0, 40.0, 10.0], device=DEV)
    with torch.no_grad():
        y = model.forward(x0, t, {"meal": meal})
    scale = y.abs().mean((0, 1)) + 0.1
    obs = y + sigma_rel * scale * torch.randn(y.shape, device=DEV, generator=g)
    return {"initial_state": x0, "observations": obs, "time_points": t, "external_inputs": {"meal": meal}}, (sigma_rel * scale).double().cpu().numpy()


@pytest.fixture(scope="module", params=["relu64x4", "tanh32x2"])
def setup(request):
    from inference import run_filter
    m = _model(request.param)
    data, sigma = _data(m)
    data["observations"][:, 3] = float("nan")                      # a grid point nobody observes: no filter step there
    data["observations"][1, 5, :] = float("nan")                   # one patient unobserved at a step
    kw = dict(n_particles=N, process_noise=0.04, initial_spread=0.1, noise_sigma=sigma, ess_threshold=0.5, seed=5)
    return m, data, kw, run_filter(m, data, store_particles=True, **kw), run_filter(m, data, **kw)


def test_storing_changes_no_other_output(setup):
    _, _, _, res, plain = setup
    assert plain.history is None and plain.predicted is None and plain.log_weight_history is None and plain.step_dt is None
    for name in ("mean", "std", "ess", "log_evidence_steps", "alive", "resampled", "particles", "log_weights", "ode_p", "step_index", "times"):
        assert bits(getattr(res, name).cpu().numpy()).tobytes() == bits(getattr(plain, name).cpu().numpy()).tobytes(), name
    S = len(res.step_index)
    assert res.predicted.shape == (S, B, N, 6) and res.predicted.dtype == torch.float32
    assert res.log_weight_history.shape == (S, B, N) and res.log_weight_history.dtype == torch.float64
    assert res.step_dt.shape == (S, B) and res.step_dt.dtype == torch.float64
    again = type(res).forecast                                      # (a forecast from either result continues identically)
    t2 = torch.stack([res.times[-1], res.times[-1] + 0.25])
    fa, fb = again(res, t2), again(plain, t2)
    assert torch.equal(fa.particles, fb.particles) and torch.equal(fa.mean, fb.mean)
    with pytest.raises(ValueError, match="forecast"):
        fa.smooth()
    with pytest.raises(ValueError, match="store_particles=True"):
        plain.smooth()


def test_the_stored_tensors_are_what_the_steps_saw(setup):
    model, data, kw, res, _ = setup
    idxs = res.step_index.tolist()
    t, meal = data["time_points"], data["external_inputs"]["meal"]
    assert torch.equal(res.predicted[0], data["initial_state"].reshape(B, 1, 6).expand(B, N, 6))
    assert torch.equal(res.log_weight_history[-1], res.log_weights)
    assert torch.equal(res.step_dt[0], torch.ones(B, dtype=torch.float64, device=DEV))
    for s in range(1, len(idxs)):
        p, g = idxs[s - 1], idxs[s]
        with torch.no_grad():
            y = model.forward(res.history[s - 1].reshape(B * N, 6), t[p:g + 1], {"meal": meal[:, p:g + 1].repeat_interleave(N, 0)})
        want = y[:, -1].reshape(B, N, 6)
        print(f"step {s}: max |predicted - model.forward| {float((res.predicted[s] - want).abs().max()):.3e}")
        assert torch.equal(res.predicted[s], want), s
        assert torch.equal(res.step_dt[s], (t[g].double() - t[p].double()).expand(B)), s
        assert (res.log_weight_history[s] == 0).all(1)[res.resampled[:, s]].all()    # 0 in every slot where the step resampled
    assert 0 < int(res.resampled.sum()) < res.resampled.numel()


def test_smooth_equals_the_restatement_on_the_stored_tensors(setup):
    _, _, kw, res, _ = setup
    M = 96
    sm = res.smooth(n_trajectories=M, seed=17)
    S = len(res.step_index)
    assert sm.paths.shape == (B, M, S, 6) and sm.index.shape == (B, M, S) and sm.index.dtype == torch.int32
    assert torch.equal(sm.step_index, res.step_index) and torch.equal(sm.times, res.times)
    hist, lwh, pred = res.history.cpu().numpy(), res.log_weight_history.cpu().numpy(), res.predicted.cpu().numpy()
    q, dt = np.full(6, kw["process_noise"]), res.step_dt.cpu().numpy()
    for b in range(B):
        ref = SR.smooth(hist[:, b], lwh[:, b], pred[:, b], q, dt[:, b], M, seed=17, key=b, link=1)
        bound = SR.tie_bound(N, ref["spread"], ref["logamp"])
        print(f"patient {b}: tie {ref['tie']:.3e} = {ref['tie'] / bound:.3g} x bound")
        assert ref["tie"] >= 100 * bound, b
        assert np.array_equal(sm.index[b].cpu().numpy(), ref["idx"].T), b
        assert np.array_equal(bits(sm.paths[b].cpu().numpy()), bits(ref["paths"].transpose(1, 0, 2))), b
    assert int(sm.lost.sum()) == 0 and torch.isfinite(sm.mean).all() and torch.isfinite(sm.std).all()
    assert ((sm.mean[:, -1] - res.mean[:, -1]).abs() <= res.std[:, -1]).all()       # the last step is a draw from the filter
    lo, hi = sm.quantile([0.05, 0.95])
    assert lo.shape == (B, S, 6) and (lo <= hi).all()
    default = res.smooth()                                          # M = N, the filter's seed
    assert default.paths.shape == (B, N, S, 6) and torch.equal(default.index, res.smooth(seed=kw["seed"]).index)


def test_backward_simulation_keeps_what_the_genealogy_loses():
    """T = 25 with a resampling at every step, M = N = 128: at step 0 the trajectories pass through more distinct slots than the
    ancestor trace has left, for every patient."""
    from inference import run_filter
    model = _model("relu64x4")
    data, sigma = _data(model, n_points=25)
    res = run_filter(model, data, n_particles=N, process_noise=0.04, initial_spread=0.1, noise_sigma=sigma, ess_threshold=1.0, seed=8,
                     store_particles=True)
    assert res.resampled.all()
    idx = torch.arange(N, device=DEV).expand(B, N)
    for s in range(res.ancestors.shape[0] - 1, 0, -1):
        idx = res.ancestors[s].long().gather(1, idx)               # the slot of step s - 1 each final particle descends from
    traced = torch.tensor([len(set(row.tolist())) for row in idx], device=DEV)
    distinct = res.smooth().distinct()
    print("distinct step-0 slots: backward simulation", distinct[:, 0].tolist(), "genealogy trace", traced.tolist())
    assert distinct.shape == (B, 25) and (distinct[:, 0] > traced).all()
