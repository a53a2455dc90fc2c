"""The parameter-move kernel (csrc/hode_pf_params.hip) and inference.run_filter(learn=...) on the GPU, held to the numpy
restatements of tests/_pf_params_reference.py and tests/_filter_reference.py.  `-m gpu`.

Tolerances against the restatement: tests/_pf_params_cases.py derives, from each case's own numbers,
what another summation order and another libm may change in pstats and in a moved value; tests/test_pf_params_host.py shows
that the restatement under another order stays inside it.  fp32 data: that bound is far below an fp32 ulp, so the one rounding
to fp32 may differ by one ulp.  Everything the header calls untouched is compared bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

import _filter_reference as FR  # noqa: E402
import _pf_params_cases as PC  # noqa: E402
import _pf_params_reference as PR  # noqa: E402

DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}
SPREAD_STEP = 0xFFFFFFFF


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)                    # (NaN and -0 included)


def _run_case(d, dtype, sel=None, id0=None):
    """The kernel on case inputs `d` (all patients, or patient `sel` alone) -> (moved aux, pstats) as numpy arrays."""
    pick = (lambda a: a) if sel is None else (lambda a: a[sel:sel + 1])
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)                     # noqa: E731
    aux = dev(pick(d["aux"]), dtype)
    pstats = hode.capi.pf_params(dev(pick(d["lw"]), torch.float64), aux, dev(d["mode"], torch.int32), dev(d["walk"], torch.float64),
                                 dev(pick(d["dt"]), torch.float64), d["step"], d["shrink"], seed=d["seed"],
                                 id0=d["id0"] if id0 is None else id0)
    torch.cuda.synchronize()
    return aux.cpu().numpy(), pstats.cpu().numpy()


def _check_patient(aux, pstats, d, b, ref, dtype, what, aux_in=None):
    """One patient's kernel output against the restatement `ref` of the same inputs."""
    bd = PC.bounds(d, b, ref)
    aux_in = (d["aux"][b] if aux_in is None else aux_in).astype(NP[dtype])
    assert np.array_equal(np.isnan(pstats), np.isnan(ref["pstats"])), what + " which pstats are NaN"
    moved = ~np.isnan(ref["phi_new"])
    assert np.array_equal(_bits(aux[~moved]), _bits(aux_in[~moved])), what + " untouched entries"
    worst = 0.0
    for k, o in bd.items():
        em, ev = abs(pstats[2 * k] - ref["pstats"][2 * k]), abs(pstats[2 * k + 1] - ref["pstats"][2 * k + 1])
        worst = max(worst, em / o["mean"], ev / o["var"] if o["var"] > 0 else 0.0)
        assert em <= o["mean"] and ev <= o["var"], (what, k, em, o["mean"], ev, o["var"])
        if "value_abs" in o and moved[:, k].any():
            rows = moved[:, k]
            want64 = ref["aux"][rows, k]
            got = aux[rows, k].astype(np.float64)
            if dtype == torch.float64:
                tol = o["value_abs"] + o["value_rel"] * np.abs(want64)
                worst = max(worst, float((np.abs(got - want64) / tol).max()))
                assert (np.abs(got - want64) <= tol).all(), (what, k)
            else:
                want = want64.astype(np.float32)
                assert (np.abs(got - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), (what, k)
            assert (got != aux_in[rows, k]).mean() > 0.9 or rows.sum() < 8, (what, k, "nothing moved")
    return worst


# ------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", range(len(PC.CASES)), ids=[PC.case_id(c) for c in PC.CASES])
def test_parameter_move_against_the_restatement(idx, dtype):
    d, refs = PC.inputs(idx), PC.reference(idx)
    aux, pstats = _run_case(d, dtype)
    worst = 0.0
    for b, ref in enumerate(refs):
        worst = max(worst, _check_patient(aux[b], pstats[b], d, b, ref, dtype, f"case {PC.case_id(d)} patient {b}"))
    print("worst error / bound", worst)
    c = PC.CASES[idx]
    if c["edge"] == "patient_dead":                                  # the dead patient: all NaN, nothing moved; its neighbours moved
        assert np.isnan(pstats[1]).all() and np.array_equal(aux[1], d["aux"][1].astype(NP[dtype]))
        assert np.isfinite(pstats[0][2 * np.nonzero(d["mode"])[0]]).all()
    if c["edge"] == "nonpos":
        k = np.nonzero(d["mode"] == PR.LOG)[0][0]
        assert aux[0, c["N"] // 3, k] == 0.0 and not refs[0]["counts"][c["N"] // 3]
    if c["move"] == "walk" and np.count_nonzero(d["mode"]) > 1:     # a selected column with a = 1 and walk = 0: pstats, no move
        k = np.nonzero(d["mode"])[0][1]
        assert np.array_equal(aux[..., k], d["aux"][..., k].astype(NP[dtype])) and np.isfinite(pstats[0, 2 * k])


_DET = [c["idx"] for c in PC.CASES if c["B"] == 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", _DET, ids=[PC.case_id(PC.CASES[i]) for i in _DET])
def test_parameter_move_is_deterministic_and_independent_of_the_batch(idx, dtype):
    """The same call twice gives the same bits; patient 2 of B = 3 gives the bits of that patient alone with id0 + 2."""
    d = PC.inputs(idx)
    a, b = _run_case(d, dtype), _run_case(d, dtype)
    alone = _run_case(d, dtype, sel=2, id0=d["id0"] + 2)
    for k in range(2):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        assert np.array_equal(_bits(a[k][2:3]), _bits(alone[k])), k


def test_capi_rejects_what_the_kernel_cannot_take():
    f64 = dict(dtype=torch.float64, device=DEV)
    lw, aux = torch.zeros(2, 8, **f64), torch.ones(2, 8, 3, device=DEV)
    mode, walk, dt = torch.ones(3, dtype=torch.int32, device=DEV), torch.zeros(3, **f64), torch.ones(2, **f64)
    hode.capi.pf_params(lw, aux, mode, walk, dt, 0, 0.9)
    for bad in (dict(lw=lw.float()), dict(aux=aux[:, :, :2]), dict(mode=mode.long()), dict(walk=walk[:2]), dict(dt=dt[:1]),
                dict(shrink=1.5), dict(aux=torch.ones(2, 8, 18, device=DEV)), dict(out=torch.empty(2, 5, **f64))):
        kw = dict(lw=lw, aux=aux, mode=mode, walk=walk, dt=dt, step=0, shrink=0.9)
        kw.update(bad)
        with pytest.raises(hode.capi.HodeError):
            hode.capi.pf_params(**kw)


# ------------------------------------------------------------------ 2. run_filter(learn=...) end to end
from test_filter_gpu import B, N, T, _check_states, _data, _model, _rtol  # noqa: E402  (the small networks and their data)


@pytest.fixture(scope="module", params=["relu64x4", "tanh32x2"])
def setup(request):
    m = _model(request.param)
    data, sigma, truth = _data(m)
    return m, data, sigma, truth


def _learn(**kw):
    from inference import ParameterLearning
    return ParameterLearning(["k_I", "ode_a_GI", "k_L"], **dict(dict(discount=0.95, walk=[0.2, 0.0, 0.1], link="log"), **kw))


def _rows(spread=0.2):
    """Initial rows through ode_sets: a cloud around the model's value for each learned constant."""
    g = torch.Generator().manual_seed(17)
    return {"k_I": 0.025 * torch.exp(spread * torch.randn(B, N, generator=g)), "a_GI": 0.0104 * torch.exp(spread * torch.randn(N, generator=g)),
            "k_L": 0.02 * torch.exp(spread * torch.randn(B, N, generator=g))}


def test_run_filter_with_learn_equals_a_loop_of_solves_and_restated_steps_and_moves(setup):
    """Every step of run_filter(learn=...) against model.forward's solve over the segment with each particle's moved constants,
    then the step restatement, then the parameter restatement -- each fed with run_filter's own particles and rows of the step
    before (so that each step is held to the kernel tolerances, not to their compound)."""
    from inference import run_filter
    from models.ode_core import ODE_PARAM_NAMES
    model, data, sigma, _ = setup
    q, q0, seed = 0.04, 0.1, 5
    learn = _learn()
    res = run_filter(model, data, n_particles=N, process_noise=q, initial_spread=q0, noise_sigma=sigma, ess_threshold=0.5, seed=seed,
                     store_particles=True, ode_sets=_rows(), learn=learn)
    idxs = res.step_index.tolist()
    assert idxs == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    assert res.learned.names == ["k_I", "a_GI", "k_L"] and res.learned.location.shape == (B, len(idxs), 3)
    cols = [ODE_PARAM_NAMES.index(n) for n in res.learned.names]
    mode, walk = np.zeros(17, dtype=np.int32), np.zeros(17)
    mode[cols], walk[cols] = PR.LOG, learn.walk
    t, meal, obs = data["time_points"], data["external_inputs"]["meal"], data["observations"].cpu().numpy().astype(np.float64)
    nn_flat, ode_vec = model._params_on(torch.device(DEV))
    ode0 = ode_vec.detach().float().reshape(1, 1, 17).repeat(B, N, 1)
    for name, v in _rows().items():
        ode0[:, :, ODE_PARAM_NAMES.index(name)] = v.to(DEV).expand(B, N)
    hist, ancs, odeh = res.history.cpu().numpy(), res.ancestors.cpu().numpy(), res.ode_history.cpu().numpy()
    lw = np.zeros((B, N))
    x_prev, ode_prev = data["initial_state"].reshape(B, 1, 6).repeat(1, N, 1), ode0
    resampled, worst = 0, 0.0
    for s, g in enumerate(idxs):
        if s == 0:
            x_in, status, dt, qs = x_prev.cpu().numpy().astype(np.float64), np.zeros((B, N), np.int32), np.ones(B), np.full(6, q0)
        else:
            p = idxs[s - 1]
            y = model._solve(x_prev.reshape(B * N, 6), t[p:g + 1], {"meal": meal[:, p:g + 1].repeat_interleave(N, 0)}, "dopri5", 1e-6, 1e-8,
                             n_sets=B * N, nn_flat=nn_flat.detach().float().contiguous(), ode_vec=ode_prev.reshape(-1), nn_shared=True)
            x_in = y[:, -1].reshape(B, N, 6).cpu().numpy().astype(np.float64)
            status = model.last_solve_info["status"].view(B, N).cpu().numpy()
            dt, qs = np.full(B, float(t[g].double() - t[p].double())), np.full(6, q)
        rows = ode_prev.cpu().numpy().astype(np.float64)
        a = learn.shrink if np.isfinite(obs[:, g]).any() else 1.0
        for b in range(B):
            ref = FR.step(x_in[b], obs[b, g], sigma, qs, dt[b], lw[b], s, seed=seed, key=b, link=1, ess_frac=0.5, status=status[b], aux=rows[b])
            assert ref["tie"] > N * 2.0 ** -50, (s, b, ref["tie"])
            what = f"step {s} (grid {g}) patient {b}"
            assert np.array_equal(ancs[s, b], ref["anc"]), what
            _check_states(hist[s, b], ref["x_out"], torch.float32, what)
            mv = PR.move(ref["lw"], ref["aux_out"], mode, walk, dt[b], a, s, seed=seed, key=b)
            d = {"N": N, "shrink": a, "mode": mode, "aux": {b: ref["aux_out"]}}
            pst = np.full(34, np.nan)
            pst[2 * np.array(cols)] = res.learned.location[b, s].cpu().numpy()
            # the result holds the standard deviation: its square carries the roundings of the root and of the square, < 4 * 2^-52
            # relatively, on top of the variance's bound; checked here, and _check_patient is given the restatement's variance
            var = res.learned.scale[b, s].cpu().numpy() ** 2
            for n, k in enumerate(cols):
                want = mv["pstats"][2 * k + 1]
                assert abs(var[n] - want) <= PC.bounds(d, b, mv)[k]["var"] + 4 * 2.0 ** -52 * want, (what, k)
                pst[2 * k + 1] = want
            worst = max(worst, _check_patient(odeh[s, b], pst, d, b, mv, torch.float32, what, aux_in=ref["aux_out"]))
            lw[b] = ref["lw"]
            resampled += int(ref["stats"][2])
        x_prev, ode_prev = res.history[s], res.ode_history[s]
    print("worst error / bound", worst)
    assert 0 < resampled < B * len(idxs)                            # both branches were taken
    np.testing.assert_allclose(res.log_weights.cpu().numpy(), lw, rtol=_rtol(N), atol=0.0)
    assert torch.equal(res.ode_p, res.ode_history[-1])
    # the column without a walk moved too (shrinkage), every value of a learned column is distinct, the others were only gathered
    for j in cols:
        assert (torch.unique(res.ode_p[0, :, j]).numel() == N), j
    others = [j for j in range(17) if j not in cols]
    assert (res.ode_p[:, :, others] == ode0[:, :, others]).all()
    med, (lo, hi) = res.learned.median(), res.learned.interval(0.9)
    assert torch.equal(med, res.learned.location.exp()) and (lo < med).all() and (med < hi).all()
    z = 1.6448536269514722
    np.testing.assert_allclose(hi.cpu().numpy(), (res.learned.location + z * res.learned.scale).exp().cpu().numpy(), rtol=1e-12)
    with pytest.raises(ValueError, match="learn"):
        res.smooth()
    sm, ss = res.smoothed()
    assert torch.isfinite(sm).all() and torch.isfinite(ss).all()


def test_the_initial_spread_is_one_random_walk_move_at_the_first_grid_point(setup):
    """discount = 1 and no walk: after step 0 nothing moves any more; without resampling the final rows are the model's value
    spread once, with the draws of the step number 0xFFFFFFFF, dt = 1."""
    from inference import ParameterLearning, run_filter
    model, data, sigma, _ = setup
    spread = [0.002, 0.3]
    learn = ParameterLearning(["k_I", "G_b"], discount=1.0, initial_spread=spread, link="identity")
    res = run_filter(model, data, n_particles=N, process_noise=0.04, noise_sigma=sigma, ess_threshold=0.0, seed=8, learn=learn)
    base = model.ode_core.param_vector().double().cpu().numpy()
    mode, walk = np.zeros(17, dtype=np.int32), np.zeros(17)
    mode[[1, 3]], walk[[1, 3]] = PR.IDENTITY, spread
    for b in range(B):
        mv = PR.move(np.zeros(N), np.tile(base, (N, 1)), mode, walk, 1.0, 1.0, SPREAD_STEP, seed=8, key=b, dtype=np.float32)
        got = res.ode_p[b].cpu().numpy()
        assert (np.abs(got.astype(np.float64) - mv["aux"].astype(np.float64)) <= np.spacing(np.abs(mv["aux"]))).all()
        assert np.array_equal(np.delete(got, [1, 3], 1), np.delete(np.tile(base.astype(np.float32), (N, 1)), [1, 3], 1))
    # step 0 reports the cloud after the spread, under the weights of step 0 (which the constants have not influenced yet): its
    # sd is the spread's, within 5 standard errors of a weighted sample of that effective size
    sc, ess = res.learned.scale[:, 0].cpu().numpy(), res.ess[:, 0].cpu().numpy()
    assert (np.abs(sc / np.array(spread) - 1) < 5 / np.sqrt(2 * ess)[:, None]).all()
    assert torch.equal(res.learned.median(), res.learned.location)


def test_learn_that_moves_nothing_is_bit_identical_to_learn_none(setup):
    from inference import ParameterLearning, run_filter
    model, data, sigma, _ = setup
    kw = dict(n_particles=N, process_noise=0.04, noise_sigma=sigma, seed=3, ode_sets={"a_GI": torch.linspace(0.009, 0.012, N)})
    plain = run_filter(model, data, **kw)
    still = run_filter(model, data, learn=ParameterLearning(["a_GI", "k_I"], discount=1.0, walk=0.0, initial_spread=0.0), **kw)
    bits = lambda v: v.cpu().numpy().tobytes()                                                              # noqa: E731
    for name in ("particles", "log_weights", "ode_p", "mean", "std", "ess", "log_evidence_steps", "alive", "resampled"):
        assert bits(getattr(plain, name)) == bits(getattr(still, name)), name
    assert plain.learned is None and torch.isfinite(still.learned.location).all()


def test_forecast_of_a_learning_run_equals_trailing_nan_rows(setup):
    """Bit for bit, the learned cloud included; the forecast only walks (a = 1), so the cloud of the walking constant widens."""
    from inference import run_filter
    model, data, sigma, _ = setup
    cut = 9
    obs = data["observations"].clone()
    obs[:, cut:] = float("nan")
    kw = dict(n_particles=N, process_noise=0.04, noise_sigma=sigma, seed=11, ode_sets=_rows(), learn=_learn(walk=[0.5, 0.0, 0.1]))
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
    for name in ("location", "scale"):
        assert bits(getattr(full.learned, name)[:, -1:]) == bits(getattr(tail.learned, name)), name
        assert bits(getattr(full.learned, name)[:, :-1]) == bits(getattr(head.learned, name)), name
    # a second forecast from the first: the walking constant's cloud is wider than where the forecast began, the others' is kept
    # to the sampling error of a gather-free step
    more = tail.forecast(torch.linspace(float(data["time_points"][-1]), float(data["time_points"][-1]) + 1.0, 3, device=DEV))
    assert (more.learned.scale[:, -1, 0] > head.learned.scale[:, -1, 0]).all()
    with pytest.raises(ValueError):
        tail.smooth()


def test_learn_in_fp64_and_on_per_patient_grids(setup):
    """The fp64 path and a per-patient [B, T] grid run the same loop: the learned clouds agree with the fp32 / shared-grid run."""
    from inference import run_filter
    model, data, sigma, _ = setup
    kw = dict(n_particles=N, process_noise=0.04, noise_sigma=sigma, seed=6, ess_threshold=0.0, ode_sets=_rows(), learn=_learn())
    a = run_filter(model, data, **kw)
    b = run_filter(model, dict(data, time_points=data["time_points"].expand(B, T).contiguous()), **kw)
    c = run_filter(model, data, dtype=torch.float64, **kw)
    assert c.ode_p.dtype == torch.float64 and torch.isfinite(c.learned.location).all()
    np.testing.assert_allclose(b.learned.location.cpu().numpy(), a.learned.location.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(c.learned.location.cpu().numpy(), a.learned.location.cpu().numpy(), rtol=2e-3, atol=1e-3)
    np.testing.assert_allclose(c.mean.cpu().numpy(), a.mean.cpu().numpy(), rtol=2e-3, atol=1e-3)


# ------------------------------------------------------------------ 3. what it is for
def test_a_wrong_constant_is_learned_from_the_record():
    """Records simulated by the model with V_max (the GLP-1 secretion capacity) scaled by 1.5, all six states observed, T = 25,
    N = 256; `learn` on V_max starts from the model's value with an initial spread.  The final median is closer to the truth
    than the start in every patient, and all N final values are distinct.
    (The GLP-1 clearance k_L was tried first: over this grid its term is a few per cent of GLP-1's rate of change, and in 25
    points its median did not move towards the truth in two of three patients -- error ratios 0.61, 1.18, 1.20.)"""
    from inference import ParameterLearning, run_filter
    model = _model("relu64x4")
    g = torch.Generator(device=DEV).manual_seed(4)
    Tn, Np, name, factor = 25, 256, "V_max", 1.5
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
    res = run_filter(model, data, n_particles=Np, process_noise=0.02, initial_spread=0.02, noise_sigma=sigma, seed=1,
                     learn=ParameterLearning([name], discount=0.98, initial_spread=0.5))
    med = res.learned.median()[:, -1, 0].cpu().numpy()
    err0, err = abs(start - factor * start), np.abs(med - factor * start)
    print(f"{name}: truth {factor * start:.5f}, start {start:.5f}, final medians {med}, error ratio {err / err0}")
    assert (err < err0).all()
    j = 8                                                             # V_max's column
    for b in range(B):
        assert torch.unique(res.ode_p[b, :, j]).numel() == Np
