"""The EM noise fit's kernels (csrc/hode_ukf_em.hip) and inference.fit_ukf_noise on the GPU, held to the numpy restatement of
tests/_ukf_em_reference.py.  `-m gpu`.

Tolerances against the restatement.  Every kernel is fed the restatement's own inputs (the smoothed
moments, the factor, the propagated rows rounded to the data type), so no bound is a compound.  The orders of all sums are the
restatement's; what differs is the device's log and exp.  With c = the condition number of the smoothed covariance of the pair's
first step on its non-zero columns, from the restatement (tests/test_ukf_em_host.py keeps c <= 1e6), and bound = 64 n c 2^-52:
  x_em, aux_em       fp64 within bound relative; fp32 within one ulp of the restatement's value rounded to fp32;
  chol               within bound of the largest magnitude in the factor;
  e2                 within bound of the largest magnitude among the terms it sums (the restatement's `scale`);
  r2                 within 64 n 2^-52 of the larger of its two terms (no factor enters it);
  sums, new values   within 64 n 2^-52 times the number of addends, relative (fed the same e2 / r2, the sums have one order);
  counts, pair_ok, seen, the NaN pattern, values that are not fitted and values at their floor: bit for bit.
Every comparison prints `UKF_FRACTION em-<what> <worst error / bound>`."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

import _ukf_cases as UC  # noqa: E402
import _ukf_em_cases as EC  # noqa: E402
import _ukf_em_reference as ER  # noqa: E402
import _ukf_reference as UR  # noqa: E402

DEV = "cuda"
NP = {torch.float32: np.float32, torch.float64: np.float64}
EPS = 2.0 ** -52
bits = lambda v: np.ascontiguousarray(v).view(np.uint8)                                 # noqa: E731  (NaN and -0 included)
f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)                         # noqa: E731
i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)                           # noqa: E731
host = lambda t: t.cpu().numpy()                                                        # noqa: E731


def _points(c, dtype):
    out = hode.capi.ukf_em_points(f64(c["mean_s"]), f64(c["cov_s"]), i32(c["alive"]),
                                  torch.as_tensor(np.ascontiguousarray(c["ode"]), dtype=dtype, device=DEV), c["mode"], c["w"], link=c["link"])
    torch.cuda.synchronize()
    return dict(zip(("x_em", "aux_em", "chol"), (host(v) for v in out)))


def _stats(c, dtype):
    real = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)                             # noqa: E731
    mask = None if c["mask"] is None else torch.as_tensor(np.ascontiguousarray(c["mask"]), device=DEV)
    out = hode.capi.ukf_em_stats(real(c["prop"]), i32(c["status"]), f64(c["chol"]), f64(c["mean_s"]), f64(c["cov_s"]), f64(c["gain"]),
                                 i32(c["alive"]), real(c["obs"]), mask, f64(c["moments"]), c["mode"], c["w"], link=c["link"])
    torch.cuda.synchronize()
    return dict(zip(("e2", "pair_ok", "r2", "seen"), (host(v) for v in out)))


def _mstep(c, fit_mask=None, floor=None):
    q, walk, sigma = f64(c["q"]), f64(c["walk"]), f64(c["sigma"])
    sums = hode.capi.ukf_em_mstep(f64(c["e2"]), i32(c["pair_ok"]), f64(c["r2"]), i32(c["seen"]), f64(c["dt"]), q, walk, sigma, c["mode"],
                                  c["fit_mask"] if fit_mask is None else fit_mask, c["floor"] if floor is None else floor, link=c["link"])
    torch.cuda.synchronize()
    return dict(sums=host(sums), q=host(q), walk=host(walk), sigma=host(sigma))


class _Worst:
    def __init__(self):
        self.value = 0.0

    def hold(self, what, err, bound):
        self.value = max(self.value, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


# ------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", range(len(EC.SPECS)), ids=[EC.case_id(s) for s in EC.SPECS])
def test_points_and_stats_kernels_against_the_restatement(idx, dtype):
    spec, c = EC.SPECS[idx], EC.case(idx)
    S, B, n, K = c["S"], c["B"], c["n"], c["K"]
    pts, st = _points(c, dtype), _stats(c, dtype)
    assert pts["x_em"].shape == (S - 1, B * K, 6) and pts["aux_em"].shape == (S - 1, B * K, 17) and pts["chol"].shape == (S - 1, B, n, n)
    assert st["e2"].shape == (S - 1, B, n) and st["r2"].shape == (S, B, 6) and pts["x_em"].dtype == NP[dtype]
    w = _Worst()
    for s in range(S - 1):
        for b in range(B):
            rows, what = slice(b * K, (b + 1) * K), f"case {EC.case_id(spec)} pair {s} patient {b}"
            x, aux, L = pts["x_em"][s, rows], pts["aux_em"][s, rows], pts["chol"][s, b]
            if not c["alive"][s + 1, b]:                                # a pair into a dead step: rows a solve can take
                assert (x == 1).all() and np.array_equal(bits(aux), bits(np.tile(c["ode"][s, b, 0].astype(NP[dtype]), (K, 1)))), what
                assert np.isnan(L).all() and np.isnan(st["e2"][s, b]).all() and st["pair_ok"][s, b] == 0, what
                continue
            bound = 64 * n * c["cond"][s, b] * EPS
            for name, got, ref in (("x_em", x, c["x_em"][s, rows]), ("aux_em", aux, c["aux_em"][s, rows])):
                if dtype == torch.float64:
                    w.hold(f"{what} {name}", np.abs(got / ref - 1).max(), bound)
                else:
                    r32 = ref.astype(np.float32)
                    assert (np.abs(got.astype(np.float64) - r32.astype(np.float64)) <= np.spacing(np.abs(r32)).astype(np.float64)).all(), f"{what} {name}"
            w.hold(f"{what} chol", np.abs(L - c["chol"][s, b]).max(), bound * np.abs(c["chol"][s, b]).max())
            assert np.array_equal(L == 0, c["chol"][s, b] == 0), what           # (the zero columns are the restatement's)
            assert st["pair_ok"][s, b] == c["pair_ok"][s, b], what
            if c["pair_ok"][s, b]:
                w.hold(f"{what} e2", np.abs(st["e2"][s, b] - c["e2"][s, b]).max(), bound * c["scale"][s, b])
            else:
                assert np.isnan(st["e2"][s, b]).all(), what
    assert np.array_equal(st["seen"], c["seen"]) and np.array_equal(st["r2"] == 0, c["r2"] == 0)
    for s in range(S):
        for b in range(B):
            for j in range(6):
                if (c["seen"][s, b] >> j) & 1:
                    r = float(c["obs"][b, s, j]) - c["moments"][s, b, j]
                    w.hold(f"r2 step {s} patient {b} state {j}", abs(st["r2"][s, b, j] - c["r2"][s, b, j]), 64 * n * EPS * max(r * r, c["moments"][s, b, 6 + j]))
    print(f"UKF_FRACTION em-kernels-{EC.case_id(spec)}-{NP[dtype].__name__} {w.value:.4f}")
    if idx == EC.STATUS_CASE:
        assert st["pair_ok"][EC.STATUS_PAIR].tolist() == [1, 1, 0, 1, 1]
    if spec.get("edge") == "zero_state":                                # exactly zero: the exact coordinate has no residual
        assert not pts["chol"][:, :, 2, :].any() and not pts["chol"][:, :, :, 2].any() and not st["e2"][:, :, 2].any()


@pytest.mark.parametrize("idx", range(len(EC.SPECS)), ids=[EC.case_id(s) for s in EC.SPECS])
def test_mstep_kernel_against_the_restatement(idx):
    spec, c = EC.SPECS[idx], EC.case(idx)
    got = _mstep(c)
    S, B, n = c["S"], c["B"], c["n"]
    w = _Worst()
    at = hode.capi.UKF_EM_SUM_AT
    assert np.array_equal(bits(got["sums"][[at["N"]]]), bits(c["sums"][[at["N"]]])) and np.array_equal(bits(got["sums"][at["M"]]), bits(c["sums"][at["M"]]))
    assert not got["sums"][n:23].any()
    addends = max((S - 1) * B, S * B)
    w.hold("sums", np.abs(got["sums"] - c["sums"]).max() if not np.array_equal(got["sums"], c["sums"]) else 0.0,
           64 * n * EPS * addends * np.abs(c["sums"]).max())
    for name, ref, old in (("q", c["new_q"], c["q"]), ("walk", c["new_walk"], c["walk"]), ("sigma", c["new_sigma"], c["sigma"])):
        same = ref == old                                               # not fitted, exactly zero, nothing counted: the bits stay
        assert np.array_equal(bits(got[name][same]), bits(old[same])), name
        if (~same).any():
            w.hold(name, np.abs(got[name][~same] / ref[~same] - 1).max(), 64 * n * EPS * addends)
    if S > 1:
        assert got["q"][0] == 10.0                                      # the floor, bit for bit
    print(f"UKF_FRACTION em-mstep-{EC.case_id(spec)} {w.value:.4f}")
    off = _mstep(c, fit_mask=np.zeros(ER.FIT, dtype=np.int32))          # a fit_mask of zeros: the sums, and nothing else
    assert np.array_equal(bits(off["sums"]), bits(got["sums"]))
    for name in ("q", "walk", "sigma"):
        assert np.array_equal(bits(off[name]), bits(c[name])), name


def test_mstep_sums_many_patients_in_the_fixed_shape():
    """B = 700 patients (more than the 256 slots, not a multiple of them) x S = 3: the restatement's slot order, to the last bit."""
    rng = np.random.default_rng(5)
    S, B, n = 3, 700, 6
    c = dict(e2=rng.random((S - 1, B, n)) * 10.0 ** rng.integers(-6, 3, (S - 1, B, n)), pair_ok=(rng.random((S - 1, B)) < 0.8).astype(np.int32),
             r2=rng.random((S, B, 6)), seen=rng.integers(0, 64, (S, B)).astype(np.int32), dt=0.5 + rng.random((S, B)),
             q=np.full(6, 0.05), walk=np.zeros(17), sigma=np.full(6, 0.3), mode=np.zeros(17, dtype=np.int32), link=1)
    c["e2"][c["pair_ok"] == 0] = np.nan
    ones, floor = np.ones(ER.FIT, dtype=np.int32), np.full(ER.FIT, 1e-6)
    got, ref = _mstep(c, ones, floor), ER.reduce(c["e2"], c["pair_ok"], c["r2"], c["seen"], c["dt"])
    assert np.array_equal(bits(got["sums"]), bits(ref))
    q, walk, sigma = ER.mstep(ref, c["q"], c["walk"], c["sigma"], c["mode"], ones, floor, link=1)
    assert np.abs(got["q"] / q - 1).max() <= 8 * EPS and np.abs(got["sigma"] / sigma - 1).max() <= 8 * EPS and not got["walk"].any()
    with pytest.raises(hode.capi.HodeError, match="positive"):
        _mstep(dict(c, dt=np.where(np.arange(S)[:, None] == 1, 0.0, c["dt"])), ones, floor)


# ------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("idx", [0, 4], ids=[EC.case_id(EC.SPECS[i]) for i in (0, 4)])
def test_em_kernels_are_deterministic_and_independent_of_the_batch(idx, dtype):
    """The same call twice gives the same bits; patient 2 of B = 3 gives the bits of that patient alone (n = 6 and n = 23)."""
    c = EC.case(idx)
    assert c["B"] == 3 and c["n"] == (6, 23)[idx == 4]
    alone = EC.select(c, 2)
    for run, keys in ((_points, ("x_em", "aux_em", "chol")), (_stats, ("e2", "pair_ok", "r2", "seen"))):
        a, b, one = run(c, dtype), run(c, dtype), run(alone, dtype)
        for k in keys:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
            sel = a[k][:, 2 * c["K"]:3 * c["K"]] if k in ("x_em", "aux_em") else a[k][:, 2:3]
            assert np.array_equal(bits(sel), bits(one[k])), k
    a, b = _mstep(c), _mstep(c)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


# ------------------------------------------------------------------ 3. what the binding refuses
def test_capi_rejects_what_the_kernels_cannot_take():
    c = EC.case(0)
    S, B, n, K = c["S"], c["B"], c["n"], c["K"]
    pts = dict(mean_s=f64(c["mean_s"]), cov_s=f64(c["cov_s"]), alive=i32(c["alive"]), ode_history=f64(c["ode"]).float(), mode=c["mode"], weights=c["w"])
    for change in (dict(mean_s=pts["mean_s"][..., :-1].contiguous()), dict(mode=UC.mode_of(1)), dict(cov_s=pts["cov_s"].float()),
                   dict(alive=pts["alive"].long()), dict(ode_history=pts["ode_history"][:, :, :-1].contiguous()), dict(ode_history=pts["ode_history"].cpu()),
                   dict(out=(torch.empty(S - 1, B * K, 6, device=DEV), torch.empty(S - 1, B * K, 17, device=DEV), pts["cov_s"][:-1]))):
        with pytest.raises(hode.capi.HodeError):
            hode.capi.ukf_em_points(**dict(pts, **change))
    real = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)                      # noqa: E731
    st = dict(prop_em=real(c["prop"]), status=i32(c["status"]), chol=f64(c["chol"]), mean_s=pts["mean_s"], cov_s=pts["cov_s"], gain=f64(c["gain"]),
              alive=pts["alive"], obs=real(c["obs"]), mask=None, moments=f64(c["moments"]), mode=c["mode"], weights=c["w"])
    for change in (dict(prop_em=st["prop_em"][:, :-1].contiguous()), dict(obs=st["obs"].double()), dict(obs=st["obs"].transpose(0, 1).contiguous()),
                   dict(mask=torch.ones(B, S, 6, dtype=torch.int32, device=DEV)), dict(status=st["status"].long()), dict(gain=st["gain"][1:]),
                   dict(moments=st["moments"][..., :6].contiguous()), dict(chol=st["chol"].cpu())):
        with pytest.raises(hode.capi.HodeError):
            hode.capi.ukf_em_stats(**dict(st, **change))
    ms = dict(e2=f64(c["e2"]), pair_ok=i32(c["pair_ok"]), r2=f64(c["r2"]), seen=i32(c["seen"]), dt=f64(c["dt"]), q=f64(c["q"]), walk=f64(c["walk"]),
              sigma=f64(c["sigma"]), mode=c["mode"], fit_mask=c["fit_mask"], floor=c["floor"])
    for change in (dict(fit_mask=c["fit_mask"][:-1]), dict(floor=-c["floor"]), dict(q=ms["q"][:5].contiguous()), dict(walk=ms["walk"].float()),
                   dict(dt=ms["dt"][1:]), dict(seen=ms["seen"].long()), dict(sums=ms["q"]), dict(sums=torch.empty(36, dtype=torch.float64, device=DEV))):
        with pytest.raises(hode.capi.HodeError):
            hode.capi.ukf_em_mstep(**dict(ms, **change))
    lib = hode.load()                                                   # the new ground: none of this exists in the parent
    assert all(hasattr(lib, sym) for sym in hode.capi.EXT_SYMBOLS["hode_ukf_em.h"])


# ------------------------------------------------------------------ 4. linear models on the device
def _device_estep(M, ys, q, walk, sigma):
    """The filter as tests/test_ukf_smooth_gpu.py runs it on the records ys [B, S, 6] -- x_in = A chi_x + Bm chi_theta formed in
    torch (fp64) from the kernel's own rows --, the smoother, and one E-step through the kernels, the propagation of the kernel's
    own x_em formed the same way.  Returns the four statistics and the summed evidence."""
    w = hode.capi.ukf_weights(M["n"])
    A, Bm = f64(M["A"]), f64(M["Bm"])
    n, K, cols, S, B = M["n"], 2 * M["n"] + 1, M["cols"], M["S"], len(ys)
    x, aux = torch.zeros(B, K, 6, dtype=torch.float64, device=DEV), torch.ones(B, K, 17, dtype=torch.float64, device=DEV)
    mean, cov = f64(np.tile(M["m0"], (B, 1))), f64(np.tile(M["P0"], (B, 1, 1)))
    alive = torch.ones(B, dtype=torch.int32, device=DEV)
    hist, odeh, prop, meanh, covh, aliveh, ev = [], [], [], [], [], [], 0.0
    obs = f64(ys)
    for s in range(S):
        if s > 0:
            x = (x @ A.T + aux[:, :, cols] @ Bm.T).contiguous()
        prop.append(x)
        x, aux, stats = hode.capi.ukf_step(x, aux, M["mode"], obs[:, s].contiguous(), sigma, q, walk, f64(np.full(B, M["dts"][s])), alive, mean, cov, w,
                                           predict=s > 0, link=0)
        ev = ev + stats[:, 0].sum()
        hist.append(x), odeh.append(aux), meanh.append(mean.clone()), covh.append(cov.clone()), aliveh.append(alive.clone())
    st = lambda v: torch.stack(v).contiguous()                                                                     # noqa: E731
    dt = f64(np.repeat(M["dts"][:S, None], B, axis=1))
    mean_s, cov_s, gain, _, _, mo = hode.capi.ukf_smooth(st(hist), st(odeh), st(prop), st(meanh), st(covh), st(aliveh), M["mode"], q, walk, dt, w, link=0)
    x_em, aux_em, chol = hode.capi.ukf_em_points(mean_s, cov_s, st(aliveh), st(odeh), M["mode"], w, link=0)
    prop_em = (x_em @ A.T + aux_em[:, :, cols] @ Bm.T).contiguous()
    status = torch.zeros(S - 1, B * K, dtype=torch.int32, device=DEV)
    out = hode.capi.ukf_em_stats(prop_em, status, chol, mean_s, cov_s, gain, st(aliveh), obs.contiguous(), None, mo, M["mode"], w, link=0)
    return out, dt, ev


@pytest.mark.parametrize("which", [1, 2])
def test_identity_link_on_the_device_gives_the_exact_smoother_statistic(which):
    M = UC.linear_model(which)
    (e2, pair_ok, r2, seen), _, _ = _device_estep(M, M["ys"][None], f64(M["q"]), f64(M["walk"]), f64(M["sigma"]))
    want_e2, want_r2, scale = EC.exact_statistics(M, M["ys"])
    assert bool(pair_ok.all())
    err_e2 = max(np.abs(host(e2)[s, 0] - want_e2[s]).max() / scale[s] for s in range(M["S"] - 1))
    err_r2 = np.abs(host(r2)[:, 0] - want_r2).max() / np.abs(want_r2).max()
    print(f"model {which} on the device: e2 {err_e2:.2e}, r2 {err_r2:.2e} of the largest term")
    assert err_e2 <= 1e-10 and err_r2 <= 1e-10


def test_five_iterations_on_the_device_raise_the_exact_evidence():
    """Records simulated from model 1 (B = 6, S = 40), q started a factor of 3 and sigma a factor of 1/2 off: five iterations through
    the three kernels; the exact Kalman evidence at each iteration's values never falls (slack 1e-9 |l|)."""
    M, ys = EC.simulate(UC.linear_model(1), S=40, B=6, seed=77)
    q, walk, sigma = f64(3.0 * M["q"]), f64(M["walk"]), f64(0.5 * M["sigma"])
    fit_mask, floor = np.array([1] * 6 + [0] * 17 + [1] * 6, dtype=np.int32), np.full(ER.FIT, 1e-6)
    ev, dev_ev = [], []
    for it in range(6):
        ev.append(EC.evidence(dict(M, q=host(q).copy(), sigma=host(sigma).copy()), ys))
        (e2, pair_ok, r2, seen), dt, lev = _device_estep(M, ys, q, walk, sigma)
        dev_ev.append(float(lev))
        if it < 5:
            sums = hode.capi.ukf_em_mstep(e2, pair_ok, r2, seen, dt, q, walk, sigma, M["mode"], fit_mask, floor, link=0)
            assert float(sums[ER.AT_N]) == 6 * 39
    print("evidence:", " ".join(f"{v:.4f}" for v in ev))
    for a, b in zip(ev, ev[1:]):
        assert b >= a - 1e-9 * abs(a), (a, b)
    assert ev[-1] > ev[0] + 10.0 and np.abs(np.array(dev_ev) - np.array(ev)).max() <= 1e-8 * abs(ev[0])       # (the filter's own evidence is it)


# ------------------------------------------------------------------ 5. fit_ukf_noise end to end
from test_ukf_gpu import B, LINKS, T, _data, _model  # noqa: E402  (the fixtures of the filter's own end-to-end tests)


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_grouped_solve_gives_the_bits_of_one_solve_per_segment(monkeypatch):
    """B = 3, T = 13, a step at every third grid point: the E-step is ONE forward solve of all pairs' rows, and its last rows are
    those of one solve per segment, bit for bit."""
    from inference import run_ukf
    model = _model("relu64x4")
    data, sigma, _ = _data(model)
    res = run_ukf(model, data, process_noise=0.04, noise_sigma=sigma, steps=[3, 6, 9, 12], store_history=True)
    sm = res.smooth()
    calls, solve = [], hode.solve_fwd
    monkeypatch.setattr(hode, "solve_fwd", lambda *a, **k: (calls.append(a[0].shape[0]), solve(*a, **k))[1])
    st = sm.noise_statistics(data)
    monkeypatch.undo()
    e = res._engine
    K = e.K
    assert calls == [4 * B * K] and st["prop_em"].shape == (4, B * K, 6) and bool(st["pair_ok"].all())
    nn_flat, _ = model._params_on(e.dev)
    nn_flat = nn_flat.detach().float().contiguous()
    t, meal = data["time_points"], data["external_inputs"]["meal"].repeat_interleave(K, 0)
    for s, (p, g) in enumerate(zip([0, 3, 6, 9], [3, 6, 9, 12])):
        sol = solve(st["x_em"][s], t[p:g + 1].contiguous(), meal[:, p:g + 1].contiguous(), None, None, st["aux_em"][s].reshape(-1), nn_flat, e.H, e.L,
                    method=e.method, rtol=e.rtol, atol=e.atol, n_sets=B * K, nn_shared=True)
        assert _eq(sol.y[:, -1], st["prop_em"][s]) and _eq(sol.status.view(-1), st["status"][s]), s


@pytest.fixture(scope="module", params=["relu64x4", "tanh32x2"])
def setup(request):
    from inference import ParameterLearning
    m = _model(request.param)
    data, sigma, truth = _data(m)
    scale = (truth.abs().mean((0, 1)) + 0.1).double().cpu().numpy()
    link = LINKS[request.param]
    rel = 1.0 if link == "log" else scale
    walk = [0.1, 0.05] if request.param == "relu64x4" else None
    learn = (lambda wk: ParameterLearning(["k_I", "a_GI"], walk=wk, initial_spread=0.2)) if walk else (lambda wk: None)
    kw = dict(initial_spread=0.1 * rel, noise_link=link)
    return m, data, kw, learn, walk, 0.04 * rel * np.ones(6), 2.0 * sigma


def test_fit_ukf_noise(setup):
    from inference import UKFNoiseFit, UKFSmoothResult, fit_ukf_noise, run_ukf
    model, data, kw, learn, walk, q0, sigma0 = setup
    names = ("process_noise", "noise_sigma", "walk") if walk else ("process_noise", "noise_sigma")
    fit = fit_ukf_noise(model, data, process_noise=q0, noise_sigma=sigma0, learn=learn(walk), fit=names, n_iter=3, **kw)
    assert isinstance(fit, UKFNoiseFit) and isinstance(fit.smoothed, UKFSmoothResult)
    tr = fit.trace
    assert tr["process_noise"].shape == (4, 6) and tr["noise_sigma"].shape == (4, 6) and fit.log_evidence.shape == (4,) and fit.sums.shape == (3, 37)
    assert np.array_equal(bits(tr["process_noise"][0]), bits(np.asarray(q0, dtype=np.float64))) and np.array_equal(bits(tr["noise_sigma"][0]), bits(sigma0))
    assert np.array_equal(bits(fit.process_noise), bits(tr["process_noise"][-1])) and np.array_equal(bits(fit.noise_sigma), bits(tr["noise_sigma"][-1]))
    if walk:
        assert tr["walk"].shape == (4, 2) and np.array_equal(tr["walk"][0], np.array(walk)) and np.array_equal(bits(fit.walk), bits(tr["walk"][-1]))
    else:
        assert tr["walk"] is None and fit.walk is None
    assert np.isfinite(fit.log_evidence).all() and (np.diff(tr["noise_sigma"], axis=0) != 0).all() and (np.diff(tr["process_noise"], axis=0) != 0).all()
    print("log-evidence:", fit.log_evidence, "noise_sigma / start:", fit.noise_sigma / sigma0)
    S = len(fit.result.step_index)
    assert fit.pairs_used == B * (S - 1) == fit.sums[-1][ER.AT_N]
    # every row of the trace: the filter at those values is run_ukf's, and the iteration's sums are the restatement's, fed the
    # device's own smoother outputs and propagated rows
    worst = _Worst()
    for i in range(4):
        res = run_ukf(model, data, process_noise=tr["process_noise"][i], noise_sigma=tr["noise_sigma"][i], learn=learn(tr["walk"][i] if walk else None),
                      store_history=True, **kw)
        ev = float(torch.where(res.alive[:, -1], res.log_evidence_steps.sum(1), torch.zeros(B, dtype=torch.float64, device=DEV)).sum())
        assert ev == fit.log_evidence[i], i
        if i == 3:
            for name in ("mean", "std", "nis", "n_seen", "log_evidence_steps", "alive", "step_index", "times", "sigma_points", "ode_p", "state_mean",
                         "state_cov", "history", "ode_history", "propagated_history"):
                assert _eq(getattr(res, name), getattr(fit.result, name)), name
            sm = res.smooth()
            assert _eq(sm.state_mean, fit.smoothed.state_mean) and _eq(sm.state_cov, fit.smoothed.state_cov) and _eq(sm.mean, fit.smoothed.mean)
            break
        sm = res.smooth()
        st = sm.noise_statistics(data)
        assert np.array_equal(bits(host(st["sums"])), bits(fit.sums[i])), i
        e, n, K = res._engine, res.state_mean.shape[1], res.sigma_points.shape[1]
        mean_s, cov_s, gain = (host(v.transpose(0, 1)) for v in (sm.state_mean, sm.state_cov, sm.gain))
        chol, prop, status, alive = host(st["chol"]), host(st["prop_em"]).astype(np.float64), host(st["status"]), host(res.alive.t())
        gi = res.step_index.tolist()
        obs = host(data["observations"])[:, gi].astype(np.float64)
        e2, ok, cond = np.full((S - 1, B, n), np.nan), np.zeros((S - 1, B), dtype=np.int32), 1.0
        r2, seen = np.zeros((S, B, 6)), np.zeros((S, B), dtype=np.int32)
        for b in range(B):
            for s in range(S - 1):
                rows = slice(b * K, (b + 1) * K)
                r = ER.pair(prop[s, rows], status[s, rows], chol[s, b], mean_s[s, b], mean_s[s + 1, b], cov_s[s + 1, b], gain[s, b], alive[s + 1, b],
                            e.weights, e.link)
                e2[s, b], ok[s, b] = r["e2"], r["ok"]
                keep = [j for j in range(n) if chol[s, b][j, j] != 0]
                c_sb = UR._cond(cov_s[s, b][np.ix_(keep, keep)])
                cond = max(cond, c_sb)
                worst.hold(f"iteration {i} e2[{s}, {b}]", np.abs(host(st["e2"])[s, b] - r["e2"]).max(), 64 * n * c_sb * EPS * r["scale"])
            for s in range(S):
                r2[s, b], seen[s, b] = ER.obs(obs[b, s], None, alive[s, b], host(sm._moments)[s, b])
        assert cond <= UC.COND_CAP, cond
        assert np.array_equal(ok, host(st["pair_ok"])) and np.array_equal(seen, host(st["seen"]))
        ref = ER.reduce(e2, ok, r2, seen, host(res.dt_history))
        size = ER.reduce(np.abs(e2), ok, r2, seen, host(res.dt_history))        # (the sum of the addends' magnitudes)
        assert np.array_equal(ref[[ER.AT_N, ER.AT_D]], fit.sums[i][[ER.AT_N, ER.AT_D]]) and np.array_equal(ref[ER.AT_M:], fit.sums[i][ER.AT_M:])
        worst.hold(f"iteration {i} sums", (np.abs(fit.sums[i] - ref) / np.where(size > 0, size, 1.0)).max(), 64 * n * cond * EPS * B * S)
    print(f"UKF_FRACTION em-fit-{kw['noise_link']} {worst.value:.4f}")


def test_fit_ukf_noise_leaves_what_it_may_not_touch(setup):
    from inference import ParameterLearning, fit_ukf_noise
    model, data, kw, learn, walk, q0, sigma0 = setup
    # one iteration whose selected values are exactly zero -- a walk of 0 stays 0 --: the inputs come back, bit for bit
    still = ParameterLearning(["k_I", "a_GI"], walk=0.0, initial_spread=0.2)
    fit = fit_ukf_noise(model, data, process_noise=q0, noise_sigma=sigma0, learn=still, fit=("walk",), n_iter=1, **kw)
    assert np.array_equal(bits(fit.process_noise), bits(np.asarray(q0, dtype=np.float64))) and np.array_equal(bits(fit.noise_sigma), bits(sigma0))
    assert not fit.walk.any() and fit.log_evidence[0] == fit.log_evidence[1] and fit.pairs_used > 0
    # per-state flags: only what is selected moves; an exact state stays exact
    q = np.asarray(q0, dtype=np.float64).copy()
    q[4] = 0.0
    flags = {"process_noise": [True, True, False, True, True, True], "noise_sigma": [False] * 5 + [True]}
    fit = fit_ukf_noise(model, data, process_noise=q, noise_sigma=sigma0, fit=flags, n_iter=2, floor=1e-6, **kw)
    assert fit.process_noise[2] == q[2] and fit.process_noise[4] == 0.0 and (fit.process_noise[[0, 1, 3, 5]] != q[[0, 1, 3, 5]]).all()
    assert np.array_equal(bits(fit.noise_sigma[:5]), bits(sigma0[:5])) and fit.noise_sigma[5] != sigma0[5]
    # a tolerance no iteration meets stops the fit after the second filter
    fit = fit_ukf_noise(model, data, process_noise=q0, noise_sigma=sigma0, n_iter=5, tol=1e9, **kw)
    assert fit.log_evidence.shape == (2,) and fit.trace["noise_sigma"].shape == (2, 6) and fit.sums.shape == (1, 37)
    # refusals
    from inference.observation import ObservationModel
    for bad, match in ((dict(n_iter=0), "n_iter"), (dict(fit=()), "selects nothing"),
                       (dict(noise_sigma=ObservationModel(1.0, noise="marginal")), "marginal")):
        with pytest.raises(ValueError, match=match):
            fit_ukf_noise(model, data, **dict(dict(process_noise=q0, noise_sigma=sigma0, **kw), **bad))
