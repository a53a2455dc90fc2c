"""The tail and quantile kernels of csrc/hode_predictive.hip (include/hode.h, "Posterior bands") against their NumPy
restatement (tests/_quantile_reference.py), in fp32 and fp64, at the shapes of test_predictive_gpu.py (N = 18, under one wave;
N = 390, a ragged wave; N = 3348, fourteen workgroups, the last ragged), with S = 1, 2, 7 and 19 = 16 + 3 draws (the batch of loads
in flight and its remainder), buffers of K = 1, 2, 5, S and S + 3 values, and S = 300 into K = 9 (heaps three levels deep that
overflow hundreds of times); draws in random, ascending and descending order and with ties; an entry without any draw, a
non-finite value, a failed trajectory with zero rows.  `-m gpu`.

Everything is compared EXACTLY: the kernels copy values and compare them, and the interpolation is IEEE fp64 without
contraction rounded once, which NumPy restates bit for bit.  The band table's two sums are fixed-order fp64 sums of
non-negative terms against np.sum: N * 2^-52 relative."""
import os
from functools import lru_cache

import numpy as np
import pytest

import _quantile_reference as QR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

DTYPES = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
LEVELS = (0.025, 0.25, 0.5, 0.9, 0.975)
BAND_LEVELS = (0.025, 0.5, 0.975)
DEV = "cuda"
SENTINEL = -7.0                                                 # what the tests put into the buffers' untouched slots


@lru_cache(maxsize=None)
def case(n_traj, T, S, dt, order):
    return QR.make_case(n_traj, T, S, DTYPES[dt][1], order)


@lru_cache(maxsize=None)
def reference(n_traj, T, S, dt, order, K, levels=LEVELS):
    """Computed once per case and shared (never modified by the tests): cnt, lower, upper, out."""
    c = case(n_traj, T, S, dt, order)
    return QR.quantiles_of(c["y"], levels, K, c["status"], DTYPES[dt][1])


def bits(t):
    if not t.is_floating_point():
        return t
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)       # (NaN == NaN)


def same(got, want, npdt):
    return np.array_equal(got.cpu().numpy(), np.asarray(want).astype(npdt), equal_nan=True)


def run(c, dt, K, splits, levels=LEVELS, offset=False, perm=None, quantiles_after=None):
    """Fold c's draws in the given consecutive pieces; returns the raw state as folded (clones), and after pred_quantiles the
    quantiles, the sorted tails and the state itself."""
    tdt = DTYPES[dt][0]
    S, N = c["y"].shape
    y = torch.tensor(c["y"], dtype=tdt, device=DEV)
    status = torch.tensor(c["status"], device=DEV)
    if perm is not None:
        y, status = y[perm].contiguous(), status[perm].contiguous()
    if offset:                                                  # the same values one element off the allocation's alignment
        buf = torch.empty(S * N + 1, dtype=tdt, device=DEV)
        buf[1:].copy_(y.reshape(-1))
        y = buf[1:].view(S, N)
        assert y.data_ptr() % 16 != 0
    ts = hode.capi.pred_tail_state(N, K, tdt, DEV)
    ts["lo"].fill_(SENTINEL)
    ts["hi"].fill_(SENTINEL)
    for n, (lo, hi) in enumerate(splits):
        hode.capi.pred_tails(y[lo:hi], ts, status[lo:hi])
        if quantiles_after is not None and n == quantiles_after:
            hode.capi.pred_quantiles(ts, levels)
    raw = {k: v.clone() for k, v in ts.items()}
    out, _ = hode.capi.pred_quantiles(ts, levels)
    lower, upper = hode.capi.pred_tail_values(ts)
    return raw, out, lower, upper, ts


def check(got, ref, dt, K):
    raw, out, lower, upper, ts = got
    cnt, rlower, rupper, rout = ref
    npdt = DTYPES[dt][1]
    assert np.array_equal(raw["cnt"].cpu().numpy(), cnt)
    assert same(lower, rlower, npdt) and same(upper, rupper, npdt)
    assert out.dtype == DTYPES[dt][0] and same(out, rout, npdt)
    # slots past min(cnt, K) were never written
    m = torch.tensor(np.minimum(cnt, K), device=DEV).unsqueeze(0)
    untouched = torch.arange(K, device=DEV).unsqueeze(1) >= m
    assert bool((raw["lo"][untouched] == SENTINEL).all()) and bool((raw["hi"][untouched] == SENTINEL).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", QR.SHAPES)
@pytest.mark.parametrize("S", [1, 2, 7, 19])
def test_tails_and_quantiles_against_restatement(shape, S, dt):
    for order in QR.ORDERS:
        c = case(*shape, S, dt, order)
        for K in sorted({1, 2, 5, S, S + 3}):
            ref = reference(*shape, S, dt, order, K)
            got = run(c, dt, K, [(0, S)])
            check(got, ref, dt, K)
            out, cnt = got[1].cpu().numpy(), ref[0]
            # the contract's NaN, independently of the restatement: no draw, no quantile; every value kept, every quantile
            assert cnt[1] == 0 and np.isnan(out[:, 1]).all()
            if K >= S:
                assert not np.isnan(out[:, cnt > 0]).any()
            if K == 1 and S >= 7:
                assert np.isnan(out[:, cnt > 1]).all()
    # the skips reached the counts
    cnt = reference(*shape, S, dt, "random", S)[0].reshape(shape[0], shape[1], 6)
    assert cnt[0, 0, 0] == (S - 1 if S >= 2 else S) and cnt[0, 0, 2] == S
    if S >= 3 and shape[0] >= 2:
        assert (cnt[-1] == S - 1).all()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", QR.SHAPES)
def test_deep_heaps_that_overflow_many_times(shape, dt):
    """S = 300 draws into K = 9 slots: three heap levels, hundreds of replacements at the root in ascending / descending order."""
    levels = (0.01, 0.025, 0.5, 0.975, 0.99)
    for order in QR.ORDERS:
        c = case(*shape, 300, dt, order)
        ref = reference(*shape, 300, dt, order, 9, levels)
        got = run(c, dt, 9, [(0, 300)], levels)
        check(got, ref, dt, 9)
        out = got[1].cpu().numpy()
        seen = ref[0] > 0
        assert np.isnan(out[2]).all() and not np.isnan(out[[0, 1, 3, 4]][:, seen]).any()       # the median is out of reach of 9 values


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", QR.SHAPES)
@pytest.mark.parametrize("S,K", [(7, 2), (7, 5), (7, 10), (19, 5)])
def test_splits_permutations_and_further_folds(shape, dt, S, K):
    """One call, 3 + 3 + rest, 4 + rest, draw by draw, from a misaligned view, and again: cnt, lo, hi as folded and the quantiles
    are torch.equal.  A permutation of the draws: the same tails and quantiles.  Folding on after a pred_quantiles call (which
    sorts the buffers in place): the same tails and quantiles as folding everything first."""
    c = case(*shape, S, dt, "ties" if K == 5 else "random")
    whole = run(c, dt, K, [(0, S)])
    runs = {"3+3+rest": [(0, 3), (3, 6), (6, S)], "4+rest": [(0, 4), (4, S)], "one by one": [(s, s + 1) for s in range(S)], "again": [(0, S)]}
    for name, splits in runs.items():
        other = run(c, dt, K, splits, offset=(name == "4+rest"))
        for k in ("cnt", "lo", "hi"):
            assert torch.equal(bits(whole[0][k]), bits(other[0][k])), (name, k)
        assert torch.equal(bits(whole[1]), bits(other[1])), name
    perm = torch.tensor(np.random.default_rng(S + K).permutation(S), device=DEV)
    shuffled = run(c, dt, K, [(0, S)], perm=perm)
    later = run(c, dt, K, [(0, 3), (3, S)], quantiles_after=0)
    for name, other in (("permuted", shuffled), ("folded on", later)):
        assert torch.equal(whole[0]["cnt"], other[0]["cnt"]), name
        for i in (1, 2, 3):
            assert torch.equal(bits(whole[i]), bits(other[i])), (name, i)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", QR.SHAPES)
def test_band_table(shape, dt):
    S = 19
    K = QR.tail_size(BAND_LEVELS, S)
    tdt, npdt = DTYPES[dt]
    c = case(*shape, S, dt, "random")
    cnt, _, _, rout = reference(*shape, S, dt, "random", K, BAND_LEVELS)
    obs, mask = QR.make_observations(rout[0], rout[2], npdt)
    assert QR.clear_of_bounds(obs, rout[0], rout[2])                          # over every entry with a band
    want = QR.band_table(cnt, rout[0], rout[2], obs, mask, BAND_LEVELS[0], BAND_LEVELS[-1])
    ts = run(c, dt, K, [(0, 7), (7, S)], BAND_LEVELS)[4]
    tobs, tmask = torch.tensor(obs, dtype=tdt, device=DEV), torch.tensor(mask, device=DEV)
    out, table = hode.capi.pred_quantiles(ts, BAND_LEVELS, tobs, tmask, band=True)
    again = hode.capi.pred_quantiles(ts, BAND_LEVELS, tobs, tmask, band=True)
    assert torch.equal(table, again[1]) and torch.equal(bits(out), bits(again[0])) and same(out, rout, npdt)
    table = table.cpu().numpy()
    print("band table\n", table, "\nrestatement\n", want)
    assert np.array_equal(table[:, [0, 2]], want[:, [0, 2]])
    np.testing.assert_allclose(table[:, [1, 3]], want[:, [1, 3]], rtol=c["N"] * 2.0 ** -52, atol=0)
    assert (table[QR.UNSEEN_STATE] == 0).all() and 0 < table[:, 2].sum() < table[:, 0].sum()    # some inside, some outside
    from inference.predictive import band_metrics
    m, mw = band_metrics(table), QR.band_metrics(want)
    for k in ("band_width", "band_coverage", "band_interval_score"):
        np.testing.assert_allclose(m[k], mw[k], rtol=c["N"] * 2.0 ** -52)
        np.testing.assert_allclose(m[k + "_per_state"], mw[k + "_per_state"], rtol=c["N"] * 2.0 ** -52, equal_nan=True)
        assert np.isnan(m[k + "_per_state"][QR.UNSEEN_STATE]) and np.isfinite(m[k])
    # no mask: finiteness alone decides; one draw: nothing has a band to score
    _, nomask = hode.capi.pred_quantiles(ts, BAND_LEVELS, tobs, None, band=True)
    assert np.array_equal(nomask.cpu().numpy()[:, [0, 2]], QR.band_table(cnt, rout[0], rout[2], obs, None, 0.025, 0.975)[:, [0, 2]])
    one = run(case(*shape, 1, dt, "random"), dt, 1, [(0, 1)], BAND_LEVELS)[4]
    _, t1 = hode.capi.pred_quantiles(one, BAND_LEVELS, tobs, tmask, band=True)
    assert bool((t1 == 0).all()) and np.isnan(band_metrics(t1.cpu().numpy())["band_coverage"])


def test_accumulator_quantiles_band_and_tails():
    """PredictiveAccumulator(quantiles=...) end to end on the N = 390 case, folded 4 + 3: levels, quantiles, band(), tails(),
    the band keys of metrics(); everything the summary had before is bit-identical with and without quantiles."""
    from inference.predictive import PredictiveAccumulator, tail_size
    n_traj, T = QR.SHAPES[1]
    S, q = 7, (0.975, 0.025)
    c = case(n_traj, T, S, "f32", "random")
    K = tail_size(q, S)
    cnt, rlower, rupper, rout = QR.quantiles_of(c["y"], (0.025, 0.975), K, c["status"], np.float32)
    obs, mask = QR.make_observations(rout[0], rout[1], np.float32)
    assert QR.clear_of_bounds(obs, rout[0], rout[1])
    y = torch.tensor(c["y"], dtype=torch.float32, device=DEV).view(S, n_traj, T, 6)
    status = torch.tensor(c["status"])
    tobs, tmask = torch.tensor(obs).view(n_traj, T, 6), torch.tensor(mask).view(n_traj, T, 6).bool()
    acc = PredictiveAccumulator(n_traj, T, tobs, tmask, quantiles=q, expected_draws=S)
    summ = acc.fold(y[:4], status=status[:4]).fold(y[4:], status=status[4:]).finish()
    shape = (n_traj, T, 6)
    assert summ.levels == [0.025, 0.975] and tuple(summ.quantiles.shape) == (2, *shape)
    assert same(summ.quantiles.reshape(2, -1), rout, np.float32)
    lo, hi = summ.band(0.95)
    assert torch.equal(bits(lo), bits(summ.quantiles[0])) and torch.equal(bits(hi), bits(summ.quantiles[1]))
    with pytest.raises(KeyError):
        summ.band(0.5)
    lower, upper = summ.tails()
    assert tuple(lower.shape) == (K, *shape) and same(lower.reshape(K, -1), rlower, np.float32) and same(upper.reshape(K, -1), rupper, np.float32)
    want = QR.band_table(cnt, rout[0], rout[1], obs, mask, 0.025, 0.975)
    assert np.array_equal(summ.band_table[:, [0, 2]], want[:, [0, 2]])
    np.testing.assert_allclose(summ.band_table[:, [1, 3]], want[:, [1, 3]], rtol=c["N"] * 2.0 ** -52)
    plain = PredictiveAccumulator(n_traj, T, tobs, tmask).fold(y, status=status).finish()
    assert plain.levels is None and plain.quantiles is None and plain.band_table is None
    for name in ("mean", "std", "pit", "n"):
        assert torch.equal(bits(getattr(plain, name)), bits(getattr(summ, name))), name
    assert np.array_equal(plain.table, summ.table)
    # ... and is what the fold and score entries give on their own
    st = hode.capi.pred_state(c["N"], DEV)
    hode.capi.pred_fold(y.view(S, -1), st, acc.obs, acc.mask, None, status.to(DEV))
    direct = hode.capi.pred_score(st, torch.float32, acc.obs, acc.mask, [0.0] * 6, plain.thresholds)
    for got, ref in zip((plain.mean, plain.std, plain.pit), direct[:3]):
        assert torch.equal(bits(got.reshape(-1)), bits(ref))
    assert np.array_equal(plain.table, direct[3].cpu().numpy())
    pm, sm = plain.metrics(), summ.metrics()
    assert set(sm) - set(pm) == {k + s for k in ("band_width", "band_coverage", "band_interval_score") for s in ("", "_per_state")}
    assert all(np.array_equal(pm[k], sm[k], equal_nan=True) for k in pm)
    wm = QR.band_metrics(want)
    for k in ("band_width", "band_coverage", "band_interval_score"):
        np.testing.assert_allclose(sm[k], wm[k], rtol=c["N"] * 2.0 ** -52)
    acc.fold(y[:1], status=status[:1])
    with pytest.raises(RuntimeError):
        summ.tails()                                            # the buffers have moved on
    with pytest.raises(ValueError, match="expected_draws"):
        acc.finish()                                            # eight draws into buffers sized for seven


# ------------------------------------------------------------------------------------------------ the entry points
B, T = 3, 13
Q95 = (0.025, 0.975)


def _model(golden_dir, variational=False):
    import models
    w = np.load(os.path.join(golden_dir, "g0_weights_h32_l2.npz"))
    ode8 = {"a_GI": 0.0104, "k_I": 0.025, "rho": 0.003, "E_max": 0.1, "EC_50": 50.0, "V_max": 9.0, "K_m": 7.0, "k_L": 0.02}
    prior = {f"ode_{n}": {"mean": v, "std": 0.05 * v} for n, v in ode8.items()}
    m = models.HybridODENN(nn_hidden=32, nn_layers=2, use_variational=variational, prior_params=prior if variational else None,
                           device="cuda")
    flat, off = torch.tensor(w["nn_flat"]), 0
    with torch.no_grad():
        for name, p in m.nn_residual.named_parameters():
            p.copy_(flat[off:off + p.numel()].reshape(p.shape))
            if variational:                                  # a posterior centred on the golden weights, 2 % wide
                key = f"nn_{name.replace('.', '_')}"
                m.variational_params.means[key].copy_(p)
                m.variational_params.log_stds[key].fill_(float(np.log(0.02)))
            off += p.numel()
    return m


@pytest.fixture(scope="module")
def batch(golden_dir):
    g = np.load(os.path.join(golden_dir, "g4_t61_pulses.npz"))
    rng = np.random.default_rng(5)
    obs = g["y_rk45_tight"][:B, :T].astype(np.float64) * (1.0 + 0.05 * rng.standard_normal((B, T, 6)))
    obs[rng.random((B, T, 6)) < 0.05] = np.nan
    return {"initial_state": torch.tensor(g["x0"][:B]), "observations": torch.tensor(obs, dtype=torch.float32),
            "time_points": torch.tensor(g["t"][:T]),
            "external_inputs": {"meal": torch.tensor(g["meal"][:B, :T]), "tVNS": torch.tensor(g["tvns"][:B, :T])}}


def _check_summary_against_block(summ, y, batch):
    """summ's quantiles, tails and band table against the restatement applied to the held block y [S, B, T, 6]."""
    y = y.detach().cpu().numpy().astype(np.float64)
    S = y.shape[0]
    K = QR.tail_size(Q95, S)
    cnt, rlower, rupper, rout = QR.quantiles_of(y.reshape(S, -1), Q95, K, None, np.float32)
    assert int((summ.n != S).sum()) == 0 and (cnt == S).all()
    assert summ.levels == list(Q95) and same(summ.quantiles.reshape(2, -1), rout, np.float32)
    lower, upper = summ.tails()
    assert same(lower.reshape(K, -1), rlower, np.float32) and same(upper.reshape(K, -1), rupper, np.float32)
    lo, hi = summ.band()
    assert bool((lo <= hi).all())
    obs = batch["observations"].numpy().astype(np.float64).reshape(-1)
    want = QR.band_table(cnt, rout[0], rout[1], obs, None, *Q95)
    np.testing.assert_allclose(summ.band_table, want, rtol=obs.size * 2.0 ** -52)
    assert "band_coverage" in summ.metrics()


def test_predictive_summary_and_vi_quantiles_in_pieces(golden_dir, batch):
    from inference import VariationalInference, predictive_summary
    m = _model(golden_dir, variational=True)
    torch.manual_seed(3)
    with torch.no_grad():
        draws = [m.variational_params.sample(1)[0] for _ in range(5)]
        y = m.forward_param_sets(draws, batch["initial_state"], batch["time_points"], batch["external_inputs"])
    assert m.solve_failures() == 0
    summ = predictive_summary(m, draws, batch, max_bytes=2 * B * T * 6 * 4, quantiles=Q95)            # cut 2 + 2 + 1
    _check_summary_against_block(summ, y, batch)
    plain = predictive_summary(m, draws, batch, max_bytes=2 * B * T * 6 * 4)
    assert plain.levels is None and plain.quantiles is None and plain.band_table is None
    for name in ("mean", "std", "pit"):
        assert torch.equal(bits(getattr(plain, name)), bits(getattr(summ, name))), name
    assert torch.equal(plain.n, summ.n) and np.array_equal(plain.table, summ.table)
    assert set(plain.metrics()) < set(summ.metrics())
    torch.manual_seed(3)
    vs = VariationalInference(m, device=torch.device("cuda")).predictive_summary(batch, n_samples=5, max_bytes=2 * B * T * 6 * 4, quantiles=Q95)
    _check_summary_against_block(vs, y, batch)


def test_hmc_result_quantiles_and_summary(golden_dir, batch):
    from inference.hmc import HMCResult
    from inference.observation import ObservationModel
    m = _model(golden_dir)
    nn_base, ode_base = m._params_on(torch.device("cuda"))
    rng = np.random.default_rng(9)
    mu = np.array([0.025, 7.0])
    draws = torch.tensor(mu * (1.0 + 0.05 * rng.standard_normal((2, 4, 2))), dtype=torch.float32, device="cuda")
    res = HMCResult(draws, ["k_I", "K_m"], [], {}, m, ode_base.detach(), nn_base.detach(), ObservationModel([6.0, 0.8, 3.0, 0.4, 0.03, 0.02]), batch)
    summ = res.predictive_summary(thin=2, observation_noise=False, max_bytes=3 * B * T * 6 * 4, quantiles=Q95)
    y = res.predict(batch["initial_state"], batch["time_points"], batch["external_inputs"], thin=2)
    assert tuple(y.shape) == (4, B, T, 6)
    _check_summary_against_block(summ, y, batch)
    plain = res.predictive_summary(thin=2, observation_noise=False, max_bytes=3 * B * T * 6 * 4)
    assert plain.quantiles is None and torch.equal(bits(plain.std), bits(summ.std)) and np.array_equal(plain.table, summ.table)


def test_hmc_result_summary_is_the_reference_posterior_summary():
    """HMCResult.summary() on synthetic draws [4, 25, D]: the keys of the reference's posterior_summary (mean, std, median, q025,
    q975) plus rhat and ess; the quantiles bit-equal to the restatement over the 100 pooled draws, mean and std (ddof = 0)
    within S * 2^-52 * mean|x| of numpy in fp64."""
    from inference.hmc import HMCResult
    rng = np.random.default_rng(11)
    C, n = 4, 25
    nn_names = [("net.0.weight", (2, 3)), ("net.0.bias", (3,))]
    D = 2 + 6 + 3
    centre = np.concatenate([[0.025, 7.0], rng.standard_normal(9)])
    x = (centre * (1.0 + 0.05 * rng.standard_normal((C, n, D)))).astype(np.float32)
    res = HMCResult(torch.tensor(x, device=DEV), ["k_I", "K_m"], nn_names, {})
    out = res.summary()
    assert list(out) == ["ode.k_I", "ode.K_m", "nn.net.0.weight", "nn.net.0.bias"] == list(res.samples)
    S = C * n
    flat = x.reshape(S, D).astype(np.float64)
    levels = (0.025, 0.5, 0.975)
    rq = QR.quantiles_of(flat, levels, QR.tail_size(levels, S), None, np.float32)[3].astype(np.float64)
    rhat, ess = res.rhat().cpu().numpy(), res.ess().cpu().numpy()
    tol = S * 2.0 ** -52 * np.abs(flat).mean(0)
    off = 0
    for name, shape in (("ode.k_I", ()), ("ode.K_m", ()), ("nn.net.0.weight", (2, 3)), ("nn.net.0.bias", (3,))):
        k = int(np.prod(shape)) if shape else 1
        sl = slice(off, off + k)
        s = out[name]
        assert set(s) == {"mean", "std", "median", "q025", "q975", "rhat", "ess"}
        assert all(np.shape(v) == shape for v in s.values()), name
        for key, row in (("q025", 0), ("median", 1), ("q975", 2)):
            assert np.array_equal(np.reshape(s[key], -1), rq[row, sl]), (name, key)
        assert np.all(np.abs(np.reshape(s["mean"], -1) - flat[:, sl].mean(0)) <= tol[sl])
        assert np.all(np.abs(np.reshape(s["std"], -1) - flat[:, sl].std(0)) <= tol[sl])
        assert np.array_equal(np.reshape(s["rhat"], -1), rhat[sl]) and np.array_equal(np.reshape(s["ess"], -1), ess[sl])
        assert np.all(s["q025"] <= s["median"]) and np.all(s["median"] <= s["q975"])
        off += k
