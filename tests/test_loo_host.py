"""Host-side checks of the model comparison (no GPU): the NumPy restatement the GPU tests compare the LOO kernels with
(tests/_loo_reference.py) in its two forms, its precision bound in np.longdouble on exactly the GPU tests' inputs, a conjugate
model with a closed-form leave-one-out density, the invariances of PSIS; loo_tail_size; the exported names and symbols;
argument validation by return code; `compare` on hand-built results; the accumulator's guards."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _loo_reference as LR

torch = pytest.importorskip("torch")
import hode  # noqa: E402


def conjugate(seed, S=1000, n=30):
    """n observations y_i ~ N(mu, 1), flat prior: the posterior is N(mean y, 1 / n), drawn exactly.  Returns l [S, n] and the
    closed-form leave-one-out log density sum_i log N(y_i | mean y_-i, 1 + 1 / (n - 1))."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(n)
    mu = y.mean() + rng.standard_normal(S) / np.sqrt(n)
    l = -0.5 * (y[None] - mu[:, None]) ** 2 - 0.5 * np.log(2 * np.pi)
    m, v = (y.sum() - y) / (n - 1), 1.0 + 1.0 / (n - 1)
    return l, float((-0.5 * (y - m) ** 2 / v - 0.5 * np.log(2 * np.pi * v)).sum())


def test_two_forms_of_the_restatement_agree():
    """The full-array form (sort all r, smooth in place, renormalise, logsumexp(x + l)) against the heap form the kernel uses
    (the K largest r + a running log-sum-exp of the rest).  Measured: elpd differs by at most 2.7e-15 on the conjugate model at
    S = 300 and 1 000 and by at most 1.5e-14 (one ulp of an elpd near -100) on the GPU tests' heavy-tailed inputs, with
    K = loo_tail_size(S) and K = S + 3; k and t are equal (the fit sees the same numbers).  Ten times that is asserted."""
    for S in (300, 1000):
        l, _ = conjugate(0, S)
        _, out = LR.loo_of(l, LR.loo_tail_size(S))
        for i in range(l.shape[1]):
            e, k, t = LR.psis_full(l[:, i])
            assert abs(e - out["elpd_loo"][i]) <= 2.7e-14 and k == out["pareto_k"][i] and t == out["t"][i]
    worst = 0.0
    for shape, S in ((LR.SHAPES[0], 19), (LR.SHAPES[1], 40), (LR.SHAPES[1], 300)):
        for K in (LR.loo_tail_size(S), S + 3):
            l, _, out = LR.reference(*shape, S, "f64", K)
            for i in np.where(~np.isnan(out["lppd"]))[0]:
                e, k, t = LR.psis_full(l[:, i][~np.isnan(l[:, i])])
                worst = max(worst, abs(e - out["elpd_loo"][i]))
                assert t == out["t"][i] and (k == out["pareto_k"][i] or (np.isinf(k) and np.isinf(out["pareto_k"][i])))
    print("full-array form against heap form, worst |elpd| difference:", worst)
    assert worst <= 1.5e-13


def test_precision_bound_in_longdouble_on_the_gpu_inputs():
    """The restatement in np.longdouble (64-bit mantissa here) against itself in fp64 on every input of tests/test_loo_gpu.py
    (LR.GPU_CASES, fp32- and fp64-valued, K = loo_tail_size(S)).  Measured: |elpd_loo| differs by at most 1.35e-13 and pareto_k by
    at most 1.55e-13 (k from -0.6 to 14.9); LR.TOL_ELPD = 1.4e-12 and LR.TOL_K = 1.6e-12, what the GPU tests allow, are ten times
    that, which is what this test holds them to.  All four k bins are populated."""
    assert np.finfo(np.longdouble).nmant >= 63
    worst_e = worst_k = 0.0
    bins = np.zeros(4)
    for shape, S in LR.GPU_CASES:
        for dt in ("f32", "f64"):
            K = LR.loo_tail_size(S)
            _, _, o = LR.reference(*shape, S, dt, K)
            _, _, o2 = LR.reference(*shape, S, dt, K, True)
            ok = ~np.isnan(o["lppd"])
            assert np.array_equal(ok, ~np.isnan(np.asarray(o2["lppd"], dtype=np.float64))) and np.array_equal(o["t"], o2["t"])
            if not ok.any():
                continue
            fk = ok & np.isfinite(o["pareto_k"])
            assert np.array_equal(fk, ok & np.isfinite(np.asarray(o2["pareto_k"], dtype=np.float64)))
            worst_e = max(worst_e, float(np.abs((o["elpd_loo"] - o2["elpd_loo"])[ok]).max()))
            if fk.any():
                worst_k = max(worst_k, float(np.abs(o["pareto_k"][fk] - o2["pareto_k"][fk]).max()))
            bins += LR.table(o)[:, 8:12].sum(0)
    print("fp64 against longdouble: elpd", worst_e, "k", worst_k, "k bins", bins)
    assert 10.0 * worst_e <= LR.TOL_ELPD and 10.0 * worst_k <= LR.TOL_K
    assert (bins > 0).all()


def test_exact_model_psis_is_closer_than_lppd():
    """Conjugate normal-mean model, 30 observations, 1 000 exact posterior draws, seeds 0..19.  sum elpd_loo is closer to the
    closed-form leave-one-out density than sum lppd is, in every seed (seed 0: PSIS -38.203, exact -38.237, lppd -37.557, WAIC
    -38.200; every k below 0.4).  Over the 20 seeds sum p_loo has mean 1.000 and standard deviation 0.29 (one parameter; the
    spread is the data's), and sum elpd_waic - sum elpd_loo has mean 0.0047, standard deviation 0.0030 and maximum 0.0149.
    Margins: |sum p_loo - 1| <= 0.87 (three standard deviations), |sum elpd_waic - sum elpd_loo| <= 0.02 (mean + five)."""
    for seed in range(20):
        l, exact = conjugate(seed)
        _, o = LR.loo_of(l, LR.loo_tail_size(1000))
        loo, lppd, waic = o["elpd_loo"].sum(), o["lppd"].sum(), o["elpd_waic"].sum()
        assert abs(loo - exact) < abs(lppd - exact), seed
        assert abs((lppd - loo) - 1.0) <= 0.87 and abs(waic - loo) <= 0.02, seed
        assert o["pareto_k"].max() < 0.5
        if seed == 0:
            assert abs(loo + 38.203) < 1e-3 and abs(exact + 38.237) < 1e-3 and abs(lppd + 37.557) < 1e-3 and abs(waic + 38.200) < 1e-3


def test_invariances():
    l, _, out = LR.reference(*LR.SHAPES[1], 40, "f64", LR.loo_tail_size(40))
    ok = np.where(~np.isnan(out["lppd"]) & np.isfinite(out["pareto_k"]))[0][:40]
    # a power of two added to an entry's l shifts r, c and nothing else: x, the tail and the fit see the same numbers up to the
    # rounding of l + 8 itself, which moves elpd and k by 9.4e-15 at most here; ten times that is allowed
    worst = 0.0
    for i in ok:
        li = l[:, i][~np.isnan(l[:, i])]
        e0, k0, t0 = LR.psis_full(li)
        e1, k1, t1 = LR.psis_full(li + 8.0)
        worst = max(worst, abs((e1 - e0) - 8.0), abs(k1 - k0) / max(1.0, abs(k0)))
        assert t0 == t1 and abs((e1 - e0) - 8.0) <= 1e-13 and abs(k1 - k0) <= 1e-13 * max(1.0, abs(k0))
    print("shift by 8: worst deviation", worst)
    # scaling the input of the fit scales sigma and leaves k (measured: 6e-16 relative at a factor of 4; 1e-13 is allowed)
    rng = np.random.default_rng(3)
    a = np.sort(rng.pareto(2.0, (5, 25)), axis=1)
    k0, s0 = LR.gpdfit(a)
    for f in (4.0, 3.7e-3):
        k1, s1 = LR.gpdfit(f * a)
        np.testing.assert_allclose(k1, k0, rtol=1e-13)
        np.testing.assert_allclose(s1, f * s0, rtol=1e-13)
    # a constant l: nothing is above the cut, k is infinite, elpd_loo = l and p_loo = 0
    for n in (7, 40, 300):
        lc = np.full((n, 6), -1.75)
        for K in (LR.loo_tail_size(n), n + 3):
            _, o = LR.loo_of(lc, K)
            assert (o["t"] == 0).all() and np.isinf(o["pareto_k"]).all()
            tol = 8 * LR.EPS * (np.log(n) + 1.75)                  # a handful of roundings of values up to log n + |l|
            np.testing.assert_allclose(o["elpd_loo"], -1.75, rtol=0, atol=tol)
            np.testing.assert_allclose(o["lppd"] - o["elpd_loo"], 0.0, atol=tol)
        e, k, t = LR.psis_full(lc[:, 0])
        assert t == 0 and np.isinf(k) and abs(e + 1.75) <= tol
    # the case builder's constant entry is the only entry with a tail value on its cut, and no k or p_waic is near a threshold
    for shape, S in LR.GPU_CASES:
        for dt in ("f32", "f64"):
            _, _, o = LR.reference(*shape, S, dt, LR.loo_tail_size(S))
            assert LR.clear_of_thresholds(o), (shape, S, dt)
            assert list(np.where(o["tie"])[0]) in ([], [LR.CONST_ENTRY]), (shape, S, dt)


def test_loo_tail_size_known_values_and_sufficiency():
    from inference.predictive import loo_tail_size
    for S, want in ((1, 2), (2, 2), (7, 3), (25, 6), (300, 53), (1000, 96), (1024, 97), (40, 9)):
        assert loo_tail_size(S) == want == LR.loo_tail_size(S), S
    assert loo_tail_size(1000, 0.5) == 136 and loo_tail_size(25, 0.5) == 6 and loo_tail_size(300, r_eff=0.25) == 61
    for bad in ((0, 1.0), (10, 0.0), (10, 1.5), (10, float("nan")), (-3, 0.5)):
        with pytest.raises(ValueError):
            loo_tail_size(*bad)
    # with that many ratios held the heap form scores every entry with at least two draws; with one fewer it scores none
    for S in (2, 7, 25, 40):
        l, _ = conjugate(1, S, 6)
        K = loo_tail_size(S)
        assert not np.isnan(LR.loo_of(l, K)[1]["elpd_loo"]).any()
        if K > 2:
            assert np.isnan(LR.loo_of(l, K - 1)[1]["elpd_loo"]).all()


def test_new_names_and_symbols_are_exported():
    import inference
    from inference.hmc import HMCResult
    from inference.vi import VariationalInference
    for name in ("loo_tail_size", "LooResult", "compare"):
        assert name in inference.__all__ and getattr(inference, name) is getattr(inference.predictive, name)
        assert name in inference.predictive.__all__
    assert len(inference.predictive.LOO_COLUMNS) == hode.capi.PRED_LOO_COLS == LR.LOO_COLS == 13
    for fn in (inference.predictive_summary, HMCResult.predictive_summary, VariationalInference.predictive_summary):
        p = inspect.signature(fn).parameters
        assert p["loo"].kind is inspect.Parameter.KEYWORD_ONLY and p["loo"].default is False
        assert p["r_eff"].kind is inspect.Parameter.KEYWORD_ONLY and p["r_eff"].default == 1.0
    sig = inspect.signature(inference.PredictiveAccumulator.__init__).parameters
    assert sig["loo"].kind is inspect.Parameter.KEYWORD_ONLY and sig["loo"].default is False
    assert sig["r_eff"].kind is inspect.Parameter.KEYWORD_ONLY and sig["r_eff"].default == 1.0
    for name in ("pred_loo_state", "pred_loo_fold", "pred_loo_finish"):
        assert callable(getattr(hode.capi, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hode.h")).read()
    lib = ctypes.CDLL(hode.lib_path())
    for sym in ("hode_pred_loo_fold_f32", "hode_pred_loo_fold_f64", "hode_pred_loo_finish_f32", "hode_pred_loo_finish_f64"):
        assert sym in hode.capi.SYMBOLS and re.search(r"\b" + sym + r"\s*\(", hdr) and hasattr(lib, sym)
    assert int(re.search(r"#define HODE_PRED_LOO_COLS (\d+)", hdr).group(1)) == hode.capi.PRED_LOO_COLS
    assert hode.capi.pred_loo_fit_rows(97) == 96 + 30 + 9 and hode.capi.pred_loo_fit_rows(2) == 32


def test_bad_arguments_are_refused_by_return_code_without_gpu():
    lib = hode.load()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    i64, dbl = ctypes.c_int64, ctypes.c_double
    for sfx in ("f32", "f64"):
        fold, finish = getattr(lib, "hode_pred_loo_fold_" + sfx), getattr(lib, "hode_pred_loo_finish_" + sfx)
        st = [one] * 8
        # (stream, n_draws, N, y, obs, mask, sigma, status, row_len, K, state...)
        assert fold(z, -1, i64(12), one, one, z, one, z, i64(0), 3, *st) == -1                       # n_draws < 0
        assert fold(z, 1, i64(0), one, one, z, one, z, i64(0), 3, *st) == -1                         # N < 6
        assert fold(z, 1, i64(13), one, one, z, one, z, i64(0), 3, *st) == -1                        # N % 6 != 0
        assert fold(z, 1, i64(12), one, one, z, one, z, i64(0), 1, *st) == -1                        # K < 2
        for k in range(8):
            assert fold(z, 1, i64(12), one, one, z, one, z, i64(0), 3, *(st[:k] + [z] + st[k + 1:])) == -1   # a null state pointer
        assert fold(z, 1, i64(12), z, one, z, one, z, i64(0), 3, *st) == -1                          # no y
        assert fold(z, 1, i64(12), one, z, z, one, z, i64(0), 3, *st) == -1                          # no obs
        assert fold(z, 1, i64(12), one, z, one, one, z, i64(0), 3, *st) == -1                        # a mask without obs
        assert fold(z, 1, i64(12), one, one, z, z, z, i64(0), 3, *st) == -1                          # no sigma: no likelihood
        assert fold(z, 1, i64(12), one, one, z, one, one, i64(0), 3, *st) == -1                      # status with row_len < 6
        assert fold(z, 1, i64(12), one, one, z, one, one, i64(4), 3, *st) == -1                      # row_len % 6 != 0
        assert fold(z, 1, i64(18), one, one, z, one, one, i64(12), 3, *st) == -1                     # row_len does not divide N
        assert fold(z, 0, i64(12), z, one, z, one, z, i64(0), 3, *st) == 0                           # nothing to take: no launch
        assert fold(z, 0, i64(12), z, one, one, one, one, i64(6), 2, *st) == 0
        # (stream, N, K, r_eff, state..., five outputs, table, fit, work)
        rest = [one] * 8
        assert finish(z, i64(0), 3, dbl(1.0), *st, *rest) == -1                                      # N < 6
        assert finish(z, i64(14), 3, dbl(1.0), *st, *rest) == -1                                     # N % 6 != 0
        assert finish(z, i64(12), 1, dbl(1.0), *st, *rest) == -1                                     # K < 2
        for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            assert finish(z, i64(12), 3, dbl(bad), *st, *rest) == -1                                 # r_eff outside (0, 1]
        for k in range(8):
            assert finish(z, i64(12), 3, dbl(1.0), *(st[:k] + [z] + st[k + 1:]), *rest) == -1        # a null state pointer
            assert finish(z, i64(12), 3, dbl(1.0), *st, *(rest[:k] + [z] + rest[k + 1:])) == -1      # a null output / table / fit / work


def test_binding_refuses_host_tensors_and_bad_sizes():
    cpu = hode.capi.pred_loo_state(12, 3, "cpu")
    assert cpu["top"].shape == (3, 12) and bool((cpu["pmax"] == float("-inf")).all()) and bool((cpu["rmax"] == float("-inf")).all())
    assert all(bool((cpu[k] == 0).all()) for k in ("cnt", "lmean", "lm2", "psum", "rsum"))
    with pytest.raises(hode.HodeError):
        hode.capi.pred_loo_fold(torch.zeros(1, 12), cpu, torch.zeros(12), None, torch.ones(1, 6))
    with pytest.raises(hode.HodeError):
        hode.capi.pred_loo_finish(cpu, torch.float32)
    for N, K in ((0, 3), (13, 3), (12, 1)):
        with pytest.raises(hode.HodeError):
            hode.capi.pred_loo_state(N, K, "cpu")


def _result(elpd, k=None, p_waic=None, shift=0.0):
    """A LooResult from pointwise values [B, T, 6] (NaN = not scored): elpd_waic = elpd + shift, lppd = elpd + 0.1."""
    from inference.predictive import LooResult
    elpd = np.asarray(elpd, dtype=np.float64)
    scored = ~np.isnan(elpd)
    k = np.where(scored, 0.1 if k is None else k, np.nan)
    pw = np.where(scored, 0.05 if p_waic is None else p_waic, np.nan)
    out = {"elpd_loo": elpd.reshape(-1), "pareto_k": k.reshape(-1), "elpd_waic": (elpd + shift).reshape(-1), "p_waic": pw.reshape(-1),
           "lppd": (elpd + 0.1).reshape(-1)}
    t = lambda key: torch.tensor(out[key].reshape(elpd.shape))                                                # noqa: E731
    return LooResult(t("elpd_loo"), t("pareto_k"), t("elpd_waic"), t("p_waic"), t("lppd"), LR.table(out))


def test_compare_on_hand_built_results():
    from inference import compare
    rng = np.random.default_rng(0)
    base = -1.0 + 0.3 * rng.standard_normal((2, 5, 6))
    base[0, 0, 3] = np.nan
    base[:, :, 4] = np.nan
    worse = base - 0.2 + 0.1 * rng.standard_normal(base.shape)
    worst = base - 1.0
    k_bad = np.full(base.shape, 0.1)
    k_bad[1, 2, 0] = 0.8
    res = {"worse": _result(worse, k=k_bad), "best": _result(base), "worst": _result(worst, p_waic=np.full(base.shape, 0.5), shift=3.0)}
    rows = compare(res)
    assert [r["name"] for r in rows] == ["best", "worse", "worst"] and [r["rank"] for r in rows] == [0, 1, 2]
    scored = ~np.isnan(base)
    n = scored.sum()
    for r in rows:
        e = {"best": base, "worse": worse, "worst": worst}[r["name"]][scored]
        d = e - base[scored]
        np.testing.assert_allclose(r["elpd"], e.sum(), rtol=1e-13)
        np.testing.assert_allclose(r["se"], np.sqrt(n * e.var()), rtol=1e-10)
        np.testing.assert_allclose(r["elpd_diff"], d.sum(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(r["dse"], 0.0 if r["name"] == "best" else np.sqrt(n * d.var(ddof=1)), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(r["p"], 0.1 * n, rtol=1e-12)
    assert rows[0]["elpd_diff"] == 0.0 and rows[0]["dse"] == 0.0 and rows[2]["dse"] < 1e-12          # a constant shift: no spread
    el = np.array([r["elpd"] for r in rows])
    np.testing.assert_allclose([r["weight"] for r in rows], np.exp(el - el.max()) / np.exp(el - el.max()).sum(), rtol=1e-12)
    assert abs(sum(r["weight"] for r in rows) - 1.0) <= 1e-12
    assert [r["warning"] for r in rows] == [False, True, False]                                      # one k of 0.8
    wrows = compare(res, ic="waic")
    assert [r["name"] for r in wrows] == ["worst", "best", "worse"]                                  # elpd_waic = elpd + 3 there
    assert [r["warning"] for r in wrows] == [True, False, False]                                     # p_waic of 0.5
    np.testing.assert_allclose(wrows[0]["p"], 0.5 * n, rtol=1e-12)
    est = res["best"].estimates()
    assert est["count"] == n and est["pareto_k_counts"].tolist() == [n, 0, 0, 0] and est["looic"] == -2.0 * est["elpd_loo"]
    assert np.isnan(est["elpd_loo_per_state"][4]) and np.isnan(est["se_per_state"][4]) and est["count_per_state"][4] == 0
    assert res["worse"].estimates()["pareto_k_counts"].tolist() == [n - 1, 0, 1, 0]
    # other data: another pattern of scored entries
    other = base.copy()
    other[1, 1, 1] = np.nan
    with pytest.raises(ValueError, match="same"):
        compare({"a": _result(base), "b": _result(other)})
    with pytest.raises(ValueError):
        compare({"a": _result(base)}, ic="bic")
    with pytest.raises(ValueError):
        compare({})
    nothing = _result(np.full((1, 2, 6), np.nan)).estimates()
    assert np.isnan(nothing["elpd_loo"]) and np.isnan(nothing["se"]) and nothing["count"] == 0


def test_accumulator_guards_without_a_device(monkeypatch):
    """Host logic of the Python surface (the device and the kernels are stubbed out): loo without observations or without
    expected_draws, a fold without sigma, finish() after more draws than expected_draws; one expected_draws sizes the quantile
    and the LOO buffers; with loo off nothing of it is touched."""
    from inference import predictive as P
    monkeypatch.setattr(P, "_device", lambda: torch.device("cpu"))
    obs = torch.zeros(2, 3, 6)
    with pytest.raises(ValueError, match="observations"):
        P.PredictiveAccumulator(2, 3, loo=True, expected_draws=4)
    with pytest.raises(ValueError, match="expected_draws"):
        P.PredictiveAccumulator(2, 3, obs, loo=True)
    with pytest.raises(ValueError):
        P.PredictiveAccumulator(2, 3, obs, loo=True, expected_draws=4, r_eff=0.0)
    calls = []
    monkeypatch.setattr(hode.capi, "_need_gpu", lambda t: None)
    monkeypatch.setattr(hode.capi, "pred_fold", lambda *a, **k: None)
    monkeypatch.setattr(hode.capi, "pred_tails", lambda *a, **k: calls.append("tails"))
    monkeypatch.setattr(hode.capi, "pred_loo_fold", lambda *a, **k: calls.append("loo"))
    monkeypatch.setattr(hode.capi, "pred_loo_finish", lambda *a, **k: calls.append("loo_finish"))
    monkeypatch.setattr(hode.capi, "pred_score", lambda st, dt, *a, **k: tuple(torch.zeros(36) for _ in range(3)) + (torch.zeros(6, 36),))
    monkeypatch.setattr(hode.capi, "pred_quantiles", lambda *a, **k: calls.append("quantiles"))
    acc = P.PredictiveAccumulator(2, 3, obs, loo=True, quantiles=(0.025, 0.975), expected_draws=4, r_eff=0.5)
    assert acc.loo_state["top"].shape == (P.loo_tail_size(4, 0.5), 36) and acc.tail_state["lo"].shape == (P.tail_size((0.025, 0.975), 4), 36)
    with pytest.raises(ValueError, match="sigma"):
        acc.fold(torch.zeros(3, 2, 3, 6))
    assert calls == [] and acc.n_folded == 0
    acc.fold(torch.zeros(3, 2, 3, 6), sigma=1.0).fold(torch.zeros(2, 2, 3, 6), sigma=[1.0] * 6)
    assert calls == ["tails", "loo", "tails", "loo"] and acc.n_folded == 5
    with pytest.raises(ValueError, match="expected_draws"):
        acc.finish()
    assert "loo_finish" not in calls and "quantiles" not in calls
    del calls[:]
    summ = P.PredictiveAccumulator(2, 3, obs).fold(torch.zeros(3, 2, 3, 6)).finish()                 # today's behaviour
    assert summ.loo is None and calls == []
    model = type("M", (), {})()
    with pytest.raises(ValueError, match="sigma"):
        P.predictive_summary(model, [{}], {"initial_state": torch.zeros(2, 6), "time_points": torch.zeros(3), "observations": obs}, loo=True)
