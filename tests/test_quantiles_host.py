"""Host-side checks of the posterior bands (no GPU): the NumPy restatement the GPU tests compare the tail and quantile kernels
with (tests/_quantile_reference.py) against np.quantile; tail_size; the exported names and symbols; argument validation by
return code; the accumulator's expected_draws guard."""
import ctypes
import os
import re

import numpy as np
import pytest

import _quantile_reference as QR

torch = pytest.importorskip("torch")
import hode  # noqa: E402

DRAWS = (1, 2, 3, 7, 19, 41, 100, 1000)
LEVELS = (0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999)
ULPS = 4


def host_case(S, dtype, N=60):
    """y [S, N] in `dtype` precision with a block of tied values (a fifth of the draws of every other entry share one value)."""
    rng = np.random.default_rng(100 + S + (7 if dtype == np.float32 else 0))
    y = np.tile(QR.SCALE, N // 6) * (1.0 + 0.05 * rng.standard_normal((S, N)))
    k = max(1, S // 5)
    y[rng.permutation(S)[:k], ::2] = y[0, ::2]
    return y.astype(dtype).astype(np.float64)


def test_restatement_agrees_with_numpy_quantile():
    """np.sort + the formula of include/hode.h against np.quantile(y, q, axis=0) (a fraction, not np.percentile: q * 100 / 100
    moves h by hundreds of ulps) for S in DRAWS, seven levels down to 0.001 and up to 0.999, fp32- and fp64-valued inputs with
    tied values.  numpy arranges the same interpolation differently (it interpolates from b when g >= 1/2), so the two differ
    by rounding: the observed maximum on these inputs is 1 ulp of fp64 at max(|a|, |b|) with numpy 2.2.6 (2 ulp have been
    seen on others); 4 ulp are allowed."""
    worst = 0.0
    for S in DRAWS:
        for dtype in (np.float32, np.float64):
            y = host_case(S, dtype)
            _, lower, upper, got = QR.quantiles_of(y, LEVELS)
            assert not np.isnan(got).any()
            want = np.quantile(y, LEVELS, axis=0)
            n = S
            for l, q in enumerate(LEVELS):
                j = int(np.floor(q * (n - 1)))
                srt = np.sort(y, axis=0)
                scale = np.maximum(np.abs(srt[j]), np.abs(srt[min(j + 1, n - 1)]))
                worst = max(worst, float(np.max(np.abs(got[l] - want[l]) / np.spacing(scale))))
    print("restatement vs np.quantile, worst difference in ulp of fp64:", worst)
    assert worst <= ULPS, worst


def test_tail_size_known_values_and_sufficiency():
    from inference.predictive import tail_size
    assert tail_size((0.025,), 1000) == 26
    assert tail_size((0.5,), 1000) == 501
    assert tail_size((0.025,), 7) == 2
    assert tail_size((0.025, 0.975), 1024) == 27
    for lv in ((0.025,), (0.5,), LEVELS):
        assert tail_size(lv, 1) == 1
    assert tail_size((0.025, 0.5, 0.975), 100) == 51
    for bad in ((), (0.0,), (1.0,), (0.5, 1.5)):
        with pytest.raises(ValueError):
            tail_size(bad, 10)
    with pytest.raises(ValueError):
        tail_size((0.5,), 0)
    # the restatement with that many values kept equals the restatement with every value kept
    for S in DRAWS:
        for dtype in (np.float32, np.float64):
            y = host_case(S, dtype)
            for lv in ((0.025, 0.975), (0.001, 0.999), LEVELS, (0.25,)):
                K = tail_size(lv, S)
                assert K == QR.tail_size(lv, S) and 1 <= K <= S
                full = QR.quantiles_of(y, lv)[3]
                some = QR.quantiles_of(y, lv, K=K)[3]
                assert np.array_equal(full, some), (S, lv, K)


def test_restatement_nan_rules_and_fewer_draws_than_expected():
    y = host_case(19, np.float64)
    y[:, 3] = np.nan                                            # an entry without a draw
    y[5:, 4] = np.inf                                           # an entry with five
    cnt, lower, upper, out = QR.quantiles_of(y, (0.025, 0.5, 0.975), K=3)
    assert cnt[3] == 0 and cnt[4] == 5 and np.isnan(out[:, 3]).all()
    assert np.isnan(out[1]).all()                               # the median of 19 (or 5) values is not among the 3 outermost
    assert not np.isnan(out[0][cnt > 0]).any() and not np.isnan(out[2][cnt > 0]).any()
    np.testing.assert_allclose(out[[0, 2], 4], np.quantile(y[:5, 4], (0.025, 0.975)), rtol=1e-15)
    full = QR.quantiles_of(y, (0.025, 0.5, 0.975))[3]
    assert np.array_equal(full[[0, 2]], out[[0, 2]], equal_nan=True) and not np.isnan(full[:, cnt > 0]).any()


def test_new_names_and_symbols_are_exported():
    import inference
    from inference.hmc import HMCResult
    from inference.vi import VariationalInference
    import inspect
    assert "tail_size" in inference.__all__ and inference.tail_size is inference.predictive.tail_size
    for name in ("tail_size", "BAND_COLUMNS"):
        assert name in inference.predictive.__all__
    for fn in (inference.predictive_summary, HMCResult.predictive_summary, VariationalInference.predictive_summary):
        p = inspect.signature(fn).parameters["quantiles"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    sig = inspect.signature(inference.PredictiveAccumulator.__init__).parameters
    for name in ("quantiles", "expected_draws"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None
    assert callable(HMCResult.summary)
    for name in ("band", "tails"):
        assert callable(getattr(inference.PredictiveSummary, name))
    for name in ("pred_tail_state", "pred_tails", "pred_quantiles"):
        assert callable(getattr(hode.capi, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hode.h")).read()
    lib = ctypes.CDLL(hode.lib_path())
    for sym in ("hode_pred_tails_f32", "hode_pred_tails_f64", "hode_pred_quantiles_f32", "hode_pred_quantiles_f64"):
        assert sym in hode.capi.SYMBOLS and re.search(r"\b" + sym + r"\s*\(", hdr) and hasattr(lib, sym)
    assert int(re.search(r"#define HODE_PRED_MAX_LEVELS (\d+)", hdr).group(1)) == hode.capi.PRED_MAX_LEVELS == 16


def test_bad_arguments_are_refused_by_return_code_without_gpu():
    lib = hode.load()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    i64 = ctypes.c_int64

    def lv(*q):
        return (ctypes.c_double * max(len(q), 1))(*q)
    for sfx in ("f32", "f64"):
        tails, quant = getattr(lib, "hode_pred_tails_" + sfx), getattr(lib, "hode_pred_quantiles_" + sfx)
        st = [one] * 3
        assert tails(z, -1, i64(5), one, z, i64(0), 3, *st) == -1                          # n_draws < 0
        assert tails(z, 1, i64(5), one, z, i64(0), 0, *st) == -1                           # K < 1
        assert tails(z, 1, i64(0), one, z, i64(0), 3, *st) == -1                           # N < 1
        for k in range(3):
            assert tails(z, 1, i64(5), one, z, i64(0), 3, *(st[:k] + [z] + st[k + 1:])) == -1                # a null state pointer
        assert tails(z, 1, i64(5), z, z, i64(0), 3, *st) == -1                             # no y
        assert tails(z, 1, i64(12), one, one, i64(0), 3, *st) == -1                        # status with row_len < 1
        assert tails(z, 1, i64(12), one, one, i64(5), 3, *st) == -1                        # row_len does not divide N
        assert tails(z, 0, i64(5), z, z, i64(0), 3, *st) == 0                              # nothing to take: no launch
        assert tails(z, 0, i64(7), z, one, i64(7), 1, *st) == 0
        ok = lv(0.025, 0.975)
        # after the levels: out, obs, mask, band_table, work
        assert quant(z, i64(0), 3, *st, 2, ok, one, z, z, z, z) == -1                      # N < 1
        assert quant(z, i64(6), 0, *st, 2, ok, one, z, z, z, z) == -1                      # K < 1
        for k in range(3):
            assert quant(z, i64(6), 3, *(st[:k] + [z] + st[k + 1:]), 2, ok, one, z, z, z, z) == -1           # a null state pointer
        assert quant(z, i64(6), 3, *st, 2, z, one, z, z, z, z) == -1                       # no levels
        assert quant(z, i64(6), 3, *st, 2, ok, z, z, z, z, z) == -1                        # no out
        assert quant(z, i64(6), 3, *st, 0, ok, one, z, z, z, z) == -1                      # n_levels range
        assert quant(z, i64(6), 3, *st, 17, lv(*[(i + 1) / 20 for i in range(17)]), one, z, z, z, z) == -1
        assert quant(z, i64(6), 3, *st, 2, lv(0.0, 0.5), one, z, z, z, z) == -1            # a level on the boundary
        assert quant(z, i64(6), 3, *st, 2, lv(0.5, 1.0), one, z, z, z, z) == -1
        assert quant(z, i64(6), 3, *st, 1, lv(float("nan")), one, z, z, z, z) == -1
        assert quant(z, i64(6), 3, *st, 2, lv(0.975, 0.025), one, z, z, z, z) == -1        # not ascending
        assert quant(z, i64(6), 3, *st, 2, lv(0.5, 0.5), one, z, z, z, z) == -1
        assert quant(z, i64(6), 3, *st, 2, ok, one, z, one, z, z) == -1                    # a mask without obs
        assert quant(z, i64(6), 3, *st, 2, ok, one, z, z, one, one) == -1                  # a band table without obs
        assert quant(z, i64(6), 3, *st, 2, ok, one, one, z, one, z) == -1                  # ... without work
        assert quant(z, i64(7), 3, *st, 2, ok, one, one, z, one, one) == -1                # ... with N % 6 != 0
        assert quant(z, i64(6), 3, *st, 2, lv(0.025, 0.4), one, one, z, one, one) == -1    # ... with both levels below 1/2
        assert quant(z, i64(6), 3, *st, 2, lv(0.5, 0.9), one, one, z, one, one) == -1
        assert quant(z, i64(6), 3, *st, 1, lv(0.025), one, one, z, one, one) == -1         # ... with one level


def test_binding_refuses_host_tensors_and_bad_levels():
    cpu = {"cnt": torch.zeros(6, dtype=torch.int32), "lo": torch.empty(2, 6), "hi": torch.empty(2, 6)}
    with pytest.raises(hode.HodeError):
        hode.capi.pred_tails(torch.zeros(1, 6), cpu)
    with pytest.raises(hode.HodeError):
        hode.capi.pred_quantiles(cpu, (0.5,))
    with pytest.raises(hode.HodeError):
        hode.capi.pred_tail_state(0, 1, torch.float32, "cpu")
    with pytest.raises(hode.HodeError):
        hode.capi.pred_tail_state(6, 1, torch.float16, "cpu")


def test_accumulator_guards_without_a_device(monkeypatch):
    """Argument checks of the Python surface that need no kernel: quantiles without expected_draws, bad fractions, and finish()
    after more draws than expected_draws (the device and the kernels are stubbed out: the guard is host logic)."""
    from inference import predictive as P
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hode.HodeError):
        P.PredictiveAccumulator(2, 3, quantiles=(0.025, 0.975), expected_draws=4)
    monkeypatch.setattr(P, "_device", lambda: torch.device("cpu"))
    with pytest.raises(ValueError):
        P.PredictiveAccumulator(2, 3, quantiles=(0.025, 0.975))
    with pytest.raises(ValueError):
        P.PredictiveAccumulator(2, 3, quantiles=(0.0, 0.975), expected_draws=4)
    with pytest.raises(ValueError):
        P.PredictiveAccumulator(2, 3, quantiles=(), expected_draws=4)
    calls = []
    monkeypatch.setattr(hode.capi, "_need_gpu", lambda t: None)
    monkeypatch.setattr(hode.capi, "pred_fold", lambda *a, **k: None)
    monkeypatch.setattr(hode.capi, "pred_tails", lambda *a, **k: calls.append("tails"))
    monkeypatch.setattr(hode.capi, "pred_score", lambda st, dt, *a, **k: tuple(torch.zeros(36) for _ in range(3)) + (torch.zeros(6, 36),))
    monkeypatch.setattr(hode.capi, "pred_quantiles", lambda *a, **k: calls.append("quantiles"))
    acc = P.PredictiveAccumulator(2, 3, quantiles=(0.975, 0.025), expected_draws=4)
    assert acc.levels == [0.025, 0.975] and acc.tail_state["lo"].shape == (P.tail_size((0.025, 0.975), 4), 36)
    acc.fold(torch.zeros(3, 2, 3, 6)).fold(torch.zeros(2, 2, 3, 6))
    assert calls == ["tails", "tails"] and acc.n_folded == 5
    with pytest.raises(ValueError, match="expected_draws"):
        acc.finish()
    assert "quantiles" not in calls
    summ = P.PredictiveAccumulator(2, 3).fold(torch.zeros(3, 2, 3, 6)).finish()             # today's behaviour: no quantile fields
    assert summ.levels is None and summ.quantiles is None and summ.band_table is None
    with pytest.raises(KeyError):
        summ.band()
    with pytest.raises(KeyError):
        summ.tails()
