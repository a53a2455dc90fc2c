"""Host-side checks of the posterior-predictive summaries (no GPU): the NumPy restatement the GPU tests compare the kernels with
(tests/_predictive_reference.py) against values captured from the reference's eval/evaluate.py
(tests/golden/eval/calibration.npz, tools/capture_golden_eval.py) and against a two-pass long-double computation; the piece
cutter; the exported names; argument validation by return code; HodeError without a device."""
import ctypes
import os

import numpy as np
import pytest

import _predictive_reference as PR

torch = pytest.importorskip("torch")
import hode  # noqa: E402

# |Welford - two-pass| over every GPU test input, measured by test_welford_agrees_with_two_pass_long_double (its docstring
# has the observed maxima); the GPU tests allow ten times this for FMA contraction and the device's erfc / exp / log
WELFORD_BOUND = 1.1e-12


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "eval", "calibration.npz"))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_the_reference_metrics(fixture, tag):
    """Deterministic keys to 1e-12 relative; ece (exact half-normal thresholds) inside the reference's own spread over
    np.random.seed(0..39); rmse and mae overall and per state."""
    g = fixture
    p, u, t = g[f"{tag}_predictions"], g[f"{tag}_uncertainties"], g[f"{tag}_targets"]
    cal, m = PR.calibration(p, u, t, 10)
    for k in ("msis", "sharpness", "coverage_95", "mean_normalized_error"):
        assert abs(cal[k] - float(g[f"{tag}_{k}"])) <= 1e-12 * abs(float(g[f"{tag}_{k}"])), k
    print(tag, "ece", cal["ece"], "reference", float(g[f"{tag}_ece_min"]), float(g[f"{tag}_ece_max"]))
    assert float(g[f"{tag}_ece_min"]) <= cal["ece"] <= float(g[f"{tag}_ece_max"])
    for k in ("rmse", "mae"):
        assert abs(m[k] - float(g[f"{tag}_{k}"])) <= 1e-12 * float(g[f"{tag}_{k}"]), k
        np.testing.assert_allclose(m[k + "_per_state"], g[f"{tag}_{k}_per_state"], rtol=1e-12, atol=0)
    # the package's host-side metrics agree with the restatement's on the same table
    from inference.predictive import table_metrics
    _, _, _, table, _ = PR.score(PR.from_moments(p, u), t.reshape(-1), None, None, PR.thresholds(10))
    pk = table_metrics(table, 10)
    for k in ("ece", "msis", "sharpness", "coverage_95", "mean_normalized_error", "rmse", "mae", "target_std", "crps"):
        np.testing.assert_allclose(pk[k], m[k], rtol=1e-14, err_msg=k)
        np.testing.assert_allclose(pk[k + "_per_state"], m[k + "_per_state"], rtol=1e-14, err_msg=k)
    np.testing.assert_allclose(pk["target_std_per_state"], t.reshape(-1, 6).std(0, ddof=1), rtol=1e-10)


def test_thresholds_are_the_half_normal_quantiles():
    from inference.predictive import half_normal_thresholds
    for nb in (1, 4, 10, 32):
        np.testing.assert_allclose(half_normal_thresholds(nb), PR.thresholds(nb), rtol=1e-13, atol=0)
    assert half_normal_thresholds(10)[0] == 0.0 and abs(half_normal_thresholds(2)[1] - 0.6744897501960817) < 1e-15


@pytest.mark.parametrize("S,per", [(7, 3), (7, 7), (7, 1), (6, 2), (6, 4), (1, 5), (0, 3), (5, 100)])
def test_piece_cutter_covers_every_draw_once_in_order(S, per):
    from inference.predictive import cut_draws
    bytes_per = 1000
    for budget in (per * bytes_per, per * bytes_per + 999):
        pieces = cut_draws(S, bytes_per, budget)
        assert [i for lo, hi in pieces for i in range(lo, hi)] == list(range(S))
        assert all(0 < hi - lo <= per for lo, hi in pieces)
        assert len(pieces) == -(-S // per)
    assert cut_draws(3, 1000, 10) == [(0, 1), (1, 2), (2, 3)]            # a draw that does not fit still goes alone


def test_new_names_are_exported():
    import inference
    import eval as E
    import eval.evaluate as EV
    for name in ("PredictiveAccumulator", "PredictiveSummary", "predictive_summary"):
        assert name in inference.__all__ and getattr(inference, name) is getattr(inference.predictive, name)
    for name in ("compute_rmse", "compute_mae", "compute_calibration_error", "evaluate_model", "evaluate_checkpoint", "save_evaluation_results"):
        assert callable(getattr(EV, name)) and getattr(E, name) is getattr(EV, name)
    from inference.hmc import HMCResult
    from inference.vi import VariationalInference
    assert callable(HMCResult.predictive_summary) and callable(VariationalInference.predictive_summary)
    for sym in ("hode_pred_fold_f32", "hode_pred_fold_f64", "hode_pred_score_f32", "hode_pred_score_f64"):
        assert sym in hode.capi.SYMBOLS


def test_bad_arguments_are_refused_by_return_code_without_gpu():
    lib = hode.load()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    i64 = ctypes.c_int64
    for sfx in ("f32", "f64"):
        fold, score = getattr(lib, "hode_pred_fold_" + sfx), getattr(lib, "hode_pred_score_" + sfx)
        st = [one] * 6
        assert fold(z, 1, i64(20), one, z, z, z, z, i64(0), *st) == -1                    # N % 6
        assert fold(z, 1, i64(0), one, z, z, z, z, i64(0), *st) == -1                     # N < 6
        assert fold(z, -1, i64(18), one, z, z, z, z, i64(0), *st) == -1                   # n_draws < 0
        assert fold(z, 1, i64(18), z, z, z, z, z, i64(0), *st) == -1                      # no y
        for k in range(6):
            assert fold(z, 1, i64(18), one, z, z, z, z, i64(0), *(st[:k] + [z] + st[k + 1:])) == -1          # a null state pointer
        assert fold(z, 1, i64(18), one, z, one, z, z, i64(0), *st) == -1                  # a mask without obs
        assert fold(z, 1, i64(36), one, z, z, z, one, i64(24), *st) == -1                 # row_len does not divide N
        assert fold(z, 1, i64(36), one, z, z, z, one, i64(9), *st) == -1                  # row_len % 6
        assert fold(z, 0, i64(18), z, z, z, z, z, i64(0), *st) == 0                       # nothing to fold: no launch
        thr = (ctypes.c_double * 40)(*([0.0] * 40))
        out = [one] * 5
        assert score(z, i64(20), *st, z, z, z, thr, 10, *out) == -1                       # N % 6
        assert score(z, i64(18), *st, z, z, z, thr, 0, *out) == -1                        # n_bins range
        assert score(z, i64(18), *st, z, z, z, thr, 33, *out) == -1
        assert score(z, i64(18), *st, z, z, z, z, 10, *out) == -1                         # no thresholds
        for k in range(6):
            assert score(z, i64(18), *(st[:k] + [z] + st[k + 1:]), z, z, z, thr, 10, *out) == -1
        for k in range(5):
            assert score(z, i64(18), *st, z, z, z, thr, 10, *(out[:k] + [z] + out[k + 1:])) == -1
        assert score(z, i64(18), *st, z, one, z, thr, 10, *out) == -1                     # a mask without obs


def test_metric_functions_raise_hode_error_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from eval.evaluate import compute_calibration_error, compute_mae, compute_rmse
    from inference.predictive import PredictiveAccumulator
    p = torch.zeros(2, 3, 6)
    for call in (lambda: compute_rmse(p, p), lambda: compute_mae(p, p, per_state=True), lambda: compute_calibration_error(p, p + 1, p),
                 lambda: PredictiveAccumulator(2, 3)):
        with pytest.raises(hode.HodeError):
            call()


def test_welford_agrees_with_two_pass_long_double():
    """The restatement's sequential Welford against a two-pass np.longdouble computation on every input of the GPU tests
    (shapes PR.SHAPES, S in 1, 2, 7, 19, fp32- and fp64-valued inputs).  Observed maxima of the relative differences: mean 2.2e-16,
    m2 (entries with n >= 2) 1.6e-13, sd 7.8e-14; WELFORD_BOUND = 1.1e-12 covers them, and the GPU tests use 10 x WELFORD_BOUND."""
    worst = {"mean": 0.0, "m2": 0.0, "sd": 0.0}
    for n_traj, T in PR.SHAPES:
        for S in (1, 2, 7, 19):
            for dt in (np.float32, np.float64):
                c = PR.make_case(n_traj, T, S, dt)
                st = PR.fold(PR.fresh_state(c["N"]), c["y"], status=c["status"])
                n, mean, m2 = PR.two_pass(c["y"], c["status"], n_traj)
                assert np.array_equal(st["n"], n)
                has, two = n >= 1, n >= 2
                worst["mean"] = max(worst["mean"], float(np.max(np.abs(st["mean"][has] - mean[has]) / np.abs(mean[has]))))
                if two.any():
                    worst["m2"] = max(worst["m2"], float(np.max(np.abs(st["m2"][two] - m2[two]) / m2[two])))
                    sd, sdl = np.sqrt(st["m2"][two] / (n[two] - 1)), np.sqrt(m2[two] / (n[two] - 1))
                    worst["sd"] = max(worst["sd"], float(np.max(np.abs(sd - sdl) / sdl)))
                if S >= 3 and n_traj >= 2:                    # the failed draw's zero rows were not averaged in
                    lo = (n_traj - 1) * T * 6 + (T // 3) * 6
                    assert (n[lo:] <= S - 1).all() and np.all(st["mean"][lo:][n[lo:] > 0] > 0.3 * np.tile(PR.SCALE, T)[(T // 3) * 6:][n[lo:] > 0])
    print("welford vs two-pass, max relative:", worst)
    assert max(worst.values()) <= WELFORD_BOUND, worst


def test_split_folds_of_the_restatement_are_bit_identical_and_inputs_are_clear_of_edges():
    """The property the kernel must have holds for its restatement, and the chosen inputs have no value within 1e-9 of a
    threshold, an interval bound or a PIT bin edge (so the GPU tests may ask for exact counts)."""
    for n_traj, T in PR.SHAPES:
        for dt in (np.float32, np.float64):
            for mode in ("none", "zero", "pos"):
                for S in (2, 7, 19):
                    c = PR.make_case(n_traj, T, S, dt)
                    sig = {"none": None, "zero": np.zeros((S, 6)), "pos": c["sigma"]}[mode]
                    a = PR.fold(PR.fresh_state(c["N"]), c["y"], c["obs"], c["mask"], sig, c["status"])
                    if S == 7:
                        b = PR.fresh_state(c["N"])
                        for lo, hi in ((0, 3), (3, 6), (6, 7)):
                            PR.fold(b, c["y"][lo:hi], c["obs"], c["mask"], None if sig is None else sig[lo:hi], c["status"][lo:hi])
                        for k in PR.STATE_KEYS:
                            assert np.array_equal(a[k], b[k], equal_nan=True), k
                    ev = None if mode != "pos" else (sig ** 2).mean(0)
                    *_, table, edges = PR.score(a, c["obs"], c["mask"], ev, PR.thresholds(10))
                    assert PR.clear_of_edges(edges), (n_traj, T, dt, mode, S)
                    assert table[PR.UNSEEN_STATE].sum() == 0
                    m = PR.metrics(table, 10)
                    assert np.isnan(m["rmse_per_state"][PR.UNSEEN_STATE]) and np.isfinite(m["rmse"])
