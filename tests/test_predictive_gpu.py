"""The fold and score kernels of csrc/hode_predictive.hip against their NumPy restatement (tests/_predictive_reference.py), in
fp32 and fp64, at the smallest shapes that reach every path (PR.SHAPES: N = 18, the scalar path alone; N = 390, rows with
N % 4 != 0 and more than one workgroup of the fold; N = 3348, the score pass's 16-byte path in two workgroups with a ragged
second one), with S = 1, 2 (less than the 16 draws in flight) and 7 draws, and S = 19 = 16 + 3 for the in-flight batch, missing and
masked observations, one state observed nowhere, a non-finite trajectory, a failed solve with zero rows, and the observation
noise absent, zero and positive.  `-m gpu`.

Tolerances.  fp64 mean, sd, pit and the table's sums: FP64_TOL = 1.1e-11 relative = 10 x the 1.1e-12 that
test_predictive_host.py measured for sequential Welford against two-pass long double on these very inputs (the factor covers
FMA contraction in the score pass and the device's erfc / exp / log).  fp32 outputs are the fp64 state rounded once: 2e-7
relative.  Counts are exact: the inputs have no value within 1e-9 of a threshold, interval bound or PIT bin edge (asserted)."""
from functools import lru_cache

import numpy as np
import pytest

import _predictive_reference as PR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

FP64_TOL = 1.1e-11
FP32_TOL = 2e-7
DTYPES = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
COUNT_COLS = [0, 5, 9, 10, 11, 12, 15] + list(range(16, 36))
SUM_COLS = [1, 2, 3, 4, 6, 7, 8, 13, 14]
THR = PR.thresholds(10)
DEV = "cuda"


def _sigma(c, mode, S):
    return {"none": None, "zero": np.zeros((S, 6)), "pos": c["sigma"]}[mode]


@lru_cache(maxsize=None)
def reference(n_traj, T, S, dt, mode):
    """Computed once per case and shared: the restatement's state and scores (never modified by the tests)."""
    c = PR.make_case(n_traj, T, S, DTYPES[dt][1])
    sig = _sigma(c, mode, S)
    st = PR.fold(PR.fresh_state(c["N"]), c["y"], c["obs"], c["mask"], sig, c["status"])
    ev = None if mode != "pos" else (sig ** 2).mean(0)
    mean, sd, pit, table, edges = PR.score(st, c["obs"], c["mask"], ev, THR)
    assert PR.clear_of_edges(edges)                            # (pick another seed in make_case if this ever fires)
    return c, st, (mean, sd, pit, table), ev


def kernel_fold(c, dt, mode, splits, offset=False):
    tdt = DTYPES[dt][0]
    S, N = c["y"].shape
    y = torch.tensor(c["y"], dtype=tdt, device=DEV)
    if offset:                                                  # the same values one element off the allocation's alignment
        buf = torch.empty(S * N + 1, dtype=tdt, device=DEV)
        buf[1:].copy_(y.reshape(-1))
        y = buf[1:].view(S, N)
        assert y.data_ptr() % 16 != 0
    obs = torch.tensor(c["obs"], dtype=tdt, device=DEV)
    mask = torch.tensor(c["mask"], device=DEV)
    sig = _sigma(c, mode, S)
    sig = None if sig is None else torch.tensor(sig, device=DEV)
    status = torch.tensor(c["status"], device=DEV)
    st = hode.capi.pred_state(N, DEV)
    for lo, hi in splits:
        hode.capi.pred_fold(y[lo:hi], st, obs, mask, None if sig is None else sig[lo:hi], status[lo:hi])
    return st, obs, mask


def check_state(st, ref):
    assert np.array_equal(st["n"].cpu().numpy(), ref["n"])
    for k in ("mean", "m2", "pit", "lsum", "lmax"):
        np.testing.assert_allclose(st[k].cpu().numpy(), ref[k], rtol=FP64_TOL, atol=0, err_msg=k)


def check_scores(out, ref, dt):
    tol = FP64_TOL if dt == "f64" else FP32_TOL
    for got, want, name in zip(out[:3], ref[:3], ("mean", "sd", "pit")):
        assert got.dtype == DTYPES[dt][0]
        np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), want, rtol=tol, atol=0, equal_nan=True, err_msg=name)
    table, want = out[3].cpu().numpy(), ref[3]
    assert np.array_equal(table[:, COUNT_COLS], want[:, COUNT_COLS])
    np.testing.assert_allclose(table[:, SUM_COLS], want[:, SUM_COLS], rtol=FP64_TOL, atol=0)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", PR.SHAPES)
@pytest.mark.parametrize("mode", ["none", "zero", "pos"])
@pytest.mark.parametrize("S", [2, 7, 19])
def test_fold_and_score_against_restatement(shape, S, dt, mode):
    c, ref_state, ref_out, ev = reference(*shape, S, dt, mode)
    st, obs, mask = kernel_fold(c, dt, mode, [(0, S)])
    check_state(st, ref_state)
    out = hode.capi.pred_score(st, DTYPES[dt][0], obs, mask, ev, THR)
    check_scores(out, ref_out, dt)
    table = out[3].cpu().numpy()
    assert (table[PR.UNSEEN_STATE] == 0).all()                  # a state observed nowhere: an all-zero row
    assert table[:, 0].sum() > 0 and table[:, 5].sum() > 0
    # the non-finite trajectory and the failed solve lowered n there, and the zero rows were not averaged in
    n = st["n"].cpu().numpy().reshape(shape[0], shape[1], 6)
    T = shape[1]
    assert (n[0, T // 2:] == S - 1).all() and (n[0, :T // 2] == S).all()
    if S >= 3 and shape[0] >= 2:
        assert (n[-1] == S - 1).all()
        mean = st["mean"].cpu().numpy().reshape(shape[0], T, 6)
        assert (mean[-1, T // 3:] > 0.8 * PR.SCALE).all()
    if mode == "pos":
        assert table[:, 15].sum() == table[:, 5].sum() > 0      # a log density wherever there is noise
    else:
        assert table[:, 14:16].sum() == 0 and bool(torch.isinf(st["lmax"]).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", PR.SHAPES)
def test_one_draw_has_no_uncertainty(shape, dt):
    c, ref_state, ref_out, ev = reference(*shape, 1, dt, "pos")
    st, obs, mask = kernel_fold(c, dt, "pos", [(0, 1)])
    check_state(st, ref_state)
    out = hode.capi.pred_score(st, DTYPES[dt][0], obs, mask, ev, THR)
    check_scores(out, ref_out, dt)
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isnan(out[2]).all()) and not bool(torch.isnan(out[0]).any())
    table = out[3].cpu().numpy()
    assert (table[:, 5:] == 0).all() and table[:, 0].sum() > 0


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", PR.SHAPES)
@pytest.mark.parametrize("mode", ["none", "pos"])
@pytest.mark.parametrize("S", [7, 19])
def test_split_folds_misaligned_views_and_reruns_give_the_same_bits(shape, dt, mode, S):
    """S = 7 in one call, split 3 + 3 + 1, draw by draw, 4 + 3, from a y view one element off its alignment, and again; S = 19
    (one batch of 16 draws in flight and a remainder of 3) the same with 3 + 3 + 13 and 4 + 15: all six state arrays are
    torch.equal, and so is everything the score pass writes."""
    c, _, _, ev = reference(*shape, S, dt, mode)
    whole, obs, mask = kernel_fold(c, dt, mode, [(0, S)])
    runs = {"3+3+rest": [(0, 3), (3, 6), (6, S)], "one by one": [(s, s + 1) for s in range(S)], "4+rest": [(0, 4), (4, S)], "again": [(0, S)]}
    for name, splits in runs.items():
        other, _, _ = kernel_fold(c, dt, mode, splits)
        for k in hode.capi.PRED_STATE:
            assert torch.equal(whole[k], other[k]), (name, k)
    off, _, _ = kernel_fold(c, dt, mode, [(0, S)], offset=True)
    for k in hode.capi.PRED_STATE:
        assert torch.equal(whole[k], off[k]), ("offset", k)
    a = hode.capi.pred_score(whole, DTYPES[dt][0], obs, mask, ev, THR)
    b = hode.capi.pred_score(other, DTYPES[dt][0], obs, mask, ev, THR)
    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)             # noqa: E731  (NaN == NaN)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))


def test_accumulator_surface_metrics_and_unobserved_state():
    """PredictiveAccumulator end to end on the N = 390 case: fold in two pieces, finish, metrics() -- equal to the restatement's,
    NaN (no exception, no division warning) for the state observed nowhere; without observations only mean / std / n."""
    import warnings
    from inference.predictive import PredictiveAccumulator
    n_traj, T = PR.SHAPES[1]
    c, _, ref_out, ev = reference(n_traj, T, 7, "f32", "pos")
    y = torch.tensor(c["y"], dtype=torch.float32, device=DEV).view(7, n_traj, T, 6)
    acc = PredictiveAccumulator(n_traj, T, torch.tensor(c["obs"]).view(n_traj, T, 6), torch.tensor(c["mask"]).view(n_traj, T, 6).bool())
    acc.fold(y[:4], torch.tensor(c["sigma"][:4]), torch.tensor(c["status"][:4]))
    acc.fold(y[4:], torch.tensor(c["sigma"][4:]), torch.tensor(c["status"][4:]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        summ = acc.finish(10)
        m = summ.metrics()
    assert summ.mean.shape == summ.std.shape == summ.pit.shape == summ.n.shape == (n_traj, T, 6)
    np.testing.assert_allclose(summ.std.cpu().numpy().reshape(-1), ref_out[1], rtol=FP32_TOL, equal_nan=True)
    want = PR.metrics(ref_out[3], 10)
    for k in ("rmse", "mae", "ece", "msis", "sharpness", "coverage_50", "coverage_95", "mean_normalized_error", "crps", "lppd", "target_std"):
        np.testing.assert_allclose(m[k], want[k], rtol=FP64_TOL, err_msg=k)
        np.testing.assert_allclose(m[k + "_per_state"], want[k + "_per_state"], rtol=FP64_TOL, equal_nan=True, err_msg=k)
        assert np.isnan(m[k + "_per_state"][PR.UNSEEN_STATE]) and np.isfinite(m[k])
    assert abs(m["pit_histogram"].sum() - 1.0) < 1e-12 and np.isnan(m["pit_histogram_per_state"][PR.UNSEEN_STATE]).all()
    bare = PredictiveAccumulator(n_traj, T).fold(y, status=torch.tensor(c["status"])).finish()
    assert torch.equal(bare.mean, summ.mean) and (bare.table == 0).all() and bool(torch.isnan(bare.pit).all())
    assert np.isnan(bare.metrics()["rmse"])
