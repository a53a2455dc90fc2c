"""Posterior-predictive summaries and their scores on the GPU, without the stack of draws (csrc/hode_predictive.hip;
include/hode.h, "Posterior-predictive summaries").

`HMCResult.predict` and `VariationalInference.posterior_predictive` hold every draw's trajectories, [draws, B, T, 6], to reduce
them to a mean and a standard deviation per entry.  Here the draws are FOLDED into a per-entry running state as they are
produced (`PredictiveAccumulator.fold`: Welford's update, the predictive CDF at the observation, a streaming log-sum-exp of
the pointwise log density), a piece of draws at a time, so memory depends on one piece and not on all of them; `finish` scores
the state against the data in one deterministic pass and `PredictiveSummary.metrics()` names the sums.

Folding the same draws in any split into consecutive `fold` calls gives bit-identical state (the kernel takes the draws one at
a time in draw order and the state is fp64 in memory as in registers), so `max_bytes` changes memory and nothing else.

With `quantiles=` the fold also keeps the few smallest and largest values of every entry (`tail_size` of them: a tail quantile
is interpolated between two order statistics near its end), and `finish` turns them into the exact empirical quantiles of the
draws -- the credible bands of the reference's third figure -- again whatever the split.

With `loo=True` the fold also keeps, per observed entry, what Pareto-smoothed importance-sampling leave-one-out cross-validation
and WAIC need of the pointwise log likelihood -- its `loo_tail_size` largest importance ratios and running sums over the rest
(csrc/hode_loo.hip) -- and `finish` turns them into `PredictiveSummary.loo`, a `LooResult`; `compare` ranks fitted models by
it."""
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

import hode

__all__ = ["PredictiveAccumulator", "PredictiveSummary", "predictive_summary", "cut_draws", "half_normal_thresholds", "tail_size",
           "loo_tail_size", "LooResult", "compare", "STATE_NAMES", "TABLE_COLUMNS", "BAND_COLUMNS", "LOO_COLUMNS"]

STATE_NAMES = ("glucose", "insulin", "glucagon", "glp1", "ge", "ffa")
# the fixed columns of the score table (include/hode.h); the n_bins threshold counts and the n_bins PIT counts follow
TABLE_COLUMNS = ("count", "sum_sq_err", "sum_abs_err", "sum_obs", "sum_obs_sq", "count_unc", "sum_sd", "sum_norm_err", "sum_interval_score",
                 "cover_50", "cover_80", "cover_90", "cover_95", "sum_crps", "sum_lppd", "count_lppd")
# the columns of the band table (include/hode.h, "Posterior bands")
BAND_COLUMNS = ("count", "sum_width", "cover", "sum_interval_score")
# the columns of the LOO table (include/hode.h, "Model comparison")
LOO_COLUMNS = ("count", "sum_elpd_loo", "sum_elpd_loo_sq", "sum_p_loo", "sum_elpd_waic", "sum_elpd_waic_sq", "sum_p_waic", "sum_lppd",
               "k_good", "k_ok", "k_bad", "k_very_bad", "p_waic_large")
_DEFAULT_MAX_BYTES = 256 << 20


def half_normal_thresholds(n_bins: int) -> List[float]:
    """The exact thresholds of the calibration curve: t_j with P(|Z| <= t_j) = j / n_bins, j = 0 .. n_bins - 1, i.e.
    sqrt(2) erfinv(j / n_bins).  (The reference estimates each from 10 000 fresh |randn| per call, eval/evaluate.py:134-138, so
    its ECE changes from call to call; these are what its percentiles converge to.)"""
    c = torch.arange(n_bins, dtype=torch.float64) / n_bins
    return (math.sqrt(2.0) * torch.erfinv(c)).tolist()


def cut_draws(n_draws: int, bytes_per_draw: int, max_bytes: int) -> List[Tuple[int, int]]:
    """Cut draws 0 .. n_draws - 1 into consecutive pieces [lo, hi) whose trajectories fit max_bytes (at least one draw per
    piece): every draw once, in order."""
    if n_draws < 0 or bytes_per_draw < 1:
        raise ValueError("cut_draws: n_draws >= 0 and bytes_per_draw >= 1")
    per = max(1, int(max_bytes) // int(bytes_per_draw))
    return [(lo, min(lo + per, n_draws)) for lo in range(0, n_draws, per)]


def _levels(quantiles) -> List[float]:
    lv = sorted({float(q) for q in quantiles})
    if not lv or not all(0.0 < q < 1.0 for q in lv) or len(lv) > hode.capi.PRED_MAX_LEVELS:
        raise ValueError(f"quantiles must be 1..{hode.capi.PRED_MAX_LEVELS} fractions strictly inside (0, 1)")
    return lv


def tail_size(levels: Sequence[float], n_draws: int) -> int:
    """How many of the smallest and of the largest values of an entry the quantiles at `levels` (fractions in (0, 1)) of n_draws
    draws need: the quantile q is interpolated between order statistics floor(q (n - 1)) and the next one, counted from the
    nearer end, so min(n_draws, max over the levels of floor(min(q, 1 - q) (n_draws - 1)) + 2).  26 of 1 000 draws at 2.5 %."""
    n = int(n_draws)
    lv = [float(q) for q in levels]
    if n < 1 or not lv or not all(0.0 < q < 1.0 for q in lv):
        raise ValueError("tail_size: n_draws >= 1 and levels strictly inside (0, 1)")
    return min(n, max(int(math.floor(min(q, 1.0 - q) * float(n - 1))) + 2 for q in lv))


def loo_tail_size(n_draws: int, r_eff: float = 1.0) -> int:
    """How many of the largest importance ratios of an entry PSIS needs of n_draws draws: M + 1 with the tail length
    M = ceil(min(n / 5, 3 sqrt(n / r_eff))) of Vehtari et al. 2024 (the extra one is the cut).  53 of 300 draws, 97 of 1 024.
    The kernel computes the same M in the same fp64 arithmetic from the draws it actually counted."""
    n, r = int(n_draws), float(r_eff)
    if n < 1 or not 0.0 < r <= 1.0:
        raise ValueError("loo_tail_size: n_draws >= 1 and r_eff in (0, 1]")
    return int(math.ceil(min(float(n) / 5.0, 3.0 * math.sqrt(float(n) / r)))) + 1


def _device():
    if not torch.cuda.is_available():
        raise hode.HodeError("predictive summaries need a HIP device: the fold and score kernels have no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


class PredictiveSummary:
    """What `PredictiveAccumulator.finish` returns: `mean`, `std`, `pit` (working precision) and `n` (int32), all [B, T, 6] on
    the device -- std is unbiased like torch.std plus the mean noise variance, NaN where fewer than two draws were folded; pit is
    the mean predictive CDF at the observation, NaN where unobserved -- `table` (fp64 numpy [6, 16 + 2 n_bins], the per-state
    sums of include/hode.h, columns TABLE_COLUMNS then the threshold counts then the PIT histogram) and `metrics()`.

    When the accumulator was given `quantiles`: `levels` (the requested fractions, ascending), `quantiles` [Q, B, T, 6] (the
    exact empirical quantiles of the folded draws, numpy's "linear" method; NaN where no draw was folded), `band(level)`,
    `tails()` and, when the outer levels enclose 1/2 and there are observations, `band_table` (fp64 numpy [6, 4], columns
    BAND_COLUMNS) whose scores `metrics()` adds as band_width, band_coverage and band_interval_score.  Otherwise `levels` and
    `quantiles` are None.  `loo` is a `LooResult` when the accumulator was given loo=True, else None."""

    def __init__(self, mean, std, pit, n, table, thresholds, levels=None, quantiles=None, band_table=None, tails=None, loo=None):
        self.mean, self.std, self.pit, self.n = mean, std, pit, n
        self.table = np.asarray(table, dtype=np.float64)
        self.thresholds = list(thresholds)
        self.n_bins = len(self.thresholds)
        self.levels = None if levels is None else list(levels)
        self.quantiles = quantiles
        self.band_table = None if band_table is None else np.asarray(band_table, dtype=np.float64)
        self._tails = tails                            # a callable of the accumulator: the buffers are not copied
        self.loo = loo                                 # a LooResult when the accumulator was given loo=True

    def metrics(self) -> Dict[str, Union[float, np.ndarray]]:
        out = table_metrics(self.table, self.n_bins)
        if self.band_table is not None:
            out.update(band_metrics(self.band_table))
        return out

    def band(self, level: float = 0.95):
        """(lower, upper), each [B, T, 6]: the central credible band of mass `level`, i.e. the quantiles 1/2 - level/2 and
        1/2 + level/2, when that pair was requested; KeyError otherwise."""
        if self.levels is None:
            raise KeyError("no quantiles were requested")
        pair = []
        for q in (0.5 - 0.5 * float(level), 0.5 + 0.5 * float(level)):
            hit = [i for i, have in enumerate(self.levels) if abs(have - q) <= 1e-12]
            if not hit:
                raise KeyError(f"quantile {q} was not requested (levels {self.levels})")
            pair.append(self.quantiles[hit[0]])
        return pair[0], pair[1]

    def tails(self):
        """(lower, upper), each [K, B, T, 6] ascending and NaN-padded at the end: the K smallest and the K largest values every
        entry was given, i.e. the sorted contents of the accumulator's buffers (which this reads: it raises once the accumulator
        has folded further draws)."""
        if self._tails is None:
            raise KeyError("no quantiles were requested")
        return self._tails()


class LooResult:
    """PSIS-LOO and WAIC of one fitted model on one data set: the pointwise `elpd_loo`, `pareto_k`, `elpd_waic`, `p_waic`, `lppd`
    ([B, T, 6] device tensors in the working precision, NaN where the entry is unobserved, has no observation noise or fewer
    than two draws), `table` (fp64 numpy [6, 13], columns LOO_COLUMNS, per-state sums of the fp64 values) and `estimates()`.
    `r_eff` is the relative efficiency the tail length was computed with."""

    def __init__(self, elpd_loo, pareto_k, elpd_waic, p_waic, lppd, table, r_eff=1.0):
        self.elpd_loo, self.pareto_k, self.elpd_waic, self.p_waic, self.lppd = elpd_loo, pareto_k, elpd_waic, p_waic, lppd
        self.table = np.asarray(table, dtype=np.float64)
        if self.table.shape != (6, len(LOO_COLUMNS)):
            raise ValueError(f"table must be [6, {len(LOO_COLUMNS)}]")
        self.r_eff = float(r_eff)

    def estimates(self) -> Dict[str, Union[float, np.ndarray]]:
        """elpd_loo (the SUM over the scored entries), se = sqrt(count * var) of the pointwise values (ddof 0, as arviz), p_loo,
        looic = -2 elpd_loo; elpd_waic, se_waic, p_waic, waic = -2 elpd_waic; lppd; pareto_k_counts (k <= 0.5, (0.5, 0.7],
        (0.7, 1], > 1), n_p_waic_large (p_waic > 0.4), count -- pooled over the states and per state under `<key>_per_state`.
        NaN where nothing was scored: nothing raises."""
        col = {name: i for i, name in enumerate(LOO_COLUMNS)}

        def scores(r):
            c = r[..., col["count"]]
            some = c > 0
            cs = np.where(some, c, 1.0)
            nan = np.full(r.shape[:-1], np.nan)
            pick = lambda name: np.where(some, r[..., col[name]], nan)                                         # noqa: E731

            def se(s1, s2):
                var = np.maximum(r[..., col[s2]] / cs - (r[..., col[s1]] / cs) ** 2, 0.0)
                return np.where(some, np.sqrt(cs * var), nan)
            return {"elpd_loo": pick("sum_elpd_loo"), "se": se("sum_elpd_loo", "sum_elpd_loo_sq"), "p_loo": pick("sum_p_loo"),
                    "looic": -2.0 * pick("sum_elpd_loo"), "elpd_waic": pick("sum_elpd_waic"),
                    "se_waic": se("sum_elpd_waic", "sum_elpd_waic_sq"), "p_waic": pick("sum_p_waic"),
                    "waic": -2.0 * pick("sum_elpd_waic"), "lppd": pick("sum_lppd"),
                    "pareto_k_counts": r[..., col["k_good"]:col["k_very_bad"] + 1], "n_p_waic_large": r[..., col["p_waic_large"]],
                    "count": c}
        pooled, per = scores(self.table.sum(0)), scores(self.table)
        out = {k: (v if v.ndim else float(v)) for k, v in pooled.items()}
        out.update({f"{k}_per_state": v for k, v in per.items()})
        return out


def compare(results: Dict[str, Union["LooResult", "PredictiveSummary"]], ic: str = "loo") -> List[Dict[str, object]]:
    """Rank fitted models by expected log pointwise predictive density on the SAME data (what arviz.compare reports).  results:
    name -> LooResult (or a PredictiveSummary made with loo=True); ic: "loo" or "waic".  Returns one row per model, best first:
    {name, rank, elpd, se, p, elpd_diff (to the best, <= 0), dse (sqrt(n var) of the pointwise difference to the best over the n
    entries scored in both, ddof 1; 0 for the best), weight (pseudo-BMA: the softmax of elpd), warning (a Pareto k > 0.7 for
    "loo", a p_waic > 0.4 for "waic")}.  Raises when the models were not scored on the same entries."""
    if ic not in ("loo", "waic"):
        raise ValueError('ic must be "loo" or "waic"')
    if not results:
        raise ValueError("compare needs at least one result")
    loos = {}
    for name, r in results.items():
        r = r.loo if isinstance(r, PredictiveSummary) else r
        if not isinstance(r, LooResult):
            raise ValueError(f"{name!r} carries no LooResult (was its summary made with loo=True?)")
        loos[name] = r
    point = {name: torch.as_tensor(r.elpd_loo if ic == "loo" else r.elpd_waic).to(torch.float64) for name, r in loos.items()}
    first = next(iter(point))
    scored = ~torch.isnan(point[first])
    for name, v in point.items():
        if v.shape != point[first].shape or not torch.equal(~torch.isnan(v.to(scored.device)), scored):
            raise ValueError(f"{name!r} and {first!r} were not scored on the same entries: the comparison needs the same data")
    rows = []
    for name, r in loos.items():
        e = r.estimates()
        warn = bool(e["pareto_k_counts"][2:].sum() > 0) if ic == "loo" else bool(e["n_p_waic_large"] > 0)
        rows.append({"name": name, "elpd": e["elpd_loo" if ic == "loo" else "elpd_waic"], "se": e["se" if ic == "loo" else "se_waic"],
                     "p": e["p_loo" if ic == "loo" else "p_waic"], "warning": warn})
    rows.sort(key=lambda row: -row["elpd"] if row["elpd"] == row["elpd"] else float("inf"))
    best = rows[0]
    n = int(scored.sum())
    el = np.array([row["elpd"] for row in rows])
    with np.errstate(invalid="ignore"):
        w = np.exp(el - np.nanmax(el)) if n else np.full(len(rows), np.nan)
    w = w / w.sum()
    for rank, (row, wt) in enumerate(zip(rows, w)):
        d = (point[row["name"]].to(scored.device) - point[best["name"]].to(scored.device))[scored]
        row["rank"], row["weight"] = rank, float(wt)
        row["elpd_diff"] = float(row["elpd"] - best["elpd"])
        row["dse"] = float(torch.sqrt(n * d.var(unbiased=True))) if n > 1 and rank > 0 else (0.0 if rank == 0 else float("nan"))
    return rows


def band_metrics(band_table: np.ndarray) -> Dict[str, Union[float, np.ndarray]]:
    """The scores of a band table [6, 4] (BAND_COLUMNS): band_width, band_coverage and band_interval_score, pooled from the pooled
    sums and per state under `<key>_per_state`; NaN where no entry was scored."""
    t = np.asarray(band_table, dtype=np.float64)

    def scores(r):
        c = r[..., 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            over = lambda i: np.where(c > 0, r[..., i] / np.where(c > 0, c, 1.0), np.nan)                      # noqa: E731
            return {"band_width": over(1), "band_coverage": over(2), "band_interval_score": over(3)}
    out = {k: float(v) for k, v in scores(t.sum(0)).items()}
    out.update({f"{k}_per_state": v for k, v in scores(t).items()})
    return out


def table_metrics(table: np.ndarray, n_bins: int) -> Dict[str, Union[float, np.ndarray]]:
    """The scores of a table [6, 16 + 2 n_bins] (tables of several batches add): every key pooled over the states -- from the
    pooled sums, e.g. rmse = sqrt(sum sum e^2 / sum count), what the reference's flatten() computes -- and per state under
    `<key>_per_state` (arrays of 6).  rmse, mae, target_std (unbiased), count; over the entries with at least two draws: ece,
    msis, sharpness, coverage_50 / 80 / 90 / 95, mean_normalized_error, crps, pit_histogram (fractions, [n_bins]); lppd (the SUM
    of the log pointwise predictive densities) where observation noise defined one.  A state observed nowhere, or a score with
    nothing to average, is NaN: nothing raises or divides by zero."""
    t = np.asarray(table, dtype=np.float64)
    col = {name: i for i, name in enumerate(TABLE_COLUMNS)}
    F = len(TABLE_COLUMNS)
    conf = np.arange(n_bins) / n_bins

    def scores(r):                                     # r: [..., K] sums of one state or of all of them
        nan = np.full(r.shape[:-1], np.nan)
        with np.errstate(divide="ignore", invalid="ignore"):
            ce, cu, cl = r[..., col["count"]], r[..., col["count_unc"]], r[..., col["count_lppd"]]
            over = lambda name, c: np.where(c > 0, r[..., col[name]] / np.where(c > 0, c, 1.0), nan)          # noqa: E731
            var = (r[..., col["sum_obs_sq"]] - r[..., col["sum_obs"]] ** 2 / np.where(ce > 0, ce, 1.0)) / np.where(ce > 1, ce - 1.0, 1.0)
            freq = r[..., F:F + n_bins] / np.where(cu > 0, cu, 1.0)[..., None]
            out = {
                "count": ce,
                "rmse": np.sqrt(over("sum_sq_err", ce)),
                "mae": over("sum_abs_err", ce),
                "target_std": np.where(ce > 1, np.sqrt(np.maximum(var, 0.0)), nan),
                "ece": np.where(cu > 0, np.mean(np.abs(conf - freq), axis=-1), nan),
                "msis": over("sum_interval_score", cu),
                "sharpness": over("sum_sd", cu),
                "coverage_50": over("cover_50", cu), "coverage_80": over("cover_80", cu), "coverage_90": over("cover_90", cu),
                "coverage_95": over("cover_95", cu),
                "mean_normalized_error": over("sum_norm_err", cu),
                "crps": over("sum_crps", cu),
                "lppd": np.where(cl > 0, r[..., col["sum_lppd"]], nan),
                "pit_histogram": np.where((cu > 0)[..., None], r[..., F + n_bins:F + 2 * n_bins] / np.where(cu > 0, cu, 1.0)[..., None],
                                          np.nan),
            }
        return out
    pooled, per = scores(t.sum(0)), scores(t)
    out = {k: (v if v.ndim else float(v)) for k, v in pooled.items()}
    out.update({f"{k}_per_state": v for k, v in per.items()})
    return out


class PredictiveAccumulator:
    """The running state of n_traj x T x 6 entries on the device.  `fold(y, sigma=None, status=None)` adds draws,
    `finish(n_bins=10)` scores them.  observations [n_traj, T, 6] (NaN = missing) and observation_mask (bool, same shape) as in
    inference/observation.py; without observations only mean / std / n are produced and the table is empty.

    quantiles (keyword, fractions in (0, 1)) with expected_draws (the most draws that will be folded): `fold` also keeps the
    tail_size(quantiles, expected_draws) smallest and largest values of every entry (hode.capi.pred_tails) and `finish` turns
    them into the exact quantiles of the folded draws; like the rest of the state they do not depend on how the draws were cut.

    loo=True (keyword; needs observations and, in every `fold`, sigma; the same expected_draws): `fold` also folds the pointwise
    log likelihood (hode.capi.pred_loo_fold, loo_tail_size(expected_draws, r_eff) ratios kept per entry) and `finish` returns
    PSIS-LOO and WAIC as `PredictiveSummary.loo`.  r_eff: the relative efficiency of the draws (1 for independent draws)."""

    def __init__(self, n_traj: int, T: int, observations=None, observation_mask=None, dtype=torch.float32, *, quantiles=None,
                 expected_draws: Optional[int] = None, loo: bool = False, r_eff: float = 1.0):
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        if n_traj < 1 or T < 1:
            raise ValueError("n_traj and T must be >= 1")
        if observation_mask is not None and observations is None:
            raise ValueError("observation_mask needs observations")
        self.n_traj, self.T, self.dtype = int(n_traj), int(T), dtype
        self.N = self.n_traj * self.T * 6
        dev = self.device = _device()
        self.obs = self.mask = None
        if observations is not None:
            obs = torch.as_tensor(observations)
            if tuple(obs.shape) != (self.n_traj, self.T, 6):
                raise ValueError(f"observations must be [{self.n_traj}, {self.T}, 6]")
            self.obs = obs.to(dev, dtype).reshape(-1).contiguous()
            if observation_mask is not None:
                m = torch.as_tensor(observation_mask)
                if m.shape != obs.shape:
                    raise ValueError("observation_mask must have the shape of observations")
                self.mask = m.to(dev).ne(0).to(torch.uint8).reshape(-1).contiguous()
        self.state = hode.capi.pred_state(self.N, dev)
        self._var_sum = torch.zeros(6, dtype=torch.float64, device=dev)       # sum over the folded draws of sigma_k^2
        self.n_folded = 0
        self.levels = self.tail_state = self.expected_draws = None
        if quantiles is not None:
            self.levels = _levels(quantiles)
            if expected_draws is None or int(expected_draws) < 1:
                raise ValueError("quantiles need expected_draws >= 1: the number of draws that will be folded sizes the buffers")
            self.expected_draws = int(expected_draws)
            self.tail_state = hode.capi.pred_tail_state(self.N, tail_size(self.levels, self.expected_draws), dtype, dev)
        self._tail_version = 0
        self.loo_state, self.r_eff = None, float(r_eff)
        if loo:
            if self.obs is None:
                raise ValueError("loo needs observations: the likelihood of nothing is undefined")
            if expected_draws is None or int(expected_draws) < 1:
                raise ValueError("loo needs expected_draws >= 1: the number of draws that will be folded sizes the buffer")
            self.expected_draws = int(expected_draws)
            self.loo_state = hode.capi.pred_loo_state(self.N, loo_tail_size(self.expected_draws, self.r_eff), dev)

    @classmethod
    def from_moments(cls, predictions, uncertainties, observations, observation_mask=None, dtype=None):
        """An accumulator whose state IS the given mean and standard deviation ([B, T, 6] each; two pseudo-draws per entry, so
        std = uncertainties exactly): what the metric functions of eval/evaluate.py score.  uncertainties=None: one draw."""
        p = torch.as_tensor(predictions)
        if p.dim() != 3 or p.shape[2] != 6:
            raise ValueError("predictions must be [batch, time, 6]")
        dtype = dtype or (torch.float64 if p.dtype == torch.float64 else torch.float32)
        acc = cls(p.shape[0], p.shape[1], observations, observation_mask, dtype)
        acc.state["mean"].copy_(p.to(acc.device, torch.float64).reshape(-1))
        if uncertainties is None:
            acc.state["n"].fill_(1)
        else:
            u = torch.as_tensor(uncertainties)
            if u.shape != p.shape:
                raise ValueError("uncertainties must have the shape of predictions")
            acc.state["n"].fill_(2)
            acc.state["m2"].copy_(u.to(acc.device, torch.float64).reshape(-1) ** 2)
        return acc

    def _sigma(self, sigma, S):
        if sigma is None:
            return None
        s = torch.as_tensor(sigma, dtype=torch.float64).to(self.device)
        if s.dim() == 0 or s.numel() == 1:
            s = s.reshape(1, 1).expand(S, 6)
        elif s.dim() == 1 and s.numel() == 6:
            s = s.reshape(1, 6).expand(S, 6)
        if tuple(s.shape) != (S, 6) or not bool((s >= 0).all()):
            raise ValueError("sigma must be non-negative: a scalar, one value per state or [n_draws, 6]")
        return s.contiguous()

    def fold(self, y, sigma=None, status=None):
        """y: [n_draws, n_traj, T, 6] (or [n_traj, T, 6]: one draw) on the device; sigma: the observation noise of the draws,
        a scalar, six values or [n_draws, 6]; status: int [n_draws, n_traj], the solve statuses (non-zero: that trajectory of that
        draw is skipped whole; a non-finite y is skipped for its entry).  Returns self."""
        y = torch.as_tensor(y)
        if y.dim() == 3:
            y = y.unsqueeze(0)
        if y.dim() != 4 or tuple(y.shape[1:]) != (self.n_traj, self.T, 6):
            raise ValueError(f"y must be [n_draws, {self.n_traj}, {self.T}, 6]")
        hode.capi._need_gpu(y)
        S = y.shape[0]
        if y.dtype != self.dtype:
            y = y.to(self.dtype)
        sig = self._sigma(sigma, S)
        if self.loo_state is not None and sig is None:
            raise ValueError("loo needs sigma in every fold: without observation noise there is no likelihood")
        if status is not None:
            status = torch.as_tensor(status).reshape(S, self.n_traj)
        y = y.reshape(S, self.N) if y.is_contiguous() else y
        hode.capi.pred_fold(y, self.state, self.obs, self.mask, sig, status)
        if self.tail_state is not None:
            hode.capi.pred_tails(y, self.tail_state, status)
            self._tail_version += 1
        if self.loo_state is not None:
            hode.capi.pred_loo_fold(y, self.loo_state, self.obs, self.mask, sig, status)
        if sig is not None:
            self._var_sum += (sig * sig).sum(0)
        self.n_folded += S
        return self

    def finish(self, n_bins: int = 10) -> PredictiveSummary:
        if not 1 <= int(n_bins) <= hode.capi.PRED_MAX_BINS:
            raise ValueError(f"n_bins must lie in 1..{hode.capi.PRED_MAX_BINS}")
        thr = half_normal_thresholds(int(n_bins))
        if self.loo_state is not None and self.n_folded > self.expected_draws:
            raise ValueError(f"{self.n_folded} draws were folded but the LOO buffer was sized for expected_draws = {self.expected_draws}")
        extra = (self._var_sum / max(self.n_folded, 1)).tolist()
        mean, sd, pit, table = hode.capi.pred_score(self.state, self.dtype, self.obs, self.mask, extra, thr)
        shape = (self.n_traj, self.T, 6)
        extra = {}
        if self.tail_state is not None:
            if self.n_folded > self.expected_draws:
                raise ValueError(f"{self.n_folded} draws were folded but the quantile buffers were sized for expected_draws = "
                                 f"{self.expected_draws}")
            band = self.obs is not None and self.levels[0] < 0.5 < self.levels[-1]
            q, bt = hode.capi.pred_quantiles(self.tail_state, self.levels, self.obs if band else None, self.mask if band else None, band)
            extra = dict(levels=self.levels, quantiles=q.view(len(self.levels), *shape), band_table=None if bt is None else bt.cpu().numpy(),
                         tails=self._tails_reader())
        if self.loo_state is not None:
            out, lt = hode.capi.pred_loo_finish(self.loo_state, self.dtype, self.r_eff)
            extra["loo"] = LooResult(*[out[k].view(shape) for k in hode.capi.PRED_LOO_OUTPUTS], lt.cpu().numpy(), self.r_eff)
        return PredictiveSummary(mean.view(shape), sd.view(shape), pit.view(shape), self.state["n"].view(shape).clone(),
                                 table.cpu().numpy(), thr, **extra)

    def _tails_reader(self):
        version = self._tail_version

        def read():
            if version != self._tail_version:
                raise RuntimeError("the accumulator has folded further draws since this summary was made: call finish() again")
            lower, upper = hode.capi.pred_tail_values(self.tail_state)                            # (finish() sorted the buffers)
            return lower.view(-1, self.n_traj, self.T, 6), upper.view(-1, self.n_traj, self.T, 6)
        return read


def _rep_inputs(S, x0, t_span, external_inputs):
    """The batch repeated for S parameter sets, as HybridODENN.forward_param_sets lays it out."""
    rep = lambda v: torch.as_tensor(v).repeat(*([S] + [1] * (torch.as_tensor(v).dim() - 1)))                  # noqa: E731
    t = torch.as_tensor(t_span)
    u = {}
    for k, v in (external_inputs or {}).items():
        big = v is not None and torch.as_tensor(v).dim() >= 1 and torch.as_tensor(v).numel() > 1
        u[k] = rep(v) if big else v
    return x0.repeat(S, 1), (rep(t) if t.dim() == 2 else t), u


def predictive_summary(model, draws, batch: Dict[str, torch.Tensor], sigma=None, n_bins: int = 10,
                       max_bytes: int = _DEFAULT_MAX_BYTES, solver: str = "dopri5", rtol: float = 1e-6, atol: float = 1e-8,
                       dtype=torch.float32, *, quantiles=None, loo: bool = False, r_eff: float = 1.0,
                       initial_states=None) -> PredictiveSummary:
    """The posterior-predictive summary of `draws` on `batch` {initial_state, time_points[, observations, observation_mask,
    external_inputs]}.  draws: a list of named parameter overrides (what `variational_params.sample` and `forward_param_sets`
    take), or a pair (nn_flat [S, P], ode_vec [S, 17]) of parameter tensors.  sigma: the observation noise, None, a scalar, six
    values or one row of six per draw.  The draws are cut into pieces whose trajectories fit max_bytes (`cut_draws`), each piece
    is ONE batched solve (no tape) and is folded with the solve's statuses before the next one starts: no more than one
    piece of trajectories exists at a time, and the result does not depend on the cut.  quantiles (fractions in (0, 1), e.g.
    (0.025, 0.975) for the 95 % credible band): also the exact empirical quantiles of the LATENT trajectories across the draws,
    `PredictiveSummary.quantiles` / `.band()`; sigma does not enter them.  loo=True (needs observations and sigma): also PSIS-LOO
    and WAIC of the pointwise log likelihood, `PredictiveSummary.loo`, with the relative efficiency r_eff of the draws.
    initial_states [S, B, 6]: every draw's own initial states of the batch's patients (inference/initial_state.py) instead of
    batch["initial_state"] under every draw."""
    if loo and sigma is None:
        raise ValueError("loo needs sigma: without observation noise there is no likelihood")
    from models.hybrid_ode_nn import _compute_device
    dev = _compute_device()
    x0 = batch["initial_state"]
    x0 = x0.unsqueeze(0) if x0.dim() == 1 else x0
    B = x0.shape[0]
    t = torch.as_tensor(batch["time_points"])
    T = t.shape[-1]
    named = not (isinstance(draws, tuple) and len(draws) == 2 and isinstance(draws[0], torch.Tensor))
    S = len(draws) if named else draws[0].shape[0]
    acc = PredictiveAccumulator(B, T, batch.get("observations"), batch.get("observation_mask"), dtype, quantiles=quantiles,
                                expected_draws=None if quantiles is None and not loo else max(S, 1), loo=loo, r_eff=r_eff)
    sig = acc._sigma(sigma, S)
    if initial_states is not None and tuple(initial_states.shape) != (S, B, 6):
        raise ValueError(f"initial_states must be [S, B, 6] = [{S}, {B}, 6], not {list(initial_states.shape)}")
    for lo, hi in cut_draws(S, B * T * 6 * 4, max_bytes):                         # (the solve's trajectories are fp32)
        n = hi - lo
        if named:
            flat = [model._params_on(dev, p) for p in draws[lo:hi]]
            nn_flat, ode_vec = torch.cat([f[0] for f in flat]), torch.cat([f[1] for f in flat])
        else:
            nn_flat = draws[0][lo:hi].to(dev, torch.float32).reshape(-1).contiguous()
            ode_vec = draws[1][lo:hi].to(dev, torch.float32).reshape(-1).contiguous()
        xs, ts, us = _rep_inputs(n, x0, t, batch.get("external_inputs"))
        if initial_states is not None:
            xs = initial_states[lo:hi].reshape(n * B, 6).to(x0.dtype)
        with torch.no_grad():
            y = model._solve(xs, ts, us, solver, rtol, atol, n_sets=n, nn_flat=nn_flat, ode_vec=ode_vec, differentiable=False)
        info = model.last_solve_info
        model._warn_failures(info)
        acc.fold(y.view(n, B, T, 6), None if sig is None else sig[lo:hi], info["status"].view(n, B))
        del y
    return acc.finish(n_bins)
