"""The module surface of the reference's eval/evaluate.py -- compute_rmse, compute_mae, compute_calibration_error,
evaluate_model, evaluate_checkpoint, save_evaluation_results, with its signatures and return keys -- on the fold and score
kernels of csrc/hode_predictive.hip (inference/predictive.py).

The reference runs its posterior draws one solve after another, stacks them, and moves the stack to the CPU for sklearn.  Here
the draws of a batch are solved a piece at a time and folded into per-entry summaries on the device; every metric is a ratio
of the per-state sums of one score pass, and the sums of several batches add.  Nothing here runs without a HIP device: the
metric functions raise HodeError like the rest of the hot path.

One deliberate difference: the reference's ECE thresholds are percentiles of 10 000 fresh |randn| per call, so its ECE changes
from call to call; here they are the exact half-normal quantiles (`half_normal_thresholds`), which the reference's values
scatter around.  msis, sharpness, coverage_95 and mean_normalized_error are the reference's, deterministic there as here."""
import csv
import logging
from pathlib import Path
from typing import Dict, Optional, Union

import numpy as np
import torch

from inference.predictive import STATE_NAMES, PredictiveAccumulator, cut_draws, predictive_summary, table_metrics  # noqa: F401

logger = logging.getLogger(__name__)

_CALIBRATION_KEYS = ("ece", "msis", "sharpness", "coverage_95", "mean_normalized_error")
_DISPLAY_NAMES = ("Glucose", "Insulin", "Glucagon", "GLP1", "GE", "FFA")


def _scored(predictions, targets, uncertainties=None, n_bins=10):
    p = torch.as_tensor(predictions).detach()
    t = torch.as_tensor(targets).detach()
    if p.dim() != 3 or p.shape[2] != 6 or t.shape != p.shape:
        raise ValueError("predictions and targets must both be [batch, time, 6]")
    u = None if uncertainties is None else torch.as_tensor(uncertainties).detach()
    return PredictiveAccumulator.from_moments(p, u, t).finish(n_bins).metrics()


def compute_rmse(predictions: torch.Tensor, targets: torch.Tensor, per_state: bool = False) -> Union[float, np.ndarray]:
    """Root mean squared error of [batch, time, states] predictions: a float, or with per_state one value per state.
    Non-finite targets are missing and do not count."""
    m = _scored(predictions, targets)
    return m["rmse_per_state"] if per_state else m["rmse"]


def compute_mae(predictions: torch.Tensor, targets: torch.Tensor, per_state: bool = False) -> Union[float, np.ndarray]:
    """Mean absolute error, as compute_rmse."""
    m = _scored(predictions, targets)
    return m["mae_per_state"] if per_state else m["mae"]


def compute_calibration_error(predictions: torch.Tensor, uncertainties: torch.Tensor, targets: torch.Tensor,
                              n_bins: int = 10) -> Dict[str, float]:
    """{ece, msis, sharpness, coverage_95, mean_normalized_error} of predictive means and standard deviations
    ([batch, time, states] each) against the targets, with the reference's definitions: ece = the mean over the confidence
    levels c_j = j / n_bins of |c_j - fraction of |error| / (sd + 1e-6) <= t_j| (t_j the half-normal quantile of c_j); msis =
    the mean 95 % interval score (z = 1.96); sharpness = the mean sd; coverage_95 = the fraction inside mean +- 1.96 sd."""
    m = _scored(predictions, targets, uncertainties, n_bins)
    return {k: m[k] for k in _CALIBRATION_KEYS}


def _to_device(batch, device):
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to(device)
        elif isinstance(v, dict):
            out[k] = {kk: (vv.to(device) if isinstance(vv, torch.Tensor) else vv) for kk, vv in v.items()}
        else:
            out[k] = v
    return out


def evaluate_model(model, test_loader, device: torch.device, use_variational: bool = False, n_posterior_samples: int = 100,
                   noise_sigma=None, n_bins: int = 10, max_bytes: Optional[int] = None) -> Dict[str, float]:
    """The reference's evaluation of a model over a loader of batches {initial_state, observations, time_points[,
    external_inputs, observation_mask]}: rmse, mae, rmse_<state>, mae_<state>, nrmse, nrmse_<state>, and with use_variational
    also ece, msis, sharpness, coverage_95, mean_normalized_error.

    use_variational (and a model that has variational parameters): n_posterior_samples draws PER BATCH, one `sample(1)` at a
    time as the reference takes them, folded into mean and spread on the device; the calibration keys score the draws' own
    spread (noise_sigma=None), as in the reference.  Otherwise the point prediction is folded as one draw; asked for
    calibration keys then score the reference's fixed uncertainty of 0.1.  The target standard deviation of nrmse is the
    unbiased one over batch and time, from the score table's sums.  With noise_sigma (a scalar or one value per state) the
    predictive includes the observation noise and crps, lppd (sum) and pit_histogram are returned as well.  `device` is where
    the batches are moved, as in the reference; the work runs on the HIP device."""
    from inference.predictive import _DEFAULT_MAX_BYTES
    model.eval()
    max_bytes = _DEFAULT_MAX_BYTES if max_bytes is None else max_bytes
    variational = bool(use_variational) and getattr(model, "variational_params", None) is not None
    table = None
    with torch.no_grad():
        for batch in test_loader:
            batch = _to_device(batch, device)
            if variational:
                draws = [model.variational_params.sample(1)[0] for _ in range(n_posterior_samples)]
                summ = predictive_summary(model, draws, batch, sigma=noise_sigma, n_bins=n_bins, max_bytes=max_bytes)
            else:
                pred = model.forward(batch["initial_state"], batch["time_points"], batch.get("external_inputs"))
                if use_variational:
                    acc = PredictiveAccumulator.from_moments(pred, torch.full_like(pred, 0.1), batch["observations"],
                                                             batch.get("observation_mask"))
                else:
                    acc = PredictiveAccumulator(pred.shape[0], pred.shape[1], batch["observations"], batch.get("observation_mask"))
                    acc.fold(pred if pred.is_cuda else pred.to(acc.device), sigma=noise_sigma)
                summ = acc.finish(n_bins)
            table = summ.table if table is None else table + summ.table
    if table is None:
        raise ValueError("evaluate_model: the loader gave no batch")
    m = table_metrics(table, n_bins)
    out = {"rmse": m["rmse"], "mae": m["mae"]}
    for k, name in enumerate(STATE_NAMES):
        out[f"rmse_{name}"] = m["rmse_per_state"][k]
        out[f"mae_{name}"] = m["mae_per_state"][k]
    if use_variational:
        out.update({k: m[k] for k in _CALIBRATION_KEYS})
    out["nrmse"] = m["rmse"] / np.mean(m["target_std_per_state"])
    for k, name in enumerate(STATE_NAMES):
        out[f"nrmse_{name}"] = m["rmse_per_state"][k] / m["target_std_per_state"][k]
    if noise_sigma is not None and (variational or not use_variational):
        out["crps"], out["lppd"], out["pit_histogram"] = m["crps"], m["lppd"], m["pit_histogram"]
    return out


def evaluate_checkpoint(checkpoint_path: str, test_loader, device: torch.device, config: Optional[dict] = None) -> Dict[str, float]:
    """evaluate_model on a checkpoint {model_state_dict[, config, epoch, val_loss]}; the model is built from
    config["model"] (nn_hidden, nn_layers, use_variational), taken from the checkpoint unless given."""
    from models.hybrid_ode_nn import HybridODENN
    ck = torch.load(checkpoint_path, map_location=device, weights_only=False)
    config = ck.get("config") if config is None else config
    if config is None:
        raise ValueError("Configuration not found in checkpoint")
    mc = config.get("model", {})
    use_variational = bool(mc.get("use_variational", False))
    model = HybridODENN(ode_params=None, nn_hidden=mc.get("nn_hidden", 64), nn_layers=mc.get("nn_layers", 4),
                        use_variational=use_variational, device=device).to(device)
    model.load_state_dict(ck["model_state_dict"])
    out = evaluate_model(model, test_loader, device, use_variational)
    out["checkpoint_epoch"] = ck.get("epoch", -1)
    out["checkpoint_val_loss"] = ck.get("val_loss", -1)
    return out


def save_evaluation_results(metrics: Dict[str, float], output_path: str):
    """One CSV row of the scalar metrics at output_path and a readable report next to it (<output_path stem>.txt)."""
    flat = {k: (v.tolist() if isinstance(v, np.ndarray) else (float(v) if isinstance(v, (np.floating, float)) else v))
            for k, v in metrics.items()}
    with open(output_path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(flat))
        w.writeheader()
        w.writerow(flat)
    lines = ["Model Evaluation Results", "=" * 50, "", "Overall Metrics:", f"  RMSE: {metrics['rmse']:.4f}", f"  MAE: {metrics['mae']:.4f}",
             f"  Normalized RMSE: {metrics['nrmse']:.4f}", "", "Per-State RMSE:"]
    lines += [f"  {shown}: {metrics[f'rmse_{name}']:.4f}" for shown, name in zip(_DISPLAY_NAMES, STATE_NAMES) if f"rmse_{name}" in metrics]
    if "ece" in metrics:
        lines += ["", "Calibration Metrics:", f"  Expected Calibration Error: {metrics['ece']:.4f}",
                  f"  95% Coverage: {metrics['coverage_95']:.4f}", f"  Sharpness: {metrics['sharpness']:.4f}", f"  MSIS: {metrics['msis']:.4f}"]
    Path(output_path).with_suffix(".txt").write_text("\n".join(lines) + "\n")
    logger.info(f"Evaluation results saved to {output_path}")
