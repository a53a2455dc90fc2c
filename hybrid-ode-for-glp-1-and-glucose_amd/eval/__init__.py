"""Evaluation metrics of the reference's `eval` package (eval/evaluate.py), scored on the GPU (csrc/hode_predictive.hip)."""
from .evaluate import (compute_calibration_error, compute_mae, compute_rmse, evaluate_checkpoint, evaluate_model,  # noqa: F401
                       save_evaluation_results)

__all__ = ["compute_rmse", "compute_mae", "compute_calibration_error", "evaluate_model", "evaluate_checkpoint", "save_evaluation_results"]
