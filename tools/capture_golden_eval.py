#!/usr/bin/env python3
"""Capture the reference's evaluation metrics (eval/evaluate.py: compute_rmse, compute_mae, compute_calibration_error) on
two seeded inputs into tests/golden/eval/calibration.npz -- numbers only, no program text.

    python tools/capture_golden_eval.py <reference repository root>

Runs on the CPU and needs the reference repository (with sklearn and pandas, which its module imports); the test suite needs
neither, only the fixture.  The reference's `inference` package imports arviz, which evaluate.py does not use: a placeholder
stands in for `inference.vi` while evaluate.py is loaded from its file.

Inputs, fp64 so that the reference's NumPy arithmetic is fp64: [4, 13, 6] and [37, 61, 6] -- targets on the scale of the six
states, predictions = targets + heteroscedastic error, uncertainties of the right order but deliberately miscalibrated per
state.  Outputs per input: msis, sharpness, coverage_95, mean_normalized_error (deterministic in the reference: one value);
ece_min / ece_max over np.random.seed(0..39) (the reference draws its thresholds afresh on every call); compute_rmse and
compute_mae overall and per state."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

SHAPES = {"a": (4, 13, 6), "b": (37, 61, 6)}
SCALE = np.array([120.0, 15.0, 60.0, 8.0, 0.5, 0.4])
MISCAL = np.array([1.0, 0.6, 1.5, 0.9, 2.0, 0.75])


def inputs(tag):
    rng = np.random.default_rng({"a": 11, "b": 12}[tag])
    shape = SHAPES[tag]
    targets = SCALE * (1.0 + 0.2 * rng.standard_normal(shape))
    sd = 0.05 * SCALE * (0.5 + rng.random(shape))
    predictions = targets + sd * rng.standard_normal(shape)
    return predictions, sd * MISCAL, targets


def main(ref_root):
    sys.path.insert(0, ref_root)
    vi = types.ModuleType("inference.vi")
    vi.VariationalInference = object
    pkg = types.ModuleType("inference")
    pkg.vi = vi
    sys.modules.setdefault("inference", pkg)
    sys.modules.setdefault("inference.vi", vi)
    spec = importlib.util.spec_from_file_location("ref_evaluate", os.path.join(ref_root, "eval", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    out = {}
    for tag in SHAPES:
        p, u, t = inputs(tag)
        tp, tu, tt = (torch.from_numpy(v) for v in (p, u, t))
        out[f"{tag}_predictions"], out[f"{tag}_uncertainties"], out[f"{tag}_targets"] = p, u, t
        eces = []
        for seed in range(40):
            np.random.seed(seed)
            c = ev.compute_calibration_error(tp, tu, tt)
            eces.append(float(c["ece"]))
        for k in ("msis", "sharpness", "coverage_95", "mean_normalized_error"):
            out[f"{tag}_{k}"] = np.float64(c[k])
        out[f"{tag}_ece_min"], out[f"{tag}_ece_max"] = np.float64(min(eces)), np.float64(max(eces))
        out[f"{tag}_rmse"], out[f"{tag}_mae"] = np.float64(ev.compute_rmse(tp, tt)), np.float64(ev.compute_mae(tp, tt))
        out[f"{tag}_rmse_per_state"] = np.asarray(ev.compute_rmse(tp, tt, per_state=True), dtype=np.float64)
        out[f"{tag}_mae_per_state"] = np.asarray(ev.compute_mae(tp, tt, per_state=True), dtype=np.float64)
        print(tag, {k: float(out[f"{tag}_{k}"]) for k in ("ece_min", "ece_max", "msis", "sharpness", "coverage_95", "mean_normalized_error")})
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "eval")
    os.makedirs(dst, exist_ok=True)
    np.savez_compressed(os.path.join(dst, "calibration.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
