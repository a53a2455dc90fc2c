"""Variance-based sensitivity analysis on the GPU: the Sobol study of the reference's plots/plot_all.py:139-224 from the design
to the indices (csrc/hode_sobol.hip; include/hode.h, "Sobol indices").

    saltelli_design   Saltelli's sampling design over a box, in SALib's block layout (A, AB_1..AB_D, [BA_1..BA_D,] B per base
                      sample).  SALib is not a dependency: the base sample is SciPy's scrambled Sobol sequence.
    sobol_indices     what SALib.analyze.sobol.analyze computes, for any number of output columns at once: first-order, total
                      and second-order indices with bootstrap confidence intervals, by one kernel launch.
    sobol_study       design -> HybridODENN.forward_ode_sets (one launch for all parameter sets) -> outputs -> indices.

With the solve at a few milliseconds the outputs need not be three scalars: `time_resolved=True` analyses every state at every
grid point of the same trajectories, e.g. which constant drives glucose 40 minutes after the meal."""
from statistics import NormalDist

import numpy as np
import torch

import hode

__all__ = ["SobolIndices", "saltelli_design", "sobol_indices", "sobol_study"]

_KEYS = ("S1", "S1_conf", "ST", "ST_conf", "S2", "S2_conf")
DEFAULT_OUTPUTS = ("glucose_auc", "insulin_peak", "glp1_response")


class SobolIndices:
    """The result of `sobol_indices`: fp64 device tensors S1, S1_conf, ST, ST_conf [..., D], S2, S2_conf [..., D, D] (None
    without second order; NaN off the pairs j < k) and variance [...], where ... are the trailing dimensions of the analysed
    outputs; `names` are the D parameter names (or None).  `Si["S1"]` reads like SALib's result dict; `.numpy()` gives a dict
    of arrays.  A study adds `n_dropped`, `outputs` and `resolved`."""

    def __init__(self, S1, S1_conf, ST, ST_conf, S2, S2_conf, variance, names=None):
        self.S1, self.S1_conf, self.ST, self.ST_conf, self.S2, self.S2_conf = S1, S1_conf, ST, ST_conf, S2, S2_conf
        self.variance, self.names = variance, (None if names is None else list(names))
        self.n_dropped, self.outputs, self.resolved = 0, None, None

    def keys(self):
        return [k for k in _KEYS if getattr(self, k) is not None]

    def __contains__(self, key):
        return key in self.keys()

    def __getitem__(self, key):
        if key not in _KEYS and key not in ("variance", "names"):
            raise KeyError(key)
        return getattr(self, key)

    def numpy(self):
        out = {k: getattr(self, k).cpu().numpy() for k in self.keys()}
        out["variance"] = self.variance.cpu().numpy()
        if self.names is not None:
            out["names"] = list(self.names)
        return out

    def __repr__(self):
        return f"SobolIndices(S1{tuple(self.S1.shape)}, second_order={self.S2 is not None}, names={self.names})"


def _box(bounds):
    """(names or None, lo[D], hi[D]) of a dict name -> (lo, hi) or a sequence of (lo, hi)."""
    names = list(bounds.keys()) if isinstance(bounds, dict) else None
    box = np.array(list(bounds.values()) if names is not None else bounds, dtype=np.float64)
    if box.ndim != 2 or box.shape[0] < 1 or box.shape[1] != 2:
        raise ValueError("bounds must be D pairs (lo, hi)")
    return names, box


def saltelli_design(bounds, n=1024, calc_second_order=True, seed=0):
    """Saltelli's design for first-order, total and (with calc_second_order) second-order indices: [n * nb, D] float64 with
    nb = 2 D + 2 blocks per base sample (D + 2 without second order), row i * nb + b = block b of base sample i in SALib's order:
    A, AB_1..AB_D (A with column j from B), BA_1..BA_D (B with column j from A), B.  The base sample is SciPy's scrambled Sobol
    sequence in 2 D columns (A from the first D, B from the rest) scaled to `bounds` (a dict name -> (lo, hi), or D pairs).
    n should be a power of two, as for every Sobol sequence."""
    from scipy.stats import qmc
    _, box = _box(bounds)
    D = box.shape[0]
    base = qmc.Sobol(d=2 * D, scramble=True, seed=seed).random(n)
    lo, hi = box.T
    A, Bm = lo + base[:, :D] * (hi - lo), lo + base[:, D:] * (hi - lo)
    nb = 2 * D + 2 if calc_second_order else D + 2
    rows = np.empty((n, nb, D))
    rows[:, 0] = A
    rows[:, -1] = Bm
    for i in range(D):
        rows[:, 1 + i] = A
        rows[:, 1 + i, i] = Bm[:, i]
        if calc_second_order:
            rows[:, 1 + D + i] = Bm
            rows[:, 1 + D + i, i] = A[:, i]
    return rows.reshape(-1, D)


def sobol_indices(Y, D, calc_second_order=True, num_resamples=100, conf_level=0.95, seed=0, names=None):
    """Sobol indices of model outputs Y evaluated on a `saltelli_design` (the arguments are SALib.analyze.sobol.analyze's).
    Y: [rows] or [rows, ...] on the device, fp32 or fp64, rows = n * nb in the design's order; every trailing element is an
    output of its own and the trailing shape is kept: trajectories [S, T, 6] give S1 [T, 6, D].  Confidence half-widths are
    norm.ppf(0.5 + conf_level / 2) times the standard deviation of `num_resamples` bootstrap estimates (resampling base samples,
    Philox stream 7 of `seed`).  An output that is constant over the design, or not finite somewhere, has NaN indices."""
    if not torch.is_tensor(Y):
        raise TypeError("Y must be a tensor on the device")
    if not 0.0 < conf_level < 1.0:
        raise ValueError("conf_level must be in (0, 1)")
    if names is not None and len(names) != D:
        raise ValueError(f"{len(names)} names for D = {D}")
    trail = tuple(Y.shape[1:])
    Y2 = Y.reshape(Y.shape[0], -1) if Y.dim() != 2 else Y
    out = hode.capi.sobol_indices(Y2, D, calc_second_order, num_resamples, seed, NormalDist().inv_cdf(0.5 + conf_level / 2))
    first = lambda k: out[k].reshape(*trail, D)                                                   # noqa: E731
    second = lambda k: None if out[k] is None else out[k].reshape(*trail, D, D)                    # noqa: E731
    return SobolIndices(first("S1"), first("S1_conf"), first("ST"), first("ST_conf"), second("S2"), second("S2_conf"),
                        out["variance"].reshape(trail), names)


def default_outputs(y, t_span, meal=None):
    """The reference study's three outputs (plots/plot_all.py:194-196) of trajectories y [S, T, 6] -> [S, 3] in fp64: the glucose
    AUC by the trapezoid rule on t_span, the insulin peak, the mean GLP-1 from the first grid point with a meal on (the start
    without one).  fp64 sums of the trajectories' values, so that the analysis sees no rounding of its own inputs."""
    t = torch.as_tensor(t_span).to(device=y.device, dtype=torch.float64).reshape(-1)
    g = y[:, :, 0].double()
    auc = ((g[:, 1:] + g[:, :-1]) * 0.5 * (t[1:] - t[:-1])).sum(1)
    first = 0
    if meal is not None:
        on = torch.nonzero(torch.as_tensor(meal).reshape(-1, y.shape[1]).ne(0).any(0)).flatten()
        first = int(on[0]) if on.numel() else 0
    return torch.stack([auc, y[:, :, 1].double().max(1).values, y[:, first:, 3].double().mean(1)], 1)


def sobol_study(model, bounds, initial_state, t_span, external_inputs=None, n=1024, outputs=None, time_resolved=False,
                calc_second_order=True, num_resamples=100, conf_level=0.95, seed=0, solver="dopri5", rtol=1e-6, atol=1e-8):
    """The sensitivity study of plots/plot_all.py:139-224 for ONE patient: `bounds` (dict: ODECore constant -> (lo, hi)) ->
    `saltelli_design` -> all n * nb parameter sets through `model.forward_ode_sets` in one launch -> outputs -> `sobol_indices`.

    outputs=None analyses the reference's three (`default_outputs`; S1 [3, D]); otherwise a callable y [S, T, 6] -> [S, K].
    time_resolved=True analyses y itself as well: the result's `.resolved` is a SobolIndices with S1 [T, 6, D] (the initial row
    and a state that never moves are constant over the design: their indices are NaN).  A base sample with a failed solve in any
    of its blocks is dropped whole before the analysis (`.n_dropped`); more than 10 % dropped raises."""
    if not isinstance(bounds, dict):
        raise TypeError("bounds must be a dict: constant name -> (lo, hi)")
    names, box = _box(bounds)
    D = len(names)
    x0 = torch.as_tensor(initial_state)
    if x0.numel() != 6:
        raise ValueError("sobol_study varies the constants of ONE patient: initial_state must hold 6 values")
    design = saltelli_design(box, n, calc_second_order, seed)
    nb = design.shape[0] // n
    y = model.forward_ode_sets({k: torch.as_tensor(design[:, i], dtype=torch.float32) for i, k in enumerate(names)},
                               x0.reshape(6), t_span, external_inputs, solver=solver, rtol=rtol, atol=atol)
    status = model.last_solve_info["status"]
    y = y.to(status.device)
    failed = status.reshape(n, nb).ne(0).any(1)
    n_dropped = int(failed.sum())
    if n_dropped > 0.1 * n:
        raise RuntimeError(f"{n_dropped} of {n} base samples hold a failed solve: more than 10 %, the box leaves the model's range")
    if n_dropped:
        keep = torch.nonzero(~failed).flatten()
        y = y.reshape(n, nb, *y.shape[1:]).index_select(0, keep).reshape(-1, *y.shape[1:])
    if outputs is None:
        out, out_names = default_outputs(y, t_span, (external_inputs or {}).get("meal")), list(DEFAULT_OUTPUTS)
    else:
        out, out_names = outputs(y), None
        if out.dim() == 1:
            out = out.unsqueeze(1)
        if out.dim() != 2 or out.shape[0] != y.shape[0]:
            raise ValueError("outputs(y) must be [S, K]")
    args = dict(calc_second_order=calc_second_order, num_resamples=num_resamples, conf_level=conf_level, seed=seed, names=names)
    res = sobol_indices(out.contiguous(), D, **args)
    res.n_dropped, res.outputs = n_dropped, out_names
    if time_resolved:
        res.resolved = sobol_indices(y, D, **args)
        res.resolved.n_dropped = n_dropped
    return res
