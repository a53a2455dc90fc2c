"""An unscented (sigma-point) Kalman filter on the GPU: deterministic online state tracking, forecasts and a Gaussian
log-evidence for the model with process noise that `run_filter` samples (csrc/hode_ukf.hip; include/hode.h, "Unscented Kalman
filter").

    run_ukf      a mean and a covariance per patient in link space, carried from filter step to filter step by ONE forward
                 solve of the B * K sigma-point trajectories over that segment of the grid (K = 2 n + 1, n = 6 states + the
                 learned constants; the network shared, every point's 17 mechanistic constants in its own row) and ONE launch
                 of the step kernel: the unscented moments of the propagated points, the measurement update, the next points.
                 Nothing is read back to the host inside the loop, and there is no seed: the same call gives the same bits.
    UKFResult    the filtered moments, NIS, log-evidence increments, the final mean / covariance / sigma points; `forecast`
                 continues the same loop without observations; `smooth` (store_history=True) is the unscented Rauch-Tung-Striebel
                 pass over the stored run (csrc/hode_ukf_smooth.hip): a UKFSmoothResult, the state at
                 every step given the whole record.

The state model is `run_filter`'s: between two steps a state follows the deterministic solve; over a step of length dt it gains
noise of standard deviation process_noise * sqrt(dt) -- additive, or on the logarithm with the -s^2 / 2 drift that keeps the
mean -- so the two filters' evidences are evidences of the same model.  Learned constants (`learn`) are appended to the state:
the filter learns them jointly with it through their cross-covariance, without a shrinkage heuristic."""
import warnings

import numpy as np
import torch

import hode

from .filter import (LearnedParameters, ParameterLearning, _check_data, _check_steps, _default_steps, _inputs, _six_nonneg)
from .observation import ObservationModel

__all__ = ["UKFResult", "UKFSmoothResult", "run_ukf"]


class _Engine:
    """What one run and its forecasts share: the network and the settings on the device, and the loop."""

    def __init__(self, model, B, q, sigma, link, learn, weights, method, rtol, atol, dtype, dev, store):
        nl = model.nn_residual
        self.model, self.B, self.dtype, self.dev, self.learn, self.store = model, B, dtype, dev, learn, store
        self.H, self.L, self.method, self.rtol, self.atol = nl.hidden_dim, nl.hip_layers, method, float(rtol), float(atol)
        self.link, self.weights = link, weights
        self.mode = [0] * 17                                    # host integers: the ABI validates and sizes the launch from them
        walk = np.zeros(17)
        if learn is not None:
            for c in learn.columns:
                self.mode[c] = hode.capi.PF_MOVE[learn.link]
            walk = learn._full(learn.walk)
        self.n = 6 + sum(1 for v in self.mode if v)
        self.K = 2 * self.n + 1
        f64 = dict(dtype=torch.float64, device=dev)
        self.q, self.sigma, self.walk = torch.as_tensor(q, **f64), torch.as_tensor(sigma, **f64), torch.as_tensor(walk, **f64)

    def run(self, x, ode_p, mean, cov, alive, t, ins, obs, mask, idxs, init):
        """Carry the sigma points (x [B, K, 6], ode_p [B, K, 17]) over the grid t ([T] or [B, T]) with a filter step at every
        index of `idxs` (and, with init, one without a prediction at index 0, from the given mean [B, n] / cov [B, n, n]);
        obs [B, T, 6] / mask uint8 [B, T, 6] or None (no observations).  mean, cov and alive are updated in place.  Returns
        (x, ode_p, stats [S, B, 16], the mean [S, B, n] and the variances [S, B, n] in link space after every step, and with
        store the history (sigma points [S, B, K, 6], their constants [S, B, K, 17], covariances [S, B, n, n], the rows x_in every
        step was handed [S, B, K, 6], its dt [S, B]), else None)."""
        B, K, n, dev, dtype = self.B, self.K, self.n, self.dev, self.dtype
        with torch.no_grad():
            nn_flat, _ = self.model._params_on(dev)
            nn_flat = nn_flat.detach().to(dtype).contiguous()
            S = len(idxs) + bool(init)
            stats = torch.empty(S, B, hode.capi.UKF_COLS, dtype=torch.float64, device=dev)
            means = torch.empty(S, B, n, dtype=torch.float64, device=dev)
            variances = torch.empty(S, B, n, dtype=torch.float64, device=dev)
            hist = (torch.empty(S, B, K, 6, dtype=dtype, device=dev), torch.empty(S, B, K, 17, dtype=dtype, device=dev),
                    torch.empty(S, B, n, n, dtype=torch.float64, device=dev), torch.empty(S, B, K, 6, dtype=dtype, device=dev),
                    torch.empty(S, B, dtype=torch.float64, device=dev)) if self.store else None
            bufs, aux = [x, torch.empty_like(x)], [ode_p, torch.empty_like(ode_p)]
            nan_row = torch.full((B, 6), float("nan"), dtype=dtype, device=dev)
            per_patient = t.dim() == 2
            # the inputs per sigma point: a grid input [B, T] -> [B * K, T] once, sliced per segment; a constant [B] -> [B * K]
            rep = {k: (None if v is None else v.repeat_interleave(K, 0)) for k, v in ins.items()}
            t_rep = t.repeat_interleave(K, 0) if per_patient else t
            t64 = t.double()                                    # the step's dt: the exact difference of the grid's values
            s = 0

            def step(x_in, status, g, dt, predict):
                nonlocal s
                ob = nan_row if obs is None else obs[:, g].contiguous()
                mk = None if mask is None else mask[:, g].contiguous()
                hode.capi.ukf_step(x_in, aux[0], self.mode, ob, self.sigma, self.q, self.walk, dt, alive, mean, cov, self.weights,
                                   predict=predict, link=self.link, status=status, mask=mk, out=(bufs[1], aux[1], stats[s]))
                means[s].copy_(mean)
                variances[s].copy_(cov.diagonal(dim1=1, dim2=2))
                if self.store:                                  # copies only
                    hist[0][s].copy_(bufs[1])
                    hist[1][s].copy_(aux[1])
                    hist[2][s].copy_(cov)
                    hist[3][s].copy_(x_in)
                    hist[4][s].copy_(dt)
                bufs.reverse()
                aux.reverse()
                s += 1

            if init:
                step(bufs[0], None, 0, torch.ones(B, dtype=torch.float64, device=dev), False)
            prev = 0
            for g in idxs:
                seg = slice(prev, g + 1)
                cut = lambda v: None if v is None else (v[:, seg].contiguous() if v.dim() == 2 else v)          # noqa: E731
                sol = hode.solve_fwd(bufs[0].reshape(B * K, 6), t_rep[:, seg].contiguous() if per_patient else t[seg].contiguous(),
                                     cut(rep["meal"]), cut(rep["tVNS"]), cut(rep["GD"]), aux[0].reshape(-1), nn_flat, self.H, self.L,
                                     method=self.method, rtol=self.rtol, atol=self.atol, n_sets=B * K, nn_shared=True)
                dt = (t64[:, g] - t64[:, prev] if per_patient else (t64[g] - t64[prev]).expand(B)).contiguous()
                step(sol.y[:, -1].reshape(B, K, 6).contiguous(), sol.status.view(B, K), g, dt, True)
                prev = g
        return bufs[0], aux[0], stats, means, variances, hist


class UKFResult:
    """The result of `run_ukf` / `forecast`, tensors on the compute device.  S = the filter steps taken, the update of the initial
    moments at the first grid point included (a forecast has no such step).
      mean, std [B, S, 6]        the filtered moments of the states in natural space: the unscented mean and standard deviation of
                                 the sigma points after the step's update
      log_evidence_steps [B, S]  log p(obs at step s | obs before it) under the Gaussian approximation; `log_evidence()` is
                                 their sum
      nis [B, S]                 the normalised innovation squared r^T S^-1 r (chi-squared with n_seen degrees of freedom for a
                                 consistent filter);  n_seen [B, S] (int64) the number of states observed at the step
      alive [B, S] (bool)        False from the step at which a patient was lost (a failed solve, a non-finite or, under a log
                                 link, non-positive value): its increment is -inf, its moments NaN
      step_index [S]             the grid index of every step;  times [S] or [B, S]
      state_mean [B, n], state_cov [B, n, n]   the final moments in link space (fp64), n = 6 + the learned constants
      sigma_points [B, K, 6], ode_p [B, K, 17] the final sigma points (natural space) and their mechanistic constants
      learned                    a LearnedParameters (run_ukf(learn=...), else None): per step, location = the mean of every
                                 learned constant in link space and scale = the square root of its variance
      history [S, B, K, 6], ode_history [S, B, K, 17], mean_history [S, B, n], cov_history [S, B, n, n] (store_history=True,
                                 else None): the sigma points and their constants that every step emitted, and its moments in
                                 link space
      propagated_history [S, B, K, 6], dt_history [S, B] (fp64) (store_history=True, else None): the rows every step was handed
                                 -- the end of the solve from the points of the step before; at the first step of a run its
                                 initial points -- and the dt it received.  The constants of the propagated points are
                                 ode_history[s - 1]: a solve does not change them.  `smooth()` needs the history."""

    def __init__(self, engine, stats, means, variances, step_index, times, x, ode_p, mean, cov, alive, hist=None, forecast=False):
        st = stats.permute(1, 0, 2)
        self.log_evidence_steps, self.nis = st[..., 0].contiguous(), st[..., 1].contiguous()
        self.n_seen, self.alive = st[..., 2].to(torch.int64), st[..., 3] > 0
        self.mean, self.std = st[..., 4:10].contiguous(), st[..., 10:16].clamp_min(0).sqrt()
        self.step_index, self.times = step_index, times
        self.sigma_points, self.ode_p, self.state_mean, self.state_cov = x, ode_p, mean, cov
        self._engine, self._alive = engine, alive
        self.history, self.ode_history, self.cov_history, self.propagated_history, self.dt_history = \
            hist if hist is not None else (None,) * 5
        self._forecast = forecast
        self.mean_history = means if hist is not None else None
        self.learned = None
        if engine.learn is not None:
            lr = engine.learn
            # coordinate 6 + r holds the constant with the r-th smallest column; `names` keeps the caller's order
            at = torch.as_tensor(6 + np.argsort(np.argsort(lr.columns)), device=means.device)
            self.learned = LearnedParameters(lr.names, lr.link, means.permute(1, 0, 2)[..., at].contiguous(),
                                             variances.permute(1, 0, 2)[..., at].clamp_min(0).sqrt())

    def log_evidence(self):
        """log p(all observations) per patient [B]: -inf for a patient that was lost (with a warning)."""
        total = self.log_evidence_steps.sum(1)
        lost = int(torch.isneginf(total).sum())
        if lost:
            warnings.warn(f"run_ukf: {lost} of {total.numel()} patients were lost (failed solves or non-finite states); their "
                          "log-evidence is -inf")
        return total

    def forecast(self, t_span, external_inputs=None, steps=None):
        """Continue from the final sigma points over `t_span` ([T] or [B, T], its first point the time of the last step) without
        observations: the same loop -- what a run whose trailing rows are NaN computes, bit for bit (the covariance grows by
        the process noise, a walking constant's band widens).  One filter step at the last grid point, or at the ascending
        grid indices `steps`.  Returns a UKFResult."""
        e = self._engine
        t = torch.as_tensor(t_span).to(e.dev, e.dtype)
        T = t.shape[-1]
        if t.dim() not in (1, 2) or T < 2 or (t.dim() == 2 and t.shape[0] != e.B):
            raise ValueError("t_span must be [T] or [B, T] with T >= 2")
        idxs = [T - 1] if steps is None else _check_steps(steps, T)
        last = self.times[..., -1]
        if not torch.equal(t[..., 0].expand_as(last), last):
            raise ValueError("t_span must start at the time of the filter's last step")
        ins = _inputs(external_inputs, e.B, T, e.dev, e.dtype)
        mean, cov, alive = self.state_mean.clone(), self.state_cov.clone(), self._alive.clone()
        x, ode_p, stats, means, variances, hist = e.run(self.sigma_points.clone(), self.ode_p.clone(), mean, cov, alive, t, ins, None,
                                                        None, idxs, False)
        gi = torch.as_tensor(idxs, device=e.dev)
        return UKFResult(e, stats, means, variances, gi, t[..., gi], x, ode_p, mean, cov, alive, hist, forecast=True)

    def smooth(self):
        """The unscented Rauch-Tung-Striebel smoother over this run (store_history=True): the state at every step given the whole
        record, where `mean` / `std` give it given the record up to that step.  Three kernel launches (csrc/hode_ukf_smooth.hip;
        include/hode_ukf_smooth.h), nothing is read back to the host.  Returns a UKFSmoothResult."""
        if self._forecast:
            raise ValueError("smooth() is for the result of run_ukf: a forecast has no observations to look back from")
        if self.history is None:
            raise ValueError("smooth() needs the filter's history: run_ukf(..., store_history=True)")
        e = self._engine
        alive = self.alive.t().to(torch.int32).contiguous()
        out = hode.capi.ukf_smooth(self.history, self.ode_history, self.propagated_history, self.mean_history, self.cov_history, alive,
                                   e.mode, e.q, e.walk, self.dt_history, e.weights, link=e.link)
        return UKFSmoothResult(e, self, *out)


class UKFSmoothResult:
    """The result of `UKFResult.smooth()`, tensors on the compute device; S, n and the coordinates as in the UKFResult it came from.
      mean, std [B, S, 6]        the smoothed moments of the states in natural space: the unscented mean and standard deviation of
                                 the sigma points of (state_mean, state_cov); at a patient's last step the filter's, bit for bit
      state_mean [B, S, n], state_cov [B, S, n, n]   the smoothed moments in link space (fp64)
      gain [B, S-1, n, n]        the smoother gain G_s = C_s (P-_{s+1})^-1 of every pair of steps
      pred_mean [B, S-1, n], pred_cov [B, S-1, n, n]   the predicted moments m-, P- of step s + 1 that G_s was formed with
      alive [B, S], step_index [S], times               carried over; from the step at which a patient was lost everything above is
                                 NaN for it (and the gain into that step), and its last alive step is its terminal one
      learned                    a LearnedParameters (run_ukf(learn=...), else None): per step, the smoothed location and scale of
                                 every learned constant in link space, in the caller's order"""

    def __init__(self, engine, res, mean_s, cov_s, gain, pred_mean, pred_cov, moments):
        mo = moments.permute(1, 0, 2)
        self.mean, self.std = mo[..., :6].contiguous(), mo[..., 6:].clamp_min(0).sqrt()
        self.state_mean, self.state_cov = mean_s.transpose(0, 1).contiguous(), cov_s.transpose(0, 1).contiguous()
        self.gain, self.pred_mean, self.pred_cov = (v.transpose(0, 1).contiguous() for v in (gain, pred_mean, pred_cov))
        self.alive, self.step_index, self.times = res.alive, res.step_index, res.times
        self.learned = None
        if engine.learn is not None:
            lr = engine.learn
            at = torch.as_tensor(6 + np.argsort(np.argsort(lr.columns)), device=mean_s.device)
            self.learned = LearnedParameters(lr.names, lr.link, self.state_mean[..., at].contiguous(),
                                             self.state_cov.diagonal(dim1=2, dim2=3)[..., at].clamp_min(0).sqrt())


def run_ukf(model, data, process_noise=0.05, noise_link="log", noise_sigma=1.0, initial_spread=0.1, learn=None, alpha=1.0, beta=0.0,
            kappa=1.0, steps=None, solver="dopri5", rtol=1e-6, atol=1e-8, dtype=torch.float32, store_history=False):
    """Track every patient of `data` with an unscented Kalman filter.

    data, noise_sigma, process_noise / initial_spread, noise_link, steps, solver: as `run_filter` takes them -- the batch dict
    (initial_state [B, 6], time_points [T] or [B, T], external_inputs, observations [B, T, 6] with NaN = missing, optional
    observation_mask); the observation noise as a scalar, one value per state or an ObservationModel with fixed noise
    ("marginal" is refused); a scalar or one value per state, 0 leaves a state exact; "log" or "additive"; the later grid
    points at which any patient has an observed entry plus the last one, or the ascending grid indices `steps`.
    At the first grid point a patient's moments are the mean g(x0) (minus initial_spread^2 / 2 under the log link, so that the
    natural-space mean is x0) and the covariance diag(initial_spread^2), updated against row 0.
    learn: a ParameterLearning -- its names, link, walk and initial_spread are used: the named constants join the state with the
    mean phi(the model's value), the variance initial_spread^2 and a random walk of `walk` per sqrt(time); each needs
    initial_spread > 0 or walk > 0.  Its `discount` is NOT used: a Kalman filter learns a constant through its cross-covariance
    with the states, and there is no shrinkage.
    alpha, beta, kappa: the scaled unscented transform (hode.capi.ukf_weights); the defaults 1, 0, 1 give all-positive weights,
    so no covariance sum can go indefinite by its weights.  store_history: keep what every step emitted and was handed
    (UKFResult.history, .propagated_history): what `UKFResult.smooth()` works from.
    Returns a UKFResult."""
    from models.hybrid_ode_nn import _compute_device, _method
    if noise_link not in hode.capi.PF_LINK:
        raise ValueError(f"noise_link must be one of {sorted(hode.capi.PF_LINK)}, not {noise_link!r}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be torch.float32 or torch.float64")
    q, q0 = _six_nonneg(process_noise, "process_noise"), _six_nonneg(initial_spread, "initial_spread")
    om = noise_sigma if isinstance(noise_sigma, ObservationModel) else ObservationModel(noise_sigma)
    if om.marginal:
        raise ValueError('run_ukf updates under a fixed observation noise: noise="marginal" is not offered here')
    method = _method(solver)
    x0, t, obs, B, T = _check_data(data)
    if learn is not None and not isinstance(learn, ParameterLearning):
        raise ValueError(f"learn must be a ParameterLearning or None, not {type(learn).__name__}")
    if learn is not None and not np.all((learn.initial_spread > 0) | (learn.walk > 0)):
        raise ValueError("run_ukf: every learned constant needs initial_spread > 0 or walk > 0 (a constant without either has no "
                         "variance to learn with)")
    n = 6 + (len(learn.columns) if learn is not None else 0)
    for name, v in (("alpha", alpha), ("beta", beta), ("kappa", kappa)):
        if not np.isfinite(float(v)):
            raise ValueError(f"{name} must be finite")
    if not float(alpha) ** 2 * (n + float(kappa)) > 0.0:
        raise ValueError(f"alpha = {alpha}, kappa = {kappa}: n + lambda = alpha^2 (n + kappa) must be positive (n = {n})")
    weights = hode.capi.ukf_weights(n, alpha, beta, kappa)
    idxs = None if steps is None else _check_steps(steps, T)
    model._check_supported()

    dev = _compute_device()
    om.prepare(obs, data.get("observation_mask"), device=dev, dtype=dtype)
    obs_d = om.obs.view(B, T, 6)
    mask_d = None if om.mask is None else om.mask.view(B, T, 6)
    if idxs is None:
        idxs = _default_steps(obs_d, mask_d)                            # the one read-back, before the loop
    t = t.to(dev, dtype)
    ins = _inputs(data.get("external_inputs"), B, T, dev, dtype)
    link = hode.capi.PF_LINK[noise_link]
    eng = _Engine(model, B, q, om.sigma, link, learn, weights, method, rtol, atol, dtype, dev, bool(store_history))
    K = eng.K
    with torch.no_grad():
        _, ode_vec = model._params_on(dev)
        ode_p = ode_vec.detach().to(dtype).reshape(1, 1, 17).repeat(B, K, 1).contiguous()
        x = x0.to(dev, dtype).reshape(B, 1, 6).repeat(1, K, 1).contiguous()
        f64 = dict(dtype=torch.float64, device=dev)
        s0 = torch.as_tensor(q0, **f64)
        m_x = x[:, 0].double()
        m_x = m_x.log() - 0.5 * s0 * s0 if link == hode.capi.PF_LINK["log"] else m_x
        var = [s0 * s0]
        mean = [m_x]
        if learn is not None:
            order = np.argsort(learn.columns)                            # the kernel's coordinates: ascending column order
            theta = ode_p[:, 0, sorted(learn.columns)].double()
            mean.append(theta.log() if learn.link == "log" else theta)
            var.append(torch.as_tensor(learn.initial_spread[order], **f64) ** 2)
        mean = torch.cat(mean, 1).contiguous()
        cov = torch.diag_embed(torch.cat(var).expand(B, n)).contiguous()
        alive = torch.ones(B, dtype=torch.int32, device=dev)
    x, ode_p, stats, means, variances, hist = eng.run(x, ode_p, mean, cov, alive, t, ins, obs_d, mask_d, idxs, True)
    gi = torch.as_tensor([0] + idxs, device=dev)
    return UKFResult(eng, stats, means, variances, gi, t[..., gi], x, ode_p, mean, cov, alive, hist)
