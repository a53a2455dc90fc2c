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
    fit_ukf_noise  the noise the filter is told -- process_noise, noise_sigma, the walk of the learned constants -- fitted to
                 the record by EM over the smoother (csrc/hode_ukf_em.hip): a UKFNoiseFit.

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

__all__ = ["UKFNoiseFit", "UKFResult", "UKFSmoothResult", "fit_ukf_noise", "run_ukf"]


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
        return UKFSmoothResult(self._engine, self, *self._smooth_raw())

    def _smooth_raw(self):
        """The smoother's six outputs as the kernels leave them, step-major."""
        e = self._engine
        alive = self.alive.t().to(torch.int32).contiguous()
        return hode.capi.ukf_smooth(self.history, self.ode_history, self.propagated_history, self.mean_history, self.cov_history, alive,
                                    e.mode, e.q, e.walk, self.dt_history, e.weights, link=e.link)


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
        self._engine, self._res, self._moments = engine, res, moments
        self.learned = None
        if engine.learn is not None:
            lr = engine.learn
            at = torch.as_tensor(6 + np.argsort(np.argsort(lr.columns)), device=mean_s.device)
            self.learned = LearnedParameters(lr.names, lr.link, self.state_mean[..., at].contiguous(),
                                             self.state_cov.diagonal(dim1=2, dim2=3)[..., at].clamp_min(0).sqrt())

    def noise_statistics(self, data):
        """One E-step of `fit_ukf_noise` over this smoothed run, without an update (csrc/hode_ukf_em.hip; include/hode_ukf_em.h;
        DESIGN.md section 4.24).  data: the batch dict the run was made from (its grid, inputs and observations are read).
        Returns a dict of device tensors, step-major: e2 [S-1, B, n] the expected squared residual of every coordinate over every
        pair of steps (NaN for a pair that does not count) and pair_ok [S-1, B]; r2 [S, B, 6] that of every seen observation
        (0 for an unseen one) and seen [S, B] (bit j: state j); sums [37] (hode.capi.UKF_EM_SUM_AT: A per coordinate, N, D, R, M);
        and the E-step's rows x_em, aux_em, chol, prop_em, status."""
        e, res = self._engine, self._res
        x0, t, obs, B, T = _check_data(data)
        if B != e.B:
            raise ValueError(f"noise_statistics: data holds {B} patients, the run {e.B}")
        om = ObservationModel(1.0)
        om.prepare(obs, data.get("observation_mask"), device=e.dev, dtype=e.dtype)
        gi = self.step_index.tolist()
        if gi[-1] > T - 1:
            raise ValueError("noise_statistics: the run's steps lie outside the data's grid")
        ctx = dict(t=t.to(e.dev, e.dtype), ins=_inputs(data.get("external_inputs"), B, T, e.dev, e.dtype), obs=om.obs.view(B, T, 6),
                   mask=None if om.mask is None else om.mask.view(B, T, 6), idxs=gi[1:])
        plan = _EStep(e, ctx)
        raw = (self.state_mean.transpose(0, 1).contiguous(), self.state_cov.transpose(0, 1).contiguous(),
               self.gain.transpose(0, 1).contiguous(), None, None, self._moments)
        out = plan.run(res, raw)
        q, walk, sigma = e.q.clone(), e.walk.clone(), e.sigma.clone()
        out["sums"] = hode.capi.ukf_em_mstep(out["e2"], out["pair_ok"], out["r2"], out["seen"], res.dt_history, q, walk, sigma, e.mode,
                                             [0] * hode.capi.UKF_EM_FIT, [0.0] * hode.capi.UKF_EM_FIT, link=e.link)
        return out


class _EStep:
    """The E-step of the noise fit on one engine and one record: what does not change between iterations -- the grid rows and the
    inputs of every pair's segment, all pairs whose segments have the same number of grid points stacked into ONE forward solve --
    and the launches of one iteration."""

    def __init__(self, eng, ctx):
        self.eng = eng
        t, ins, B, K = ctx["t"], ctx["ins"], eng.B, eng.K
        gi = [0] + list(ctx["idxs"])
        self.S = len(gi)
        at = torch.as_tensor(gi, device=eng.dev)
        self.obs = ctx["obs"][:, at].contiguous()
        self.mask = None if ctx["mask"] is None else ctx["mask"][:, at].contiguous()
        by_len = {}
        for s in range(self.S - 1):
            by_len.setdefault(gi[s + 1] - gi[s] + 1, []).append(s)
        self.groups = []
        for n_pts, pairs in sorted(by_len.items()):
            self.groups.append((None if len(pairs) == self.S - 1 else torch.as_tensor(pairs, device=eng.dev), len(pairs),
                                *self.rows(t, ins, [gi[s] for s in pairs], n_pts)))

    def rows(self, t, ins, starts, n_pts):
        """(t, meal, tVNS, GD) of one solve of the pairs whose segments start at the grid indices `starts` and hold n_pts points:
        per trajectory, [pairs * B * K, n_pts] (a constant input [pairs * B * K])."""
        B, K, P = self.eng.B, self.eng.K, len(starts)
        at = torch.as_tensor(starts, device=t.device)[:, None] + torch.arange(n_pts, device=t.device)[None]            # [P, n_pts]
        grid = lambda v: v[:, at].permute(1, 0, 2).repeat_interleave(K, 1).reshape(P * B * K, n_pts).contiguous()      # noqa: E731
        t_rows = grid(t if t.dim() == 2 else t.expand(B, -1))
        cut = lambda v: None if v is None else (grid(v) if v.dim() == 2 else v.repeat_interleave(K, 0).repeat(P))      # noqa: E731
        return t_rows, cut(ins["meal"]), cut(ins["tVNS"]), cut(ins["GD"])

    def solve(self, x_em, aux_em):
        """prop_em [S-1, B*K, 6] and status [S-1, B*K]: the end of the solve of every pair's rows over its segment."""
        e = self.eng
        prop, status = torch.empty_like(x_em), torch.empty(x_em.shape[:2], dtype=torch.int32, device=e.dev)
        nn_flat, _ = e.model._params_on(e.dev)
        nn_flat = nn_flat.detach().to(e.dtype).contiguous()
        for pairs, P, t_rows, meal, tvns, gd in self.groups:
            rows = P * e.B * e.K
            x, aux = (x_em, aux_em) if pairs is None else (x_em[pairs], aux_em[pairs])
            sol = hode.solve_fwd(x.reshape(rows, 6), t_rows, meal, tvns, gd, aux.reshape(-1), nn_flat, e.H, e.L, method=e.method, rtol=e.rtol,
                                 atol=e.atol, n_sets=rows, nn_shared=True)
            y, st = sol.y[:, -1].reshape(P, e.B * e.K, 6), sol.status.view(P, e.B * e.K)
            if pairs is None:
                prop.copy_(y)
                status.copy_(st)
            else:
                prop[pairs], status[pairs] = y, st
        return prop, status

    def run(self, res, raw):
        """One E-step over the stored run `res` and its smoother's raw outputs: points, the grouped solves, stats."""
        e = self.eng
        mean_s, cov_s, gain, _, _, moments = raw
        with torch.no_grad():
            alive = res.alive.t().to(torch.int32).contiguous()
            x_em, aux_em, chol = hode.capi.ukf_em_points(mean_s, cov_s, alive, res.ode_history, e.mode, e.weights, link=e.link)
            prop, status = self.solve(x_em, aux_em)
            e2, pair_ok, r2, seen = hode.capi.ukf_em_stats(prop, status, chol, mean_s, cov_s, gain, alive, self.obs, self.mask, moments, e.mode,
                                                           e.weights, link=e.link)
        return dict(e2=e2, pair_ok=pair_ok, r2=r2, seen=seen, x_em=x_em, aux_em=aux_em, chol=chol, prop_em=prop, status=status)


def _host_checks(model, data, process_noise, noise_link, noise_sigma, initial_spread, learn, alpha, beta, kappa, steps, solver, dtype,
                 who="run_ukf"):
    """Everything run_ukf validates before a device is touched; the checked values as a dict."""
    from models.hybrid_ode_nn import _method
    if noise_link not in hode.capi.PF_LINK:
        raise ValueError(f"noise_link must be one of {sorted(hode.capi.PF_LINK)}, not {noise_link!r}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be torch.float32 or torch.float64")
    q, q0 = _six_nonneg(process_noise, "process_noise"), _six_nonneg(initial_spread, "initial_spread")
    om = noise_sigma if isinstance(noise_sigma, ObservationModel) else ObservationModel(noise_sigma)
    if om.marginal:
        raise ValueError(f'{who} updates under a fixed observation noise: noise="marginal" is not offered here')
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
    return dict(q=q, q0=q0, om=om, method=method, x0=x0, t=t, obs=obs, B=B, T=T, n=n, weights=weights, idxs=idxs)


def _open(model, data, h, noise_link, learn, rtol, atol, dtype, store):
    """The engine and what its runs read, on the device: (engine, context)."""
    from models.hybrid_ode_nn import _compute_device
    q, om, method, x0, t, obs, B, T, weights, idxs = (h[k] for k in ("q", "om", "method", "x0", "t", "obs", "B", "T", "weights", "idxs"))
    dev = _compute_device()
    om.prepare(obs, data.get("observation_mask"), device=dev, dtype=dtype)
    obs_d = om.obs.view(B, T, 6)
    mask_d = None if om.mask is None else om.mask.view(B, T, 6)
    if idxs is None:
        idxs = _default_steps(obs_d, mask_d)                            # the one read-back, before the loop
    t = t.to(dev, dtype)
    ins = _inputs(data.get("external_inputs"), B, T, dev, dtype)
    link = hode.capi.PF_LINK[noise_link]
    eng = _Engine(model, B, q, om.sigma, link, learn, weights, method, rtol, atol, dtype, dev, store)
    return eng, dict(x0=x0, t=t, ins=ins, obs=obs_d, mask=mask_d, idxs=idxs, q0=h["q0"], n=h["n"])


def _filter(eng, ctx):
    """One run of the filter over the record from the engine's current q, sigma and walk.  Returns a UKFResult."""
    x0, t, ins, obs_d, mask_d, idxs, q0, n = (ctx[k] for k in ("x0", "t", "ins", "obs", "mask", "idxs", "q0", "n"))
    model, B, dev, dtype, link, learn = eng.model, eng.B, eng.dev, eng.dtype, eng.link, eng.learn
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
    h = _host_checks(model, data, process_noise, noise_link, noise_sigma, initial_spread, learn, alpha, beta, kappa, steps, solver, dtype)
    eng, ctx = _open(model, data, h, noise_link, learn, rtol, atol, dtype, bool(store_history))
    return _filter(eng, ctx)


class UKFNoiseFit:
    """The result of `fit_ukf_noise`.  I = the EM iterations made (n_iter, or fewer with `tol`).
      process_noise [6], noise_sigma [6]   the fitted values (numpy fp64); walk: the fitted walk of every learned constant in
                                 the caller's order (None without `learn`)
      trace                      a dict of numpy arrays process_noise [I+1, 6], noise_sigma [I+1, 6], walk [I+1, names]: the
                                 values before every iteration and the final ones
      log_evidence [I+1]         the filter's log-evidence summed over the patients alive at its end, at every row of `trace`
      sums [I, 37]               the statistics every iteration's update was made from (hode.capi.UKF_EM_SUM_AT)
      pairs_used                 the number of (patient, pair of steps) the last iteration counted
      result, smoothed           the UKFResult (store_history=True) and its UKFSmoothResult at the fitted values"""

    def __init__(self, trace, log_evidence, sums, result, smoothed):
        self.trace, self.log_evidence, self.sums, self.result, self.smoothed = trace, log_evidence, sums, result, smoothed
        self.process_noise, self.noise_sigma = trace["process_noise"][-1].copy(), trace["noise_sigma"][-1].copy()
        self.walk = None if trace["walk"] is None else trace["walk"][-1].copy()
        self.pairs_used = int(sums[-1][hode.capi.UKF_EM_SUM_AT["N"]])


_FIT_NAMES = ("process_noise", "noise_sigma", "walk")


def _fit_mask(fit, learn):
    """The 29 host flags of the M-step (q [6], walk [17] by column, sigma [6]) from `fit`: names, or a dict name -> a flag or one
    flag per entry (per state; for "walk" per learned name, in the caller's order)."""
    if isinstance(fit, str):
        fit = (fit,)
    chosen = dict(fit) if isinstance(fit, dict) else {name: True for name in fit}
    for name in chosen:
        if name not in _FIT_NAMES:
            raise ValueError(f"fit names {_FIT_NAMES}, not {name!r}")
    if "walk" in chosen and learn is None:
        raise ValueError('fit: "walk" needs learn=ParameterLearning(...)')
    mask = np.zeros(hode.capi.UKF_EM_FIT, dtype=np.int32)
    for name, flags in chosen.items():
        size = len(learn.columns) if name == "walk" else 6
        flags = np.asarray(flags, dtype=bool).reshape(-1)
        if flags.size == 1:
            flags = np.repeat(flags, size)
        if flags.size != size:
            raise ValueError(f"fit[{name!r}] must be one flag or {size}")
        if name == "walk":
            mask[6 + np.asarray(learn.columns)] = flags
        else:
            at = 0 if name == "process_noise" else 6 + 17
            mask[at:at + 6] = flags
    if not mask.any():
        raise ValueError("fit selects nothing")
    return mask


def fit_ukf_noise(model, data, process_noise=0.05, noise_sigma=1.0, learn=None, fit=("process_noise", "noise_sigma"), n_iter=10, tol=None,
                  floor=1e-6, noise_link="log", initial_spread=0.1, alpha=1.0, beta=0.0, kappa=1.0, steps=None, solver="dopri5", rtol=1e-6,
                  atol=1e-8, dtype=torch.float32):
    """Fit the noise `run_ukf` is told -- process_noise, noise_sigma and the walk of the learned constants -- to the record by
    expectation-maximisation over the smoother (csrc/hode_ukf_em.hip; include/hode_ukf_em.h).

    process_noise, noise_sigma, learn (its walk): the values to start from; everything else as `run_ukf` takes it.
    fit: the names to fit among "process_noise", "noise_sigma", "walk", or a dict name -> a flag or one flag per state (for
    "walk" per learned name).  A value that is exactly 0 stays 0 (an exact state stays exact), as does one nothing was counted
    for.  floor: a fitted value is not taken below it (a scalar or 29 values: q, walk by column, sigma).
    One iteration is a filter with its history, the smoother, the sigma points of every smoothed step, ONE forward solve per
    segment length over all pairs of steps, the statistics, and the update of the engine's q, sigma, walk on the device.  With
    tol=None nothing is read back until the end; with tol the summed evidence is read once per iteration and the fit stops when
    it rises by less than tol.  Returns a UKFNoiseFit."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("n_iter must be at least 1")
    if tol is not None and not float(tol) >= 0.0:
        raise ValueError("tol must be None or non-negative")
    if learn is not None and not isinstance(learn, ParameterLearning):
        raise ValueError(f"learn must be a ParameterLearning or None, not {type(learn).__name__}")
    fit_mask = _fit_mask(fit, learn)
    floors = np.asarray(floor, dtype=np.float64).reshape(-1)
    floors = np.repeat(floors, hode.capi.UKF_EM_FIT) if floors.size == 1 else floors
    if floors.size != hode.capi.UKF_EM_FIT or not np.all(np.isfinite(floors)) or not np.all(floors >= 0):
        raise ValueError(f"floor must be non-negative: a scalar or {hode.capi.UKF_EM_FIT} values")
    h = _host_checks(model, data, process_noise, noise_link, noise_sigma, initial_spread, learn, alpha, beta, kappa, steps, solver, dtype,
                     who="fit_ukf_noise")
    eng, ctx = _open(model, data, h, noise_link, learn, rtol, atol, dtype, True)
    gi = torch.as_tensor([0] + ctx["idxs"], device=eng.dev)
    if not bool((ctx["t"].double()[..., gi].diff(dim=-1) > 0).all()):         # (before the loop, like the default steps)
        raise ValueError("fit_ukf_noise: the time points of the filter steps must ascend")
    plan = _EStep(eng, ctx)
    names = None if learn is None else torch.as_tensor(np.asarray(learn.columns), device=eng.dev)

    def values():
        return (eng.q.clone(), eng.sigma.clone(), None if names is None else eng.walk[names])

    def evidence(res):
        total = res.log_evidence_steps.sum(1)
        return torch.where(res.alive[:, -1], total, torch.zeros_like(total)).sum()

    trace, ev, sums = [], [], []
    for it in range(n_iter):
        res = _filter(eng, ctx)
        trace.append(values())
        ev.append(evidence(res))
        raw = res._smooth_raw()
        if tol is not None and it > 0 and float(ev[-1] - ev[-2]) < float(tol):
            break
        st = plan.run(res, raw)
        sums.append(hode.capi.ukf_em_mstep(st["e2"], st["pair_ok"], st["r2"], st["seen"], res.dt_history, eng.q, eng.walk, eng.sigma,
                                           eng.mode, fit_mask, floors, link=eng.link, check_dt=False))
    else:
        res = _filter(eng, ctx)
        trace.append(values())
        ev.append(evidence(res))
        raw = res._smooth_raw()
    host = lambda v: v.cpu().numpy()                                                                                     # noqa: E731
    out = {"process_noise": np.stack([host(v[0]) for v in trace]), "noise_sigma": np.stack([host(v[1]) for v in trace]),
           "walk": None if names is None else np.stack([host(v[2]) for v in trace])}
    return UKFNoiseFit(out, host(torch.stack(ev)), host(torch.stack(sums)), res, UKFSmoothResult(eng, res, *raw))
