"""A bootstrap particle filter on the GPU: online state tracking, forecasts from the current state and the marginal likelihood
of a model with process noise (csrc/hode_filter.hip; include/hode.h, "Particle filter").

    run_filter      N particles per patient, carried from filter step to filter step by ONE forward solve of the B * N
                    trajectories over that segment of the grid (the network shared, every particle's 17 mechanistic constants
                    in its own row) and ONE launch of the step kernel: process noise, weights under the observation model,
                    normalisation, ESS, systematic resampling, the gather.  Nothing is read back to the host inside the loop.
    FilterResult    the filtered moments, ESS, log-evidence increments, the final particles; `forecast` continues the same loop
                    without observations; with store_particles=True the history, the ancestors, `smoothed()` (genealogy
                    tracing) and `smooth()`: backward-simulation smoothing, ONE launch of csrc/hode_smooth.hip over the stored
                    steps (include/hode.h, "Particle smoother") -> SmoothResult.
    ParameterLearning  run_filter(learn=...): chosen mechanistic constants are learned online.  After every step ONE launch of
                    csrc/hode_pf_params.hip moves those columns of the particles' rows (Liu & West's kernel shrinkage for a
                    discount, and / or a random walk for constants that drift); the next segment solve reads the moved rows
                    (include/hode.h, "Particle filter: parameter move") -> FilterResult.learned.

The state model: between two filter steps a particle follows the deterministic solve; at a step it is disturbed by noise of
standard deviation process_noise * sqrt(time since the previous step) -- additive, or on the logarithm (the default: states stay
positive and the noise is relative; the -s^2 / 2 drift keeps the mean).  The variance accumulated over a stretch of time is
therefore the same for any choice of steps."""
import statistics
import warnings

import numpy as np
import torch

import hode
from models.ode_core import ODE_PARAM_NAMES

from .observation import ObservationModel

__all__ = ["FilterResult", "LearnedParameters", "ParameterLearning", "SmoothResult", "run_filter"]

MAX_PARTICLES = hode.capi.PF_MAX_PARTICLES
SPREAD_STEP = 0xFFFFFFFF          # the step number that keys the draws of ParameterLearning.initial_spread ("the step before 0")


def _six_nonneg(v, what):
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 6)
    if a.size != 6 or not np.all(np.isfinite(a)) or not np.all(a >= 0):
        raise ValueError(f"{what} must be non-negative: a scalar or one value per state")
    return a


def _check_steps(steps, T):
    idx = [int(s) for s in steps]
    if not idx or idx[0] < 1 or idx[-1] > T - 1 or any(b <= a for a, b in zip(idx, idx[1:])):
        raise ValueError(f"steps must be ascending grid indices in 1..{T - 1}")
    return idx


def _ode_column(name):
    key = name[4:] if isinstance(name, str) and name.startswith("ode_") else name
    if key not in ODE_PARAM_NAMES:
        raise ValueError(f"unknown mechanistic constant {name!r}; known: {list(ODE_PARAM_NAMES)}")
    return ODE_PARAM_NAMES.index(key)


class ParameterLearning:
    """What `run_filter(learn=...)` learns online, and how the cloud of each constant is moved after every filter step.
      names            mechanistic constants (with or without the `ode_` prefix, as `ode_sets` takes them)
      discount         Liu & West's delta in (1/3, 1]: after a step the values are shrunk towards their weighted mean by
                       a = (3 delta - 1) / (2 delta) and given back the variance that takes away, (1 - a^2) V, as noise --
                       mean and variance of the cloud are kept, the copies a resampling makes become distinct.  1: no shrinkage.
      walk             a scalar or one value per name: the standard deviation per sqrt(time) of a random walk in link space,
                       for constants that drift (and what widens a forecast); 0: none.
      initial_spread   the same shape: the standard deviation in link space by which the particles, which all start at the
                       model's value (or at their `ode_sets` row), are spread at the first grid point; 0: none.
      link             "log" (the default: a constant stays positive, spreads are relative) or "identity".
    Everything is validated here, before a device is touched."""
    LINKS = ("log", "identity")

    def __init__(self, names, discount=0.98, walk=0.0, initial_spread=0.0, link="log"):
        names = [names] if isinstance(names, str) else list(names)
        if not names:
            raise ValueError("ParameterLearning needs at least one constant in names")
        self.columns = [_ode_column(n) for n in names]
        if len(set(self.columns)) != len(self.columns):
            raise ValueError(f"ParameterLearning: names holds a constant twice: {names}")
        self.names = [ODE_PARAM_NAMES[j] for j in self.columns]
        if link not in self.LINKS:
            raise ValueError(f"link must be one of {list(self.LINKS)}, not {link!r}")
        self.link = link
        self.discount = float(discount)
        if not 1.0 / 3.0 < self.discount <= 1.0:
            raise ValueError("discount must lie in (1/3, 1]")
        self.walk, self.initial_spread = self._per_name(walk, "walk"), self._per_name(initial_spread, "initial_spread")

    def _per_name(self, v, what):
        a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
        if a.size == 1:
            a = np.repeat(a, len(self.names))
        if a.size != len(self.names) or not np.all(np.isfinite(a)) or not np.all(a >= 0):
            raise ValueError(f"{what} must be non-negative: a scalar or one value per name")
        return a

    @property
    def shrink(self):
        """Liu & West's a = (3 delta - 1) / (2 delta)."""
        return (3.0 * self.discount - 1.0) / (2.0 * self.discount)

    def _full(self, v):
        out = np.zeros(17)
        out[self.columns] = v
        return out


class LearnedParameters:
    """`FilterResult.learned`: the cloud of every learned constant at every filter step, in link space (phi = the constant or,
    under the log link, its logarithm), tensors on the compute device.
      names, link
      location, scale [B, S, P]  the weighted mean and standard deviation of phi over the particles after step s's weight update
                                 and gather, before step s's shrinkage and walk (at the first grid point: after the initial
                                 spread); NaN for a patient without a particle alive."""

    def __init__(self, names, link, location, scale):
        self.names, self.link, self.location, self.scale = list(names), link, location, scale

    def _inverse(self, phi):
        return phi.exp() if self.link == "log" else phi

    def median(self):
        """[B, S, P]: the constant at the centre of the cloud, g^-1(location)."""
        return self._inverse(self.location)

    def interval(self, level=0.9):
        """(lower, upper) [B, S, P]: g^-1(location -+ z scale), z the normal quantile of the central `level`."""
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie in (0, 1)")
        z = statistics.NormalDist().inv_cdf(0.5 + 0.5 * float(level))
        return self._inverse(self.location - z * self.scale), self._inverse(self.location + z * self.scale)


class _Engine:
    """What one run and its forecasts share: the network and the settings on the device, and the loop."""

    def __init__(self, model, B, N, q, sigma, link, ess, seed, method, rtol, atol, dtype, dev, store, ode_sets=False, learn=None):
        nl = model.nn_residual
        self.model, self.B, self.N, self.dtype, self.dev, self.store = model, B, N, dtype, dev, store
        self.ode_sets = ode_sets                                # particles with their own mechanistic constants
        self.H, self.L, self.method, self.rtol, self.atol = nl.hidden_dim, nl.hip_layers, method, float(rtol), float(atol)
        self.link, self.ess, self.seed = link, float(ess), int(seed)
        f64 = dict(dtype=torch.float64, device=dev)
        self.q, self.sigma = torch.as_tensor(q, **f64), torch.as_tensor(sigma, **f64)
        self.learn = learn                                      # a ParameterLearning: the parameter move after every step
        if learn is not None:
            mode = np.zeros(17, dtype=np.int32)
            mode[learn.columns] = hode.capi.PF_MOVE[learn.link]
            self.mode = torch.as_tensor(mode, device=dev)
            self.walk = torch.as_tensor(learn._full(learn.walk), **f64)
            self.spread = torch.as_tensor(learn._full(learn.initial_spread), **f64)

    def run(self, x, lw, ode_p, t, ins, obs, mask, idxs, counter, init_q=None, observed=None):
        """Carry (x [B, N, 6], lw [B, N], ode_p [B, N, 17]) over the grid t ([T] or [B, T]) with a filter step at every index of
        `idxs` (and, with init_q, one at index 0 that spreads the particles by init_q); obs [B, T, 6] / mask uint8 [B, T, 6] or
        None (no observations).  `counter`: the step number of the first step taken.  `observed` (a learning run): per grid
        index, whether any patient has an observed entry there (None: nobody ever).  Returns the per-step outputs; the last
        two are (pstats [S, B, 34] of the parameter move, ode_history), each None where it does not apply, and what `smooth()`
        needs on top of the history (store_particles=True, else None): (predicted [S, B, N, 6], the x_in row of every step with
        NaN where the solve failed; log_weight_history [S, B, N]; step_dt [S, B])."""
        B, N, dev, dtype = self.B, self.N, self.dev, self.dtype
        with torch.no_grad():
            nn_flat, _ = self.model._params_on(dev)
            nn_flat = nn_flat.detach().to(dtype).contiguous()
            S = len(idxs) + (init_q is not None)
            stats = torch.empty(S, B, hode.capi.PF_COLS, dtype=torch.float64, device=dev)
            pstats = torch.empty(S, B, 34, dtype=torch.float64, device=dev) if self.learn is not None else None
            odeh = torch.empty(S, B, N, 17, dtype=dtype, device=dev) if self.learn is not None and self.store else None
            hist = torch.empty(S, B, N, 6, dtype=dtype, device=dev) if self.store else None
            ancs = torch.empty(S, B, N, dtype=torch.int32, device=dev) if self.store else None
            kept = (torch.empty(S, B, N, 6, dtype=dtype, device=dev), torch.empty(S, B, N, dtype=torch.float64, device=dev),
                    torch.empty(S, B, dtype=torch.float64, device=dev)) if self.store else None
            bufs = [torch.empty_like(x), torch.empty_like(x)]
            anc1 = torch.empty(B, N, dtype=torch.int32, device=dev)
            aux = [ode_p, torch.empty_like(ode_p)]
            nan_row = torch.full((B, 6), float("nan"), dtype=dtype, device=dev)
            per_patient = t.dim() == 2
            # the inputs per particle: a grid input [B, T] -> [B * N, T] once, sliced per segment; a constant [B] -> [B * N]
            rep = {k: (None if v is None else v.repeat_interleave(N, 0)) for k, v in ins.items()}
            t_rep = t.repeat_interleave(N, 0) if per_patient else t
            t64 = t.double()                                    # the step's dt: the exact difference of the grid's values
            s = 0

            def step(x_in, status, g, dt, q, init=False):
                nonlocal s, x
                out = (hist[s] if self.store else bufs[s & 1], ancs[s] if self.store else anc1, stats[s], aux[1])
                ob = nan_row if obs is None else obs[:, g].contiguous()
                mk = None if mask is None else mask[:, g].contiguous()
                hode.capi.pf_step(x_in, ob, self.sigma, q, dt, lw, counter + s, seed=self.seed, id0=0, link=self.link, ess_frac=self.ess,
                                  status=status, mask=mk, aux_in=aux[0], out=out)
                if self.store:                                  # copies only: what the step kernel was given does not change
                    kept[0][s].copy_(x_in if status is None else torch.where((status != 0).unsqueeze(-1), nan_row[0, 0], x_in))
                    kept[1][s].copy_(lw)
                    kept[2][s].copy_(dt)
                if self.learn is not None:
                    # the move, on the rows the step gathered; the next segment solve reads them.  Shrinking needs data to shrink
                    # towards: a step at which nobody observed anything only walks (so a forecast equals trailing NaN rows)
                    if init and bool(self.learn.initial_spread.any()):  # the first grid point: spread the cloud, draws of its own
                        hode.capi.pf_params(lw, out[3], self.mode, self.spread, dt, SPREAD_STEP, 1.0, seed=self.seed, id0=0, out=pstats[s])
                    a = self.learn.shrink if (observed is not None and observed[g]) else 1.0
                    hode.capi.pf_params(lw, out[3], self.mode, self.walk, dt, counter + s, a, seed=self.seed, id0=0, out=pstats[s])
                    if self.store:
                        odeh[s].copy_(out[3])
                x = out[0]
                aux.reverse()
                s += 1

            if init_q is not None:
                step(x, None, 0, torch.ones(B, dtype=torch.float64, device=dev), torch.as_tensor(init_q, dtype=torch.float64, device=dev),
                     init=True)
            prev = 0
            for g in idxs:
                seg = slice(prev, g + 1)
                cut = lambda v: None if v is None else (v[:, seg].contiguous() if v.dim() == 2 else v)          # noqa: E731
                sol = hode.solve_fwd(x.reshape(B * N, 6), t_rep[:, seg].contiguous() if per_patient else t[seg].contiguous(),
                                     cut(rep["meal"]), cut(rep["tVNS"]), cut(rep["GD"]), aux[0].reshape(-1), nn_flat, self.H, self.L,
                                     method=self.method, rtol=self.rtol, atol=self.atol, n_sets=B * N, nn_shared=True)
                dt = (t64[:, g] - t64[:, prev] if per_patient else (t64[g] - t64[prev]).expand(B)).contiguous()
                step(sol.y[:, -1].reshape(B, N, 6).contiguous(), sol.status.view(B, N), g, dt, self.q)
                prev = g
            x = x.clone() if self.store else x
        return x, lw, aux[0], stats, hist, ancs, (pstats, odeh), kept


class FilterResult:
    """The result of `run_filter` / `forecast`, tensors on the compute device.  S = the filter steps taken, the weighting of the
    initial particles at the first grid point included (a forecast has no such step).
      mean, std [B, S, 6]        the filtered moments: weighted over the particles, after the step's weight update
      ess [B, S], resampled [B, S] (bool), alive [B, S] (int64)
      log_evidence_steps [B, S]  log p(obs at step s | obs before it); `log_evidence()` is their sum
      step_index [S]             the grid index of every step;  times [S] or [B, S]
      particles [B, N, 6], log_weights [B, N] (fp64, unnormalised; 0 after a resampling), ode_p [B, N, 17]: the final particles
      learned                    a LearnedParameters (run_filter(learn=...), else None): the cloud of every learned constant per
                                 step; the final cloud itself is in ode_p
      ode_history [S, B, N, 17]  (learn with store_particles=True) every particle's constants after each step's gather and move:
                                 what the segment solve to the next step read
      history [S, B, N, 6], ancestors [S, B, N] (store_particles=True): the particles after each step's gather, and the slot of
                                 the step before that each one came from;
      predicted [S, B, N, 6], log_weight_history [S, B, N] (fp64), step_dt [S, B] (fp64) (store_particles=True): the state every
                                 slot of the step before was carried to by the segment solve, before the noise (step 0: x0
                                 repeated; NaN where the solve failed), the log-weights as each step left them, and each
                                 step's dt: what `smooth()` reads."""

    def __init__(self, engine, stats, step_index, times, particles, log_weights, ode_p, history, ancestors, counter, kept=None,
                 forecast=False, pstats=None):
        st = stats.permute(1, 0, 2)
        self.log_evidence_steps, self.ess = st[..., 0].contiguous(), st[..., 1].contiguous()
        self.resampled, self.alive = st[..., 2] > 0, st[..., 3].to(torch.int64)
        self.mean, self.std = st[..., 4:10].contiguous(), st[..., 10:16].clamp_min(0).sqrt()
        self.step_index, self.times = step_index, times
        self.particles, self.log_weights, self.ode_p = particles, log_weights, ode_p
        self.history, self.ancestors = history, ancestors
        self.predicted, self.log_weight_history, self.step_dt = kept if kept is not None else (None, None, None)
        self._engine, self._counter, self._forecast = engine, counter, forecast
        self.learned = self.ode_history = None
        pstats, self.ode_history = pstats if pstats is not None else (None, None)
        if pstats is not None:
            lr = engine.learn
            ps = pstats.permute(1, 0, 2)                                # [B, S, 34]
            cols = torch.as_tensor(lr.columns, device=pstats.device)
            self.learned = LearnedParameters(lr.names, lr.link, ps[..., 2 * cols].contiguous(), ps[..., 2 * cols + 1].clamp_min(0).sqrt())

    def log_evidence(self):
        """log p(all observations) per patient [B]: -inf for a patient whose particles all died (with a warning)."""
        total = self.log_evidence_steps.sum(1)
        dead = int(torch.isneginf(total).sum())
        if dead:
            warnings.warn(f"run_filter: every particle of {dead} of {total.numel()} patients died (failed solves or non-finite "
                          "states); their log-evidence is -inf")
        return total

    def weights(self):
        """The normalised weights of the final particles [B, N] (NaN for a patient without a particle alive)."""
        return torch.softmax(self.log_weights, dim=1)

    def smoothed(self):
        """(mean, std) [B, S, 6] of the surviving lineages: the ancestor indices traced back from the last step (torch gathers),
        every lineage with its final weight.  Needs store_particles=True.  The usual caveat of genealogy smoothing applies: far
        back from the last step few distinct ancestors are left, and the early `std` then describes that collapse, not the
        posterior.  `smooth()` draws backward trajectories over ALL particles of every step instead; this method remains for
        runs with `ode_sets`, which `smooth()` does not take."""
        if self.history is None:
            raise ValueError("smoothed() needs run_filter(..., store_particles=True)")
        S, B, N, _ = self.history.shape
        w = self.weights().unsqueeze(-1)
        idx = torch.arange(N, device=self.history.device).expand(B, N)
        mean, std = [], []
        for s in range(S - 1, -1, -1):
            xs = self.history[s].double().gather(1, idx.unsqueeze(-1).expand(B, N, 6))
            m = (w * xs).sum(1)
            mean.append(m)
            std.append((w * (xs - m.unsqueeze(1)) ** 2).sum(1).sqrt())
            idx = self.ancestors[s].long().gather(1, idx)
        return torch.stack(mean[::-1], 1), torch.stack(std[::-1], 1)

    def forecast(self, t_span, external_inputs=None, steps=None):
        """Continue from the final particles over `t_span` ([T] or [B, T], its first point the time of the last step) without
        observations: the same loop, the step counter continued -- what a run whose trailing rows are NaN computes (a learning
        run goes on walking its constants, so the bands of a drifting constant widen, and shrinks nothing).  One filter
        step at the last grid point, or at the ascending grid indices `steps`.  Returns a FilterResult."""
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
        x, lw, ode_p, stats, hist, ancs, pstats, kept = e.run(self.particles, self.log_weights.clone(), self.ode_p.clone(), t, ins, None,
                                                              None, idxs, self._counter)
        gi = torch.as_tensor(idxs, device=e.dev)
        return FilterResult(e, stats, gi, t[..., gi], x, lw, ode_p, hist, ancs, self._counter + len(idxs), kept, forecast=True,
                            pstats=pstats)

    def smooth(self, n_trajectories=None, seed=None):
        """Backward-simulation smoothing (forward filtering, backward simulation): `n_trajectories` (default N) trajectories
        per patient through the stored particles, each a draw from the joint smoothing distribution p(x_0..x_S | all
        observations) as the particles represent it.  From a draw of the final weights backward, every step weighs ALL N
        particles of the step before by their filter weight times the transition density to the trajectory's next state and
        draws one (include/hode.h, "Particle smoother"; one launch of csrc/hode_smooth.hip, O(B M N S) density evaluations).
        `seed` defaults to the filter's; the draws come from a Philox stream of their own.  Needs store_particles=True; not
        offered on a forecast (no weighted first step) or after a run with `ode_sets` or `learn` (each particle's constants are a static
        part of its state: no particle of the step before with other constants can have led to it, and backward simulation
        across them is not defined -- `smoothed()` remains for that case).  Returns a SmoothResult."""
        if self.history is None or self.predicted is None:
            raise ValueError("smooth() needs run_filter(..., store_particles=True)")
        if self._forecast:
            raise ValueError("smooth() is not offered on a forecast(): it has no weighted first step; smooth the run_filter result")
        e = self._engine
        if getattr(e, "learn", None) is not None:
            raise ValueError("smooth() is not defined for a run with learn (per-particle constants are part of the state, and the "
                             "stored history does not hold them); smoothed() traces the genealogy instead")
        if e.ode_sets:
            raise ValueError("smooth() is not defined for a run with ode_sets (per-particle constants are a static part of the "
                             "state); smoothed() traces the genealogy instead")
        M = e.N if n_trajectories is None else int(n_trajectories)
        if M < 1:
            raise ValueError("n_trajectories must be at least 1")
        idx, paths = hode.capi.pf_smooth(self.history, self.log_weight_history, self.predicted, e.q, self.step_dt, M,
                                         seed=e.seed if seed is None else int(seed), id0=0, link=e.link)
        return SmoothResult(paths.permute(1, 2, 0, 3).contiguous(), idx.permute(1, 2, 0).contiguous(), self.step_index, self.times)


class SmoothResult:
    """M backward-simulated trajectories per patient (`FilterResult.smooth`), tensors on the compute device.
      paths [B, M, S, 6]         the trajectories, in the filter's dtype: paths[b, m, s] = history[s, b, index[b, m, s]]
      index [B, M, S] (int32)    the slot of every step's particle; -1 (and NaN in paths) from the step backward at which no
                                 particle could have led to the trajectory's next state (every candidate dead or impossible)
      step_index [S], times [S] or [B, S]: the filter's
      mean, std [B, S, 6]        fp64, equal weights over the trajectories whose index is not -1 at that step
      lost [B]                   the number of trajectories with an index of -1 anywhere (i.e. at step 0)."""

    def __init__(self, paths, index, step_index, times):
        self.paths, self.index, self.step_index, self.times = paths, index, step_index, times
        ok = (index >= 0).unsqueeze(-1)                                  # [B, M, S, 1]
        n = ok.sum(1).double()                                           # [B, S, 1]
        x = torch.where(ok, paths.double(), torch.zeros((), dtype=torch.float64, device=paths.device))
        self.mean = x.sum(1) / n
        d = torch.where(ok, x - self.mean.unsqueeze(1), torch.zeros((), dtype=torch.float64, device=paths.device))
        self.std = ((d * d).sum(1) / n).sqrt()
        self.lost = (index < 0).any(2).sum(1)

    def quantile(self, q):
        """The q-quantile(s) of every state at every step over the trajectories (lost ones left out): [B, S, 6], or
        [len(q), B, S, 6] for a sequence q."""
        qs = torch.as_tensor(q, dtype=torch.float64, device=self.paths.device)
        return torch.nanquantile(self.paths.double(), qs, dim=1)

    def distinct(self):
        """[B, S] (int64): the number of distinct slots among the trajectories at every step -- what genealogy tracing loses
        far back from the last step and backward simulation keeps."""
        srt = self.index.sort(1).values                                   # [B, M, S]
        new = torch.ones_like(srt, dtype=torch.bool)
        new[:, 1:] = srt[:, 1:] != srt[:, :-1]
        return (new & (srt >= 0)).sum(1)


def _inputs(external_inputs, B, T, dev, dtype):
    ins = {}
    for key in ("meal", "tVNS", "GD"):
        v = (external_inputs or {}).get(key)
        if v is None:
            ins[key] = None
            continue
        v = torch.as_tensor(v).to(dev, dtype)
        if v.dim() == 2:
            if tuple(v.shape) != (B, T):
                raise ValueError(f"external input {key!r} on the grid must be [B, T] = ({B}, {T})")
            ins[key] = v.contiguous()
        else:
            v = v.reshape(-1)
            if v.numel() not in (1, B):
                raise ValueError(f"external input {key!r} must be a scalar, [B] or [B, T]")
            ins[key] = v.expand(B).contiguous()
    return ins


def _check_data(data):
    """The shapes of a batch dict, checked on the host: (initial_state [B, 6], time_points [T] or [B, T], observations
    [B, T, 6], B, T)."""
    x0 = torch.as_tensor(data["initial_state"])
    if x0.dim() != 2 or x0.shape[1] != 6:
        raise ValueError("initial_state must be [B, 6]")
    B = int(x0.shape[0])
    t = torch.as_tensor(data["time_points"])
    T = int(t.shape[-1])
    if t.dim() not in (1, 2) or T < 2 or (t.dim() == 2 and t.shape[0] != B):
        raise ValueError("time_points must be [T] or [B, T] with T >= 2")
    obs = torch.as_tensor(data["observations"])
    if tuple(obs.shape) != (B, T, 6):
        raise ValueError(f"observations must be [B, T, 6] = ({B}, {T}, 6)")
    return x0, t, obs, B, T


def _observed_at(obs_d, mask_d):
    """[T] bool on the device: the grid points at which any patient has an observed entry."""
    seen = torch.isfinite(obs_d) if mask_d is None else mask_d.bool()
    return seen.any(2).any(0)


def _default_steps(obs_d, mask_d):
    """The filter steps when none are given: the later grid points at which any patient has an observed entry, plus the last."""
    at = _observed_at(obs_d, mask_d)
    at[-1] = True
    at[0] = False
    return torch.nonzero(at).reshape(-1).tolist()


def run_filter(model, data, n_particles=1024, process_noise=0.05, noise_link="log", noise_sigma=1.0, initial_spread=0.1, ode_sets=None,
               ess_threshold=0.5, steps=None, seed=0, solver="dopri5", rtol=1e-6, atol=1e-8, dtype=torch.float32, store_particles=False,
               learn=None):
    """Track every patient of `data` with a bootstrap particle filter of `n_particles` (<= 4096) particles.

    data: the samplers' batch dict -- initial_state [B, 6], time_points [T] or [B, T], external_inputs, observations [B, T, 6]
    (NaN = missing), optional observation_mask.  noise_sigma: the observation noise, a scalar, one value per state or an
    ObservationModel with fixed noise.  process_noise / initial_spread: a scalar or one value per state, 0 leaves a state exact;
    noise_link "log" (relative noise) or "additive".  At the first grid point every particle starts at the patient's x0, is
    spread by initial_spread (as a step with dt = 1) and weighted against row 0.  Filter steps: the later grid points at which
    any patient has an observed entry plus the last one, or the ascending grid indices `steps`.  ode_sets: constant name ->
    [N] or [B, N] values, each particle's own mechanistic constants (e.g. thinned posterior draws); they follow their particle
    through resampling.  learn: a ParameterLearning -- the named constants are learned online: their columns are moved after
    every step (the initial rows may still come from ode_sets), and FilterResult.learned follows the cloud.  A step resamples a patient when ESS < ess_threshold * n_particles.  Returns a FilterResult."""
    from models.hybrid_ode_nn import _compute_device, _method
    N = int(n_particles)
    if N < 1:
        raise ValueError("n_particles must be at least 1")
    if N > MAX_PARTICLES:
        raise ValueError(f"n_particles = {N}: the step kernel takes up to {MAX_PARTICLES} particles per patient (HODE_PF_MAX_PARTICLES)")
    if noise_link not in hode.capi.PF_LINK:
        raise ValueError(f"noise_link must be one of {sorted(hode.capi.PF_LINK)}, not {noise_link!r}")
    if not 0.0 <= float(ess_threshold) <= 1.0:
        raise ValueError("ess_threshold must lie in [0, 1]")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be torch.float32 or torch.float64")
    q, q0 = _six_nonneg(process_noise, "process_noise"), _six_nonneg(initial_spread, "initial_spread")
    om = noise_sigma if isinstance(noise_sigma, ObservationModel) else ObservationModel(noise_sigma)
    if om.marginal:
        raise ValueError('run_filter weights under a fixed observation noise: noise="marginal" is not offered here')
    method = _method(solver)
    x0, t, obs, B, T = _check_data(data)
    if learn is not None and not isinstance(learn, ParameterLearning):
        raise ValueError(f"learn must be a ParameterLearning or None, not {type(learn).__name__}")
    cols = {}
    for name, vals in (ode_sets or {}).items():
        key = name[4:] if name.startswith("ode_") else name
        if key not in ODE_PARAM_NAMES:
            raise ValueError(f"unknown mechanistic constant {name!r}; known: {list(ODE_PARAM_NAMES)}")
        v = torch.as_tensor(vals)
        if tuple(v.shape) not in ((N,), (B, N)):
            raise ValueError(f"ode_sets[{name!r}] must be [N] = ({N},) or [B, N] = ({B}, {N})")
        cols[ODE_PARAM_NAMES.index(key)] = v
    idxs = None if steps is None else _check_steps(steps, T)
    model._check_supported()

    dev = _compute_device()
    om.prepare(obs, data.get("observation_mask"), device=dev, dtype=dtype)
    obs_d = om.obs.view(B, T, 6)
    mask_d = None if om.mask is None else om.mask.view(B, T, 6)
    observed = None
    if learn is not None:
        observed = _observed_at(obs_d, mask_d).tolist()                 # (a learning run's own read-back, before the loop)
    if idxs is None:
        idxs = _default_steps(obs_d, mask_d)                            # the one read-back, before the loop
    t = t.to(dev, dtype)
    ins = _inputs(data.get("external_inputs"), B, T, dev, dtype)
    with torch.no_grad():
        _, ode_vec = model._params_on(dev)
        ode_p = ode_vec.detach().to(dtype).reshape(1, 1, 17).repeat(B, N, 1)
        for j, v in cols.items():
            ode_p[:, :, j] = v.to(dev, dtype).expand(B, N)
        x = x0.to(dev, dtype).reshape(B, 1, 6).repeat(1, N, 1)
        lw = torch.zeros(B, N, dtype=torch.float64, device=dev)
    eng = _Engine(model, B, N, q, om.sigma, hode.capi.PF_LINK[noise_link], ess_threshold, seed, method, rtol, atol, dtype, dev,
                  bool(store_particles), ode_sets=bool(cols), learn=learn)
    x, lw, ode_p, stats, hist, ancs, pstats, kept = eng.run(x, lw, ode_p, t, ins, obs_d, mask_d, idxs, 0, init_q=q0, observed=observed)
    gi = torch.as_tensor([0] + idxs, device=dev)
    return FilterResult(eng, stats, gi, t[..., gi], x, lw, ode_p, hist, ancs, 1 + len(idxs), kept, pstats=pstats)
