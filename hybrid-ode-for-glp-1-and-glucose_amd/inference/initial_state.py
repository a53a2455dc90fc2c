"""Latent initial states for run_hmc, run_nuts and run_population: `InitialStatePrior`.

Without it every sampler takes data["initial_state"] as an exact, known number -- in practice the first noisy observation.  The
rates are about 0.02 per minute, so an error in x0 stays in the trajectory for the whole window (errors in variables), and a
record whose first row lacks a state (a NaN) cannot be solved at all.  With a prior, the chosen components of every patient's
initial state are sampled together with the mechanistic constants.

Model.  The latent coordinates w[b, i], one per patient b and latent state i, each have an N(0, 1) prior:
    x0[b, j] = m[b, j] + s[b, j] w[b, rank(j)]              link="identity"
    x0[b, j] = m[b, j] exp(s[b, j] w[b, rank(j)])           link="log" (m > 0): the state stays positive
for the latent j; the other entries stay at data["initial_state"].  y[:, 0] IS x0, so the first observation row is an ordinary
likelihood term of the latent state.  The prior must therefore NOT be "the first observation +- the noise": that would count
the first observation twice.  Take it from knowledge that does not come from this record's first row, e.g. the cohort
(`InitialStatePrior.from_batch`) or the physiological range.

The layer sits between the unchanged sampler kernels and the solve, as inference/population.py does -- the target `_LatentTarget`,
alone or in front of the population's: hode_x0_params maps the
chain coordinates to one initial state per (chain, patient), hode_x0_grad takes the adjoint's per-trajectory gx0 back
(csrc/hode_x0.hip).  A coordinate row is [ z_ode (K) | w (B n_lat) ] for run_hmc / run_nuts, the network at the model's weights,
and [ m | s | z | w ] with w from column K (B + 2) for run_population.  The sampler kernels see n_ode = 0 and P = D "weights"
with an N(0, 1) prior; the solve runs with one x0 row per trajectory (models.hybrid_ode_nn._run_sets(own_x0=True))."""
from typing import Dict

import numpy as np
import torch

import hode
from inference.hmc import HMCResult, _jitter_all, _parse_priors

__all__ = ["InitialStatePrior", "LatentStateResult", "STATE_NAMES"]

STATE_NAMES = ("G", "I", "Glu", "GLP1", "GE", "FFA")
_LINKS = {"identity": 0, "log": 1}


def _state_indices(states) -> list:
    if states is None:
        return list(range(6))
    if isinstance(states, (str, int)):
        states = (states,)
    out = []
    for st in states:
        if isinstance(st, str):
            if st not in STATE_NAMES:
                raise ValueError(f"unknown state {st!r}; known: {list(STATE_NAMES)}")
            out.append(STATE_NAMES.index(st))
        else:
            if not 0 <= int(st) < 6:
                raise ValueError(f"state index {st} outside 0..5")
            out.append(int(st))
    if not out or len(set(out)) != len(out):
        raise ValueError("states must name at least one state, each once")
    return sorted(out)


class InitialStatePrior:
    """The prior of the latent components of every patient's initial state (see the module docstring for the model).

    states: the latent components, names of ("G", "I", "Glu", "GLP1", "GE", "FFA") or indices (default: all six); they are kept
    in ascending state order, n_lat = len(states).  mean, sd: [6] (the same for every patient) or [B, 6]; only the latent
    entries are read, sd > 0 there.  link: "identity" (x0 = m + s w) or "log" (x0 = m exp(s w), needs m > 0).

    The first observation row is a likelihood term of the latent state (y[:, 0] = x0): do not build the prior as "the first
    observation +- the noise", which would use that observation twice."""

    def __init__(self, mean, sd, states=None, link: str = "identity"):
        self.states = _state_indices(states)
        self.n_lat = len(self.states)
        if link not in _LINKS:
            raise ValueError(f"link must be 'identity' or 'log', not {link!r}")
        self.link = link
        f64 = lambda v: (v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))).to("cpu", torch.float64)  # noqa: E731
        self.mean, self.sd = f64(mean), f64(sd)
        for name, v in (("mean", self.mean), ("sd", self.sd)):
            if v.dim() not in (1, 2) or v.shape[-1] != 6:
                raise ValueError(f"{name} must be [6] or [B, 6], not {list(v.shape)}")
        m, s = self.mean[..., self.states], self.sd[..., self.states]
        if not bool(torch.isfinite(m).all()) or not bool(torch.isfinite(s).all()):
            raise ValueError("mean and sd must be finite at the latent states")
        if not bool((s > 0).all()):
            raise ValueError("sd must be > 0 at the latent states")
        if link == "log" and not bool((m > 0).all()):
            raise ValueError("link='log' needs mean > 0 at the latent states")

    @property
    def state_names(self):
        return [STATE_NAMES[j] for j in self.states]

    @property
    def lat_mask(self) -> int:
        return sum(1 << j for j in self.states)

    @classmethod
    def from_batch(cls, batch, states=None, link: str = "identity", inflate: float = 1.0):
        """A cohort-level prior: per state the mean and the sd (ddof 1) over the patients of the finite first observations
        batch["observations"][:, 0], the sd multiplied by `inflate`; the same row for every patient.  A latent state observed at
        fewer than two patients raises ValueError."""
        idx = _state_indices(states)
        first = torch.as_tensor(batch["observations"]).detach().to("cpu", torch.float64)[:, 0]
        mask = batch.get("observation_mask")
        ok = torch.isfinite(first)
        if mask is not None:
            ok &= torch.as_tensor(mask).to("cpu").bool()[:, 0]
        mean, sd = torch.zeros(6, dtype=torch.float64), torch.ones(6, dtype=torch.float64)
        for j in idx:
            v = first[ok[:, j], j]
            if v.numel() < 2:
                raise ValueError(f"state {STATE_NAMES[j]!r} is observed at {v.numel()} patients' first row: a cohort prior needs two")
            mean[j], sd[j] = v.mean(), v.std(unbiased=True) * float(inflate)
        return cls(mean, sd, idx, link)

    def bind(self, B: int, x0_data=None) -> "_BoundPrior":
        """The prior of B patients whose other entries stay at x0_data [B, 6] (None: no batch, the prior alone)."""
        B = int(B)
        rows = []
        for name, v in (("mean", self.mean), ("sd", self.sd)):
            if v.dim() == 2 and v.shape[0] != B:
                raise ValueError(f"{name} holds {v.shape[0]} rows, the batch {B} patients")
            rows.append((v if v.dim() == 2 else v.unsqueeze(0).expand(B, 6)).clone())
        base = None
        if x0_data is not None:
            base = torch.as_tensor(x0_data).detach().to("cpu", torch.float64)
            base = base.unsqueeze(0) if base.dim() == 1 else base
            if tuple(base.shape) != (B, 6):
                raise ValueError(f"initial_state must be [B, 6] = [{B}, 6], not {list(base.shape)}")
            fixed = [j for j in range(6) if j not in self.states]
            if fixed and not bool(torch.isfinite(base[:, fixed]).all()):
                raise ValueError("data['initial_state'] must be finite at the states that are not latent: "
                                 f"{[STATE_NAMES[j] for j in fixed]}")
        return _BoundPrior(rows[0], rows[1], self.states, self.link, base)


class _BoundPrior:
    """An InitialStatePrior of B patients: m, s fp64 [B, 6] (CPU), the latent state indices, the link, and the batch's initial
    states x0_base [B, 6] (None without a batch) that the other entries keep."""

    def __init__(self, m, s, states, link, x0_base):
        self.m, self.s, self.states, self.link, self.x0_base = m, s, list(states), link, x0_base
        self.B, self.n_lat = m.shape[0], len(self.states)
        self.lat_mask = sum(1 << j for j in self.states)
        self.link_code = _LINKS[link]
        self.state_names = [STATE_NAMES[j] for j in self.states]

    def natural(self, w):
        """w [..., B n_lat] -> the latent entries of x0 [..., B, n_lat] (fp64, on w's device)."""
        w = w.double().reshape(*w.shape[:-1], self.B, self.n_lat)
        m, s = self.m[:, self.states].to(w.device), self.s[:, self.states].to(w.device)
        return m * torch.exp(s * w) if self.link_code else m + s * w

    def fill(self, x_lat):
        """The latent entries [..., B, n_lat] -> x0 [..., B, 6] with the other entries from the batch (NaN without one)."""
        out = torch.full((*x_lat.shape[:-2], self.B, 6), float("nan"), dtype=torch.float64, device=x_lat.device)
        if self.x0_base is not None:
            out[...] = self.x0_base.to(x_lat.device)
        out[..., self.states] = x_lat.double()
        return out

    def start(self):
        """w [B, n_lat] at the finite latent entries of the batch's initial states, clamped to +-3, and 0 elsewhere."""
        w = torch.zeros(self.B, self.n_lat, dtype=torch.float64)
        if self.x0_base is None:
            return w
        x, m, s = self.x0_base[:, self.states], self.m[:, self.states], self.s[:, self.states]
        if self.link_code:
            ok = torch.isfinite(x) & (x > 0)
            v = torch.log(torch.where(ok, x, m) / m) / s
        else:
            ok = torch.isfinite(x)
            v = (torch.where(ok, x, m) - m) / s
        return torch.where(ok, v, w).clamp(-3.0, 3.0)


def _bind(initial_state, data, n_patients) -> _BoundPrior:
    """The argument checks of a run with a latent initial state -> the bound prior; no device is touched."""
    if not isinstance(initial_state, InitialStatePrior):
        raise ValueError("initial_state must be an InitialStatePrior (or None)")
    if data is None:
        if n_patients is None or int(n_patients) < 1:
            raise ValueError("data=None samples the prior: give n_patients >= 1")
        return initial_state.bind(int(n_patients), None)
    x0 = torch.as_tensor(data["initial_state"])
    x0 = x0.unsqueeze(0) if x0.dim() == 1 else x0
    if n_patients is not None and int(n_patients) != x0.shape[0]:
        raise ValueError(f"n_patients = {n_patients} but the batch holds {x0.shape[0]}")
    return initial_state.bind(x0.shape[0], x0)


# ---------------------------------------------------------------------------------------------------- target
class _LatentTarget:
    """Latent initial states as a sampler target (inference.hmc._PlainTarget states the protocol).  `inner` is None: the row is
    [ z_ode (g_K) | w ] and this target carries the constants itself (g_names / g_mask / g_mu / g_sd; hode_x0_params and
    hode_x0_grad do both maps).  `inner` is the population target: the row is its row, then w, and this target stands in front
    of it.  The two are two code paths because the kernels fuse differently; `off` is where w starts in either."""

    def __init__(self, initial_state, data, n_patients=None, ode_priors=None, sample_nn=False, inner=None):
        if sample_nn:
            raise ValueError("sample_nn=True cannot be combined with initial_state: the network stays at the model's weights "
                             "(the sampler kernels take no coordinates beyond n_ode + P); pass sample_nn=False")
        self.inner = inner
        self.lat = _bind(initial_state, data, n_patients)
        self.g_names, self.g_mask, self._mu, self._sd = ([], 0, [], []) if inner is not None else _parse_priors(ode_priors)
        self.g_K = len(self.g_names)                                             # K = 0: state estimation at fixed constants

    def layout(self, s):
        f64 = dict(dtype=torch.float64, device=s.dev)
        lat = self.lat
        if self.inner is not None:
            self.inner.layout(s)
            self.g_mu = self.g_sd = None
        else:
            self.g_mu, self.g_sd = torch.tensor(self._mu or [0.0], **f64), torch.tensor(self._sd or [1.0], **f64)
            # what the sampler kernels see: no constants of their own, D = P "weights" whose buffer is the coordinate scratch
            s.ode_names, s.ode_mask, s.n_ode, s.sample_nn, s.nn_names = [], 0, 0, True, []
            s.D = s.P = self.g_K
            s.mu, s.sd = torch.tensor([0.0], **f64), torch.tensor([1.0], **f64)
        self.off = s.D                           # w follows the constants (K) or the population row (K (B + 2))
        s.D = s.P = self.off + lat.B * lat.n_lat
        self.m_d, self.s_d = lat.m.to(s.dev).contiguous(), lat.s.to(s.dev).contiguous()

    def start(self, s):
        from models.ode_core import ODE_PARAM_NAMES
        C, B, lat, R = s.C, self.lat.B, self.lat, dict(dtype=s.dt, device=s.dev)
        if self.inner is not None:
            z = self.inner.start(s)
        else:
            s.nn_p = torch.zeros(C, s.P, **R)                        # the coordinate scratch: row stride P = D
            s.glik = torch.zeros(C, s.P, **R)                        # hode_x0_grad's output, the kernels' gnn
            s.ode_p = s.ode_base.repeat(C).contiguous()
            s.nn_rep = s.nn_base.repeat(C).contiguous()              # the pieces take one copy of the network per chain
            z = torch.zeros(C, s.ld, **R)
            for i, n in enumerate(self.g_names):
                z[:, i] = (float(s.ode_base[ODE_PARAM_NAMES.index(n)]) - float(self.g_mu[i])) / float(self.g_sd[i])
        s.x0_rows = torch.zeros(C * B, 6, **R)                       # hode_x0_params's output: one x0 per (chain, patient)
        z[:, self.off:s.D] = lat.start().reshape(1, B * lat.n_lat).to(s.dev).to(s.dt)
        return z

    def initial_jitter(self, s):
        _jitter_all(s)

    def evaluate(self, s, A):
        """(hode_pop_params ->) hode_x0_params -> the pieces (taped solve of one x0 row per trajectory, the per-chain cotangent,
        the adjoint for gx0 and gode) -> (hode_pop_grad ->) hode_x0_grad."""
        from models.hybrid_ode_nn import OWN_SETS_MAX
        cap, lat, B, pop = hode.capi, self.lat, self.lat.B, self.inner
        x0_args = (A, B, lat.n_lat, s.P, self.off, s.nn_p, lat.lat_mask, lat.link_code, self.m_d, self.s_d)
        if pop is not None:
            pop.params(s, A)
            cap.x0_params(*x0_args, s.x0, s.x0_rows)
            gx0, _, gode = s._run_pieces(A, (True, False, True), x0=s.x0_rows[:A * B], ode_vec=s.ode_p, nn_flat=s.nn_base,
                                         max_traj=OWN_SETS_MAX, own_sets=True, own_x0=True)
            pop.grad(s, A, gode)
            cap.x0_grad(*x0_args, gx0, s.glik)
        else:
            cap.x0_params(*x0_args, s.x0, s.x0_rows, self.g_K, self.g_mask, self.g_mu, self.g_sd, s.ode_base, s.ode_p)
            gx0, _, gode = s._run_pieces(A, (True, False, self.g_K > 0), x0=s.x0_rows[:A * B], ode_vec=s.ode_p, nn_flat=s.nn_rep,
                                         own_x0=True)
            cap.x0_grad(*x0_args, gx0, s.glik, self.g_K, self.g_mask, self.g_sd, gode)
            s.gnn, s.gode = s.glik, None
        s.gx0_rows = gx0


# ---------------------------------------------------------------------------------------------------- result
class LatentStateResult(HMCResult):
    """Draws of run_hmc / run_nuts with a latent initial state.  `draws` [chains, draws, K + B n_lat] holds natural units: the K
    sampled constants, then x0 of the latent entries (patient-major); `raw` the chain coordinates.  `initial_states()`:
    [C, n, B, 6] with the entries that are not latent filled in from the batch; `samples`: "ode.<name>" [C, n] and "x0"
    [C, n, B, n_lat]; `summary()`: "ode.<name>" and "x0.<state>" ([B]); `rhat()` / `ess()` over all of `draws`; `predict()` and
    `predictive_summary()` on the run's batch solve every kept draw from its own drawn x0."""

    def __init__(self, raw, ode_names, mu, sd, latent: _BoundPrior, stats=None, model=None, ode_base=None, nn_base=None, observation=None,
                 data=None):
        raw = torch.as_tensor(raw)
        K, lat = len(ode_names), latent
        if raw.dim() != 3 or raw.shape[2] != K + lat.B * lat.n_lat:
            raise ValueError(f"draws must be [chains, draws, K + B n_lat] = [., ., {K + lat.B * lat.n_lat}]")
        f64 = lambda v: torch.as_tensor(v, dtype=torch.float64).reshape(-1)[:K].to(raw.device)       # noqa: E731
        C, n = raw.shape[:2]
        const = f64(mu) + f64(sd) * raw[..., :K].double() if K else raw[..., :0].double()
        x = lat.natural(raw[..., K:]).reshape(C, n, lat.B * lat.n_lat)
        nat = torch.cat([const, x], 2)
        super().__init__(nat.to(raw.dtype) if raw.dtype in (torch.float32, torch.float64) else nat, ode_names, [],
                         stats if stats is not None else {}, model, ode_base, nn_base, observation, data)
        self.raw, self.latent, self.K = raw, lat, K

    def _x_lat(self):
        C, n = self.draws.shape[:2]
        return self.draws[..., self.K:].reshape(C, n, self.latent.B, self.latent.n_lat)

    def initial_states(self) -> torch.Tensor:
        """x0 of every draw, [C, n, B, 6] (fp64, on the draws' device); entries that are not latent are the batch's."""
        return self.latent.fill(self._x_lat())

    @property
    def samples(self) -> Dict[str, np.ndarray]:
        if self._samples is None:
            d = self.draws.detach().cpu().numpy()
            out = {f"ode.{name}": d[:, :, i].copy() for i, name in enumerate(self.ode_names)}
            out["x0"] = self._x_lat().detach().cpu().numpy().copy()
            self._samples = out
        return self._samples

    def summary(self) -> Dict[str, Dict[str, np.ndarray]]:
        """{key: {mean, std, median, q025, q975, rhat, ess}} for "ode.<name>" (scalars) and "x0.<state>" ([B])."""
        C, n = self.draws.shape[:2]
        lat = self.latent
        by_state = self._x_lat().transpose(2, 3).reshape(C, n, lat.n_lat * lat.B)          # [i][b]
        tmp = HMCResult(torch.cat([self.draws[..., :self.K], by_state], 2), self.ode_names, [(f"x0.{s}", (lat.B,)) for s in lat.state_names],
                        self.stats)
        return {(k[3:] if k.startswith("nn.") else k): v for k, v in tmp.summary().items()}

    def _param_sets(self, thin=1):
        from models.ode_core import ODE_PARAM_NAMES
        d = self.draws[:, ::thin].reshape(-1, self.draws.shape[2]).to(torch.float32)
        S = d.shape[0]
        ode = self.ode_base.to(d.device, torch.float32).reshape(1, 17).repeat(S, 1)
        for i, n in enumerate(self.ode_names):
            ode[:, ODE_PARAM_NAMES.index(n)] = d[:, i]
        nn = self.nn_base.to(d.device, torch.float32).reshape(1, -1).repeat(S, 1)
        return S, nn.contiguous().reshape(-1), ode.reshape(-1).contiguous()

    def _kept_x0(self, thin):
        """[S, B, 6] of the kept draws, in `predict`'s order."""
        return self.initial_states()[:, ::thin].reshape(-1, self.latent.B, 6)

    def _own(self, initial_state):
        return initial_state is None or (self.data is not None and initial_state is self.data.get("initial_state"))

    def _solve_draws(self, initial_state, t_span, external_inputs, thin, solver, rtol, atol):
        if not self._own(initial_state):
            return super()._solve_draws(initial_state, t_span, external_inputs, thin, solver, rtol, atol)
        from inference.predictive import _rep_inputs
        if self.model is None:
            raise ValueError("this result carries no model (built from arrays)")
        if self.data is None:
            raise ValueError("predict from the drawn initial states needs the run's batch: the run had none")
        m = self.model
        S, nn_flat, ode_vec = self._param_sets(thin)
        xs = self._kept_x0(thin).to(torch.float32)
        B = xs.shape[1]
        _, ts, us = _rep_inputs(S, xs[0], t_span, external_inputs)
        with torch.no_grad():
            y = m._solve(xs.reshape(S * B, 6), ts, us, solver, rtol, atol, n_sets=S, nn_flat=nn_flat, ode_vec=ode_vec, differentiable=False)
        m._warn_failures(m.last_solve_info)
        return y.reshape(S, B, y.shape[1], 6)

    def predict(self, initial_state=None, t_span=None, external_inputs=None, thin=1, solver="dopri5", rtol=1e-6, atol=1e-8,
                observation_noise=False, data=None, seed=0):
        """HMCResult.predict; with initial_state=None every kept draw is solved from its own drawn x0 for the run's patients
        -> [n_draws, B, T, 6].  t_span (default: the batch's grid) may extend beyond the data -- the forecast -- and
        external_inputs (default: the batch's) must then be given on that grid."""
        if initial_state is None:
            if self.data is None:
                raise ValueError("predict from the drawn initial states needs the run's batch: the run had none")
            if t_span is None:
                t_span = self.data["time_points"]
                external_inputs = self.data.get("external_inputs") if external_inputs is None else external_inputs
        elif t_span is None:
            raise ValueError("predict with an initial_state of its own needs t_span")
        return super().predict(initial_state, t_span, external_inputs, thin, solver, rtol, atol, observation_noise, data, seed)

    def predictive_summary(self, batch=None, thin=1, observation_noise=True, seed=0, n_bins=10, max_bytes=None, solver="dopri5",
                           rtol=1e-6, atol=1e-8, *, quantiles=None, loo=False, r_eff=1.0):
        """HMCResult.predictive_summary; on the run's batch (batch=None) every kept draw is solved from its own drawn x0."""
        if batch is not None and batch is not self.data:
            return super().predictive_summary(batch, thin, observation_noise, seed, n_bins, max_bytes, solver, rtol, atol,
                                              quantiles=quantiles, loo=loo, r_eff=r_eff)
        from inference import predictive as PR
        if self.model is None:
            raise ValueError("this result carries no model (built from arrays)")
        if self.data is None:
            raise ValueError("predictive_summary needs a batch: the run had none")
        if loo and not observation_noise:
            raise ValueError("loo needs observation_noise=True: without observation noise there is no likelihood")
        batch = self.data
        S, nn_flat, ode_vec = self._param_sets(thin)
        sigma = self.noise_sigma(batch, thin, seed, solver, rtol, atol) if observation_noise else None
        return PR.predictive_summary(self.model, (nn_flat.view(S, -1), ode_vec.view(S, 17)), batch, sigma=sigma, n_bins=n_bins,
                                     max_bytes=PR._DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, solver=solver, rtol=rtol,
                                     atol=atol, quantiles=quantiles, loo=loo, r_eff=r_eff, initial_states=self._kept_x0(thin))
