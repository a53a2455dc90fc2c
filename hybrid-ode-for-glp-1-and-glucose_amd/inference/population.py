"""A hierarchical population posterior over a HybridODENN's mechanistic constants on the GPU: `run_population`.

Between run_hmc / run_nuts (ONE parameter vector for the whole batch) and fit_patients (every patient alone): each of the B
patients has their own K mechanistic constants theta_b, drawn from a population distribution whose mean and spread are inferred
from all patients together.  The network stays fixed at the model's weights.

Model, non-centred, every chain coordinate with an N(0, 1) prior (a row is [ m | s | z_0 | ... | z_{B-1} ], K values each, k in
ascending ODE-index order; `layout`):
    mu_pop_k    = mu0_k + sd0_k m_k              ode_priors as the hyperprior on the population mean
    tau_k       = tau0_k exp(omega s_k)          a log-normal hyperprior on the between-patient sd (tau0 = sd0, omega = 0.5)
    theta_{b,k} = mu_pop_k + tau_k z_{b,k}
    U           = NLL(theta_1..theta_B) + |coords|^2 / 2

The population model is a reparameterisation layer between the samplers' chain coordinates and the solve's per-set constants,
the target `_PopulationTarget` that inference.hmc's `_Sampler` / inference.nuts's `_NutsSampler` is handed: hode_pop_params maps
the coordinates to one row of constants per (chain, patient), hode_pop_grad takes the adjoint's per-set gradient back
(csrc/hode_population.hip).  The sampler kernels of run_hmc and run_nuts run unchanged: they see the coordinates
as "P weights with an N(0, 1) prior" (n_ode = 0, sample_nn = True) whose parameter buffer is the coordinate scratch and whose
likelihood gradient is hode_pop_grad's output.  The solve and the adjoint run with one parameter set per trajectory
(models.hybrid_ode_nn._run_sets(own_sets=True)); the per-chain likelihood kernels run with set = chain over B T 6 entries."""
from typing import Dict, Optional, Tuple

import numpy as np
import torch

import hode
from inference.hmc import HMCResult, _ess, _jitter_all, _parse_priors, _rank_normal, _rhat, _run_schedule, _split

__all__ = ["run_population", "PopulationResult", "layout"]


def layout(K: int, B: int) -> Dict[str, object]:
    """The row layout of K constants x B patients: slices `m`, `s` (K each), `z` (B K values, patient-major) and the length D."""
    K, B = int(K), int(B)
    if K < 1 or B < 1:
        raise ValueError("K and B must be >= 1")
    return {"m": slice(0, K), "s": slice(K, 2 * K), "z": slice(2 * K, K * (B + 2)), "D": K * (B + 2)}


def _hyper(ode_priors, tau_scale, tau_log_sd):
    """(names in ascending ODE-index order, mu0, sd0, tau0 as float lists) after the argument checks; no device is touched."""
    names, _, mu0, sd0 = _parse_priors(ode_priors)
    if not names:
        raise ValueError("nothing to sample: ode_priors names no constant")
    if not float(tau_log_sd) > 0.0:
        raise ValueError("tau_log_sd must be > 0")
    if tau_scale is None:
        tau0 = list(sd0)
    elif isinstance(tau_scale, dict):
        for k in tau_scale:
            if k not in names:
                raise ValueError(f"tau_scale names {k!r}, which is not sampled; sampled: {names}")
        tau0 = [float(tau_scale.get(n, s)) for n, s in zip(names, sd0)]
    else:
        tau0 = [float(tau_scale)] * len(names)
    if not all(np.isfinite(v) and v > 0.0 for v in tau0):
        raise ValueError("tau_scale must be positive")
    return names, mu0, sd0, tau0


def _init_theta(init, names, B):
    """init (a fit_patients result for the same constants, or a [B, K] tensor) -> fp64 [B, K] on the CPU, or None."""
    if init is None:
        return None
    if hasattr(init, "params") and hasattr(init, "names"):
        missing = [n for n in names if n not in init.params]
        if missing:
            raise ValueError(f"init holds no fit of {missing}")
        th = torch.stack([torch.as_tensor(init.params[n]).detach().double().cpu().reshape(-1) for n in names], 1)
    else:
        th = torch.as_tensor(init).detach().double().cpu()
    if tuple(th.shape) != (B, len(names)):
        raise ValueError(f"init must hold [B, K] = [{B}, {len(names)}] values, not {list(th.shape)}")
    return th


class _PopulationTarget:
    """The population model as a sampler target (inference.hmc._PlainTarget states the protocol): the constructor is the
    host-side validation; the hyperparameters mu0 / sd0 / tau0 live here, on the device from `layout` on."""

    def __init__(self, data, n_patients=None, ode_priors=None, tau_scale=None, tau_log_sd=0.5, init=None):
        self.pop_names, *self._hyp = _hyper(ode_priors, tau_scale, tau_log_sd)
        if data is None:
            if n_patients is None or int(n_patients) < 1:
                raise ValueError("data=None samples the prior: give n_patients >= 1")
            self.B = int(n_patients)
        else:
            self.B = int(data["initial_state"].shape[0])
            if n_patients is not None and int(n_patients) != self.B:
                raise ValueError(f"n_patients = {n_patients} but the batch holds {self.B}")
        self.K, self.omega = len(self.pop_names), float(tau_log_sd)
        self._init = _init_theta(init, self.pop_names, self.B)

    def layout(self, s):
        from models.ode_core import ODE_PARAM_NAMES
        f64 = dict(dtype=torch.float64, device=s.dev)
        self.pop_mask = sum(1 << ODE_PARAM_NAMES.index(n) for n in self.pop_names)
        self.mu0, self.sd0, self.tau0 = (torch.tensor(v, **f64) for v in self._hyp)
        # what the sampler kernels see: no constants of their own, D = P "weights" whose buffer is the coordinate scratch
        s.ode_names, s.ode_mask, s.n_ode, s.sample_nn, s.nn_names = [], 0, 0, True, []
        s.D = s.P = layout(self.K, self.B)["D"]
        s.mu, s.sd = torch.tensor([0.0], **f64), torch.tensor([1.0], **f64)

    def start(self, s):
        from models.ode_core import ODE_PARAM_NAMES
        C, K, B, R = s.C, self.K, self.B, dict(dtype=s.dt, device=s.dev)
        s.nn_p = torch.zeros(C, s.P, **R)                          # the coordinate scratch: row stride P = D
        s.glik = torch.zeros(C, s.P, **R)                          # hode_pop_grad's output, the kernels' gnn
        s.ode_p = torch.empty(C * B * 17, **R)
        lay = layout(K, B)
        base = torch.stack([s.ode_base[ODE_PARAM_NAMES.index(n)] for n in self.pop_names]).double()
        z = torch.zeros(C, s.ld, **R)
        z[:, lay["m"]] = ((base - self.mu0) / self.sd0).to(s.dt)
        if self._init is not None:
            zb = ((self._init.to(s.dev) - base) / self.tau0).clamp(-3.0, 3.0)
            z[:, lay["z"]] = zb.reshape(1, B * K).to(s.dt)
        return z

    def initial_jitter(self, s):
        _jitter_all(s)

    def params(self, s, A):
        """hode_pop_params: the first A rows of the coordinate scratch -> one row of constants per (chain, patient) in ode_p."""
        hode.capi.pop_params(A, self.B, self.K, s.P, s.nn_p, self.pop_mask, self.mu0, self.sd0, self.tau0, self.omega, s.ode_base, s.ode_p)

    def grad(self, s, A, gode):
        """hode_pop_grad: the adjoint's per-set gode -> glik, the kernels' gnn."""
        hode.capi.pop_grad(A, self.B, self.K, s.P, s.nn_p, gode, self.pop_mask, self.sd0, self.tau0, self.omega, s.glik)
        s.gnn, s.gode, s.gode_sets = s.glik, None, gode

    def evaluate(self, s, A):
        """hode_pop_params -> the pieces (taped solve of the per-(chain, patient) constants and ONE network, the per-chain
        cotangent, the adjoint for gode) -> hode_pop_grad."""
        from models.hybrid_ode_nn import OWN_SETS_MAX
        self.params(s, A)
        _, _, gode = s._run_pieces(A, (False, False, True), x0=s.x0, ode_vec=s.ode_p, nn_flat=s.nn_base, max_traj=OWN_SETS_MAX,
                                   own_sets=True)
        self.grad(s, A, gode)


# ---------------------------------------------------------------------------------------------------- result
class PopulationResult:
    """Draws of run_population.  `draws`: the raw chain coordinates [chains, draws, D] (`layout`); `names`: the K constants;
    `population()`: {"mu", "tau"} [C, n, K]; `patients()`: [C, n, B, K] in natural units; `samples` / `flat()`: numpy arrays keyed
    `pop.mu.<name>`, `pop.tau.<name>` ([C, n]) and `patient.<name>` ([C, n, B]); `rhat()` / `ess()` / `summary()` over those
    natural quantities, keyed the same way; `pooling()`: the Gelman-Pardoe pooling factor of every constant; `stats` as run_hmc's
    / run_nuts's; `predict`, `predict_new`, `predictive_summary`: the posterior predictive of the run's patients or of new ones."""

    def __init__(self, draws, names, n_patients, mu0, sd0, tau0, tau_log_sd=0.5, stats=None, model=None, ode_base=None, nn_base=None,
                 observation=None, data=None, latent=None):
        self.draws = torch.as_tensor(draws)
        self.names, self.B, self.K = list(names), int(n_patients), len(names)
        self.latent = latent                     # the bound InitialStatePrior of a run with initial_state (inference/initial_state.py)
        n_w = 0 if latent is None else latent.B * latent.n_lat
        if self.draws.dim() != 3 or self.draws.shape[2] != layout(self.K, self.B)["D"] + n_w:
            raise ValueError(f"draws must be [chains, draws, K (B + 2)] = [., ., {layout(self.K, self.B)['D']}]" +
                             (f" + B n_lat = {n_w}" if n_w else ""))
        f64 = lambda v: torch.as_tensor(v, dtype=torch.float64).reshape(self.K)          # noqa: E731
        self.mu0, self.sd0, self.tau0, self.omega = f64(mu0), f64(sd0), f64(tau0), float(tau_log_sd)
        self.stats = stats if stats is not None else {}
        self.model, self.ode_base, self.nn_base = model, ode_base, nn_base
        self.observation, self.data = observation, data
        self._nat = None

    @property
    def n_chains(self):
        return self.draws.shape[0]

    @property
    def n_draws(self):
        return self.draws.shape[1]

    def population(self) -> Dict[str, torch.Tensor]:
        """{"mu": mu_pop, "tau": tau}, each [C, n, K] (fp64, on the draws' device)."""
        d, lay = self.draws.double(), layout(self.K, self.B)
        dev = d.device
        return {"mu": self.mu0.to(dev) + self.sd0.to(dev) * d[..., lay["m"]],
                "tau": self.tau0.to(dev) * torch.exp(self.omega * d[..., lay["s"]])}

    def _offsets(self):
        """tau_k z_{b,k}: every patient's offset from the population mean, [C, n, B, K]."""
        d, lay = self.draws.double(), layout(self.K, self.B)
        C, n = d.shape[:2]
        return self.population()["tau"].unsqueeze(2) * d[..., lay["z"]].reshape(C, n, self.B, self.K)

    def patients(self) -> torch.Tensor:
        """theta_{b,k} of every draw, [C, n, B, K] in natural units (fp64, on the draws' device)."""
        return self.population()["mu"].unsqueeze(2) + self._offsets()

    def initial_states(self) -> torch.Tensor:
        """x0 of every draw of a run with initial_state, [C, n, B, 6] (fp64, on the draws' device): the latent entries from the
        draws' w columns (from K (B + 2)), the others from the batch."""
        if self.latent is None:
            raise ValueError("the run had no latent initial state (run_population(initial_state=...))")
        return self.latent.fill(self.latent.natural(self.draws[..., layout(self.K, self.B)["D"]:]))

    def _x0_rows(self, thin, x0):
        """What _solve_rows takes as x0: the batch's rows, or [S, B, 6] of the kept draws' own initial states."""
        if self.latent is None or x0 is None:
            return x0
        return self.initial_states()[:, ::thin].reshape(-1, self.B, 6).to(torch.float32)

    def _natural(self) -> HMCResult:
        """The natural quantities as an HMCResult whose "weights" are pop.mu.<name>, pop.tau.<name> (scalars) and
        patient.<name> ([B]): its samples / rhat / ess / summary are this result's."""
        if self._nat is None:
            pop = self.population()
            C, n = self.draws.shape[:2]
            th = self.patients().transpose(2, 3).reshape(C, n, self.K * self.B)          # [k][b]
            keys = ([(f"pop.mu.{k}", ()) for k in self.names] + [(f"pop.tau.{k}", ()) for k in self.names] +
                    [(f"patient.{k}", (self.B,)) for k in self.names])
            cols = [pop["mu"], pop["tau"], th]
            if self.latent is not None:          # x0.<state> [B] of the latent entries
                lat = self.latent
                cols.append(self.initial_states()[..., lat.states].transpose(2, 3).reshape(C, n, lat.n_lat * self.B))
                keys += [(f"x0.{st}", (self.B,)) for st in lat.state_names]
            self._nat = HMCResult(torch.cat(cols, 2), [], keys, self.stats)
        return self._nat

    @property
    def samples(self) -> Dict[str, np.ndarray]:
        return {k[3:]: v for k, v in self._natural().samples.items()}

    def flat(self) -> Dict[str, np.ndarray]:
        return {k: v.reshape(v.shape[0] * v.shape[1], *v.shape[2:]) for k, v in self.samples.items()}

    def _keyed(self, v):
        out, off = {}, 0
        for name, shape in self._natural().nn_names:
            k = int(np.prod(shape))
            out[name] = v[off:off + k].reshape(shape)
            off += k
        return out

    def rhat(self) -> Dict[str, torch.Tensor]:
        """Split R-hat of every natural quantity, keyed like `samples` (fp64)."""
        return self._keyed(_rhat(self._natural().draws))

    def ess(self, kind="bulk") -> Dict[str, torch.Tensor]:
        """Multi-chain ESS of every natural quantity, keyed like `samples`: "bulk" (rank-normalised) or "mean"."""
        x = self._natural().draws.double()
        return self._keyed(_ess(_split(_rank_normal(x) if kind == "bulk" else x)))

    def summary(self) -> Dict[str, Dict[str, np.ndarray]]:
        """{key: {mean, std, median, q025, q975, rhat, ess}} of every natural quantity (HMCResult.summary: the tail kernels)."""
        return {k[3:]: v for k, v in self._natural().summary().items()}

    def pooling(self) -> torch.Tensor:
        """[K] the pooling factor of Gelman & Pardoe (2006) of every constant, 1 - Var_b(E[tau_k z_bk]) / E[Var_b(tau_k z_bk)]
        (E over all draws, Var_b the ddof-1 variance across patients): 0 = no pooling, 1 = complete pooling; NaN for B = 1."""
        e = self._offsets().reshape(-1, self.B, self.K)
        return 1.0 - e.mean(0).var(0, unbiased=True) / e.var(1, unbiased=True).mean(0)

    # ------------------------------------------------------------------ predictive
    def _need_model(self):
        if self.model is None:
            raise ValueError("this result carries no model (built from arrays)")

    def _ode_rows(self, theta):
        """theta [S, B, K] -> the constants [S * B, 17] (fp32, on the compute device)."""
        from models.hybrid_ode_nn import _compute_device
        from models.ode_core import ODE_PARAM_NAMES
        dev = _compute_device()
        S, B = theta.shape[:2]
        ode = self.ode_base.to(dev, torch.float32).reshape(1, 17).repeat(S * B, 1)
        th = theta.to(dev, torch.float32).reshape(S * B, self.K)
        for i, n in enumerate(self.names):
            ode[:, ODE_PARAM_NAMES.index(n)] = th[:, i]
        return ode

    def _solve_rows(self, ode, S, x0, t_span, external_inputs, solver, rtol, atol):
        """One forward solve of S draws x the B patients of x0, every trajectory with its own constants and the network shared
        -> (y [S, B, T, 6], status [S, B]) on the compute device."""
        from inference.predictive import _rep_inputs
        m = self.model
        own = x0.dim() == 3                      # [S, B, 6]: every draw's own initial states
        x0 = x0.unsqueeze(0) if x0.dim() == 1 else x0
        B = x0.shape[-2]
        xs, ts, us = _rep_inputs(S, x0[0] if own else x0, t_span, external_inputs)
        if own:
            xs = x0.reshape(S * B, 6)
        with torch.no_grad():
            y = m._solve(xs, ts, us, solver, rtol, atol, n_sets=S * B, nn_flat=self.nn_base.to(ode.device, torch.float32),
                         ode_vec=ode.reshape(-1).contiguous(), nn_shared=True)
        info = m.last_solve_info
        m._warn_failures(info)
        return y.view(S, B, y.shape[1], 6), info["status"].view(S, B)

    def _kept(self, thin):
        """theta [S, B, K] of the kept draws (every `thin`-th of each chain)."""
        th = self.patients()[:, ::thin]
        return th.reshape(-1, self.B, self.K)

    def _new(self, thin, n_new, seed):
        """theta = mu_pop + tau xi of n_new NEW patients for every kept draw, [S, n_new, K]."""
        pop = self.population()
        mu, tau = (pop[k][:, ::thin].reshape(-1, 1, self.K) for k in ("mu", "tau"))
        gen = torch.Generator(device=mu.device).manual_seed(int(seed))
        xi = torch.randn(mu.shape[0], n_new, self.K, dtype=torch.float64, device=mu.device, generator=gen)
        return mu + tau * xi

    def predict(self, thin=1, solver="dopri5", rtol=1e-6, atol=1e-8):
        """The posterior predictive of the run's patients, each with their own constants, for the kept draws (every `thin`-th of
        each chain): ONE forward solve of n_draws x B parameter sets -> [n_draws, B, T, 6]."""
        self._need_model()
        if self.data is None:
            raise ValueError("predict needs the run's batch: the run had none (predict_new takes one)")
        th = self._kept(thin)
        d = self.data
        y, _ = self._solve_rows(self._ode_rows(th), th.shape[0], self._x0_rows(thin, d["initial_state"]), d["time_points"],
                                d.get("external_inputs"), solver, rtol, atol)
        return y.to(self.model.device)

    def predict_new(self, initial_state, t_span, external_inputs=None, thin=1, seed=0, solver="dopri5", rtol=1e-6, atol=1e-8):
        """The predictive of NEW patients (the rows of initial_state): theta = mu_pop + tau xi, xi ~ N(0, 1) drawn per kept draw
        and patient from `seed` -> [n_draws, B_new, T, 6]."""
        self._need_model()
        x0 = initial_state.unsqueeze(0) if initial_state.dim() == 1 else initial_state
        th = self._new(thin, x0.shape[0], seed)
        y, _ = self._solve_rows(self._ode_rows(th), th.shape[0], x0, t_span, external_inputs, solver, rtol, atol)
        return y.to(self.model.device)

    def predictive_summary(self, batch=None, thin=1, new_patients=False, quantiles=None, seed=0, n_bins=10, max_bytes=None,
                           solver="dopri5", rtol=1e-6, atol=1e-8):
        """The posterior predictive of the kept draws on `batch` (default: the run's) as a PredictiveSummary (mean / std / PIT per
        entry, the scores against the batch's observations, with `quantiles` the exact quantiles across the draws), folded piece
        by piece through PredictiveAccumulator.fold under max_bytes of trajectories: the whole [n_draws, B, T, 6] block never
        exists, and the result does not depend on the cut.  new_patients=True treats the batch's rows as new patients
        (`predict_new`'s constants); otherwise they are the run's patients, in order."""
        from inference import predictive as PR
        self._need_model()
        own_x0 = self.latent is not None and not new_patients and (batch is None or batch is self.data)
        batch = self.data if batch is None else batch
        if batch is None:
            raise ValueError("predictive_summary needs a batch: the run had none")
        x0 = batch["initial_state"]
        x0 = x0.unsqueeze(0) if x0.dim() == 1 else x0
        Bn, T = x0.shape[0], torch.as_tensor(batch["time_points"]).shape[-1]
        if not new_patients and Bn != self.B:
            raise ValueError(f"the batch holds {Bn} patients, the run had {self.B}: new_patients=True draws constants for new ones")
        th = self._new(thin, Bn, seed) if new_patients else self._kept(thin)
        S = th.shape[0]
        ode = self._ode_rows(th).view(S, Bn, 17)
        xs = self._x0_rows(thin, x0) if own_x0 else None          # [S, B, 6]: every draw's own initial states
        # the run's fixed observation noise enters the PIT and std; an inferred one (noise="marginal") is not drawn here
        sig = None if self.observation is None or self.observation.marginal else self.observation.sigma
        acc = PR.PredictiveAccumulator(Bn, T, batch.get("observations"), batch.get("observation_mask"), torch.float32, quantiles=quantiles,
                                       expected_draws=None if quantiles is None else max(S, 1))
        for lo, hi in PR.cut_draws(S, Bn * T * 6 * 4, PR._DEFAULT_MAX_BYTES if max_bytes is None else max_bytes):
            y, status = self._solve_rows(ode[lo:hi], hi - lo, xs[lo:hi] if own_x0 else x0, batch["time_points"],
                                         batch.get("external_inputs"), solver, rtol, atol)
            acc.fold(y, sig, status)
            del y
        return acc.finish(n_bins)


# ---------------------------------------------------------------------------------------------------- entry point
def run_population(model, data: Optional[Dict[str, torch.Tensor]], num_samples: int = 1000, num_warmup: int = 500, n_chains: int = 16,
                   sampler: str = "hmc", n_leapfrog: int = 16, max_tree_depth: int = 10, target_accept: float = 0.8,
                   noise_sigma: float = 1.0, ode_priors: Optional[Dict[str, Tuple[float, float]]] = None, tau_scale=None,
                   tau_log_sd: float = 0.5, init=None, thin: int = 1, seed: int = 0, solver: str = "dopri5", rtol: float = 1e-6,
                   atol: float = 1e-8, dtype=torch.float32, jitter: float = 0.1, progress=None, noise: str = "fixed", noise_prior=None,
                   n_patients: Optional[int] = None, initial_state=None) -> PopulationResult:
    """Sample the hierarchical population posterior of `model`'s mechanistic constants given the batch `data` (one row per
    patient; None with n_patients: the prior alone) with n_chains chains of HMC (`sampler="hmc"`, n_leapfrog steps) or NUTS
    (`sampler="nuts"`, max_tree_depth).  See the module docstring for the model.

    ode_priors: name -> (mean, sd), the hyperprior of every population mean (default: the reference's seven constants);
    tau_scale: the median tau0 of the between-patient sd, a scalar or name -> value (default: the prior's sd);
    tau_log_sd: the sd of log tau.  init: a fit_patients result for the same constants, or [B, K] values: the chains start at
    z_{b,k} = clip((theta_{b,k} - mu_pop_k) / tau0_k, +-3) instead of 0.  The observation model (noise_sigma, noise,
    noise_prior), warm-up, thinning, seed, solver and `progress` are run_hmc's.  initial_state: an InitialStatePrior
    (inference/initial_state.py) makes the chosen components of every patient's initial state latent; the row is then
    [ m | s | z | w ] with w from column K (B + 2), and the result's `initial_states()`, `predict` and `predictive_summary` pair
    every draw with its own x0."""
    if sampler not in ("hmc", "nuts"):
        raise ValueError(f"sampler must be 'hmc' or 'nuts', not {sampler!r}")
    t = pop = _PopulationTarget(data, n_patients, ode_priors, tau_scale, tau_log_sd, init)
    if initial_state is not None:
        from inference.initial_state import _LatentTarget
        t = _LatentTarget(initial_state, data, n_patients, inner=pop)          # the latent states stand in front of the population
    s, draws, stats = _run_schedule(sampler, model, data, target=t, n_chains=n_chains, n_leapfrog=n_leapfrog, max_tree_depth=max_tree_depth,
                                    num_samples=num_samples, num_warmup=num_warmup, thin=thin, target_accept=target_accept,
                                    progress=progress, noise_sigma=noise_sigma, seed=seed, solver=solver, rtol=rtol, atol=atol,
                                    dtype=dtype, jitter=jitter, noise=noise, noise_prior=noise_prior)
    return PopulationResult(draws, pop.pop_names, pop.B, pop.mu0.cpu(), pop.sd0.cpu(), pop.tau0.cpu(), pop.omega, stats, model, s.ode_base,
                            s.nn_base, s.om, data, None if t is pop else t.lat)
