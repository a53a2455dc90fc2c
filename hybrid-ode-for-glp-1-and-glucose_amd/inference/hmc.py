"""Multi-chain Hamiltonian Monte Carlo over a HybridODENN on the GPU: `run_hmc`, the replacement for the reference's
`run_nuts` (inference/mcmc.py:17-173, a one-chain random-walk placeholder that samples its prior).

Target (the density run_nuts intends, mcmc.py:50-98): a Gaussian likelihood over one batch dict {initial_state, observations,
time_points, external_inputs[, observation_mask]} -- noise_sigma fixed (a scalar or one value per state) or, noise="marginal",
inferred (inference/observation.py; NaN or masked observations are missing); Gaussian priors on the sampled mechanistic constants (the
reference's seven by default) and N(0, 1) on every MLP weight.  The chains move in prior-standardised coordinates z
(theta_ode = mu + sd z, theta_nn = z), so the identity is a sensible first mass matrix.

Static-trajectory HMC with C independent chains: each leapfrog step is ONE forward solve with tape + ONE adjoint over all
C x N trajectories (the C positions ride in the kernels' parameter-set dimension), the per-chain sum of squares and its
cotangent come from hode_mse_sets, and everything else a step does to the chains (momentum, kicks, drifts, the Metropolis
test, dual averaging, draws, the mass matrix) is a HIP kernel of csrc/hode_hmc.hip.  Step sizes are per chain (dual
averaging, Stan's constants), the diagonal mass matrix is pooled across chains over Stan's doubling warm-up windows.

Two things are kept apart.  What a chain's D coordinates mean is a target: `_PlainTarget` here (the density above),
inference/population.py's and inference/initial_state.py's for the other posteriors.  How chains move is `_Sampler` (and
inference/nuts.py's `_NutsSampler`, the same plus the tree state), which is handed a target and never subclassed per posterior.
`_run_schedule` is the one driver of run_hmc, run_nuts and run_population: the warm-up schedule around the HMC or the NUTS
transition."""
import math
from functools import partial
from typing import Dict, Optional, Tuple

import numpy as np
import torch

import hode

__all__ = ["run_hmc", "HMCResult", "REFERENCE_PRIORS"]

# reference inference/mcmc.py:60-68
REFERENCE_PRIORS = {"a_GI": (0.0104, 0.002), "k_I": (0.025, 0.005), "rho": (0.003, 0.001), "E_max": (0.1, 0.02),
                    "V_max": (9.0, 2.0), "K_m": (7.0, 1.5), "k_L": (0.02, 0.005)}

_SEARCH_ITER = 0x80000000        # Philox iteration words of the step-size search trials (sampling uses 0, 1, 2, ...)
_INIT_ITER = 0xFFFFFFFF          # ... and of the initial jitter
_MAX_SEARCH = 20


def _windows(num_warmup):
    """Stan's warm-up: (init buffer, [(start, end) of the slow windows]); 75 / 25-doubling / 50, or 15 % / 75 % / 10 %."""
    if num_warmup < 20:
        return num_warmup, []
    if num_warmup >= 150:
        init, term, base = 75, 50, 25
    else:
        init, term = int(0.15 * num_warmup), int(0.1 * num_warmup)
        base = num_warmup - init - term
    end, out, start, w = num_warmup - term, [], init, base
    while start < end:
        if start + 3 * w > end:
            w = end - start
        out.append((start, start + w))
        start += w
        w *= 2
    return init, out


def _parse_priors(ode_priors):
    """A prior dictionary name -> (mean, sd) (None: the reference's) -> (names in ascending ODE-index order, their bit mask, mu, sd
    as float lists) after the unknown-name and sd > 0 checks; no device is touched."""
    from models.ode_core import ODE_PARAM_NAMES
    priors = dict(REFERENCE_PRIORS if ode_priors is None else ode_priors)
    for k in priors:
        if k not in ODE_PARAM_NAMES:
            raise ValueError(f"unknown mechanistic constant {k!r}; known: {list(ODE_PARAM_NAMES)}")
    names = [n for n in ODE_PARAM_NAMES if n in priors]
    mu, sd = [float(priors[n][0]) for n in names], [float(priors[n][1]) for n in names]
    if names and not min(sd) > 0.0:
        raise ValueError("the prior sd of every constant must be > 0")
    return names, sum(1 << ODE_PARAM_NAMES.index(n) for n in names), mu, sd


def _jitter_all(s):
    """The start + 0.1 N(0, 1) on every coordinate (the chain's own normals)."""
    s.refresh(_INIT_ITER, 0.0)
    s.z[:, :s.D].add_(s.p[:, :s.D], alpha=0.1)


class _PlainTarget:
    """What a chain's D coordinates mean, for run_hmc / run_nuts: the sampled constants in prior-standardised units, then (with
    sample_nn) the P weights.  A target knows nothing of HMC or NUTS.  Its constructor is the host-side validation (no device, no
    model); `layout(s)` gives the sampler s what the chain kernels see (D, P, ode_names, ode_mask, n_ode, sample_nn, nn_names, mu,
    sd), `start(s)` its parameter buffers and -> z [C, ld], `initial_jitter(s)` moves z off the start, and `evaluate(s, A)` maps
    the first A rows of coordinates to parameters, runs the pieces and leaves gnn / gode / status / loss_sum for the chain
    kernels.  inference/population.py and inference/initial_state.py hold the other two targets."""

    def __init__(self, ode_priors=None, sample_nn=True):
        self.names, self.mask, self.mu, self.sd = _parse_priors(ode_priors)
        self.sample_nn = bool(sample_nn)
        if not self.names and not self.sample_nn:
            raise ValueError("nothing to sample: no ode_priors and sample_nn=False")

    def layout(self, s):
        f64 = dict(dtype=torch.float64, device=s.dev)
        s.P = hode.n_params(s.H, s.L)
        s.ode_names, s.ode_mask, s.n_ode, s.sample_nn = self.names, self.mask, len(self.names), self.sample_nn   # ascending ODE index = z order
        s.nn_names = [(n, tuple(p.shape)) for n, p in s.model.nn_residual.named_parameters()]
        s.D = s.n_ode + (s.P if s.sample_nn else 0)
        s.mu, s.sd = torch.tensor(self.mu or [0.0], **f64), torch.tensor(self.sd or [1.0], **f64)

    def start(self, s):
        """The chains' parameter buffers nn_p / ode_p and -> z [C, ld] at the model's own parameters."""
        from models.ode_core import ODE_PARAM_NAMES
        s.nn_p = s.nn_base.repeat(s.C).contiguous()
        s.ode_p = s.ode_base.repeat(s.C).contiguous()
        z = torch.zeros(s.C, s.ld, dtype=s.dt, device=s.dev)
        for i, n in enumerate(s.ode_names):
            z[:, i] = (float(s.ode_base[ODE_PARAM_NAMES.index(n)]) - float(s.mu[i])) / float(s.sd[i])
        if s.sample_nn:
            z[:, s.n_ode:s.D] = s.nn_base
        return z

    def initial_jitter(self, s):
        """The reference's start (mcmc.py:101-113): MLP weights + 0.01 N(0,1); sampled constants + 0.1 sd N(0,1)."""
        s.refresh(_INIT_ITER, 0.0)                    # p = xi (minv = 1): the chain's own normals
        scale = torch.full((s.ld,), 0.01, dtype=s.dt, device=s.dev)
        scale[:s.n_ode] = 0.1
        scale[s.D:] = 0
        s.z.addcmul_(s.p, scale)

    def evaluate(self, s, A):
        """Forward with tape -> hode_mse_sets (or hode_obs_nll_sets: the negative log-likelihood of the observation model) ->
        adjoint at the parameters in nn_p / ode_p, piece by piece under the tape budget."""
        _, s.gnn, s.gode = s._run_pieces(A, (False, s.sample_nn, s.n_ode > 0), x0=s.x0, ode_vec=s.ode_p, nn_flat=s.nn_p)


class _Sampler:
    """Device state of C chains and the three passes of an iteration (refresh, L leapfrog steps, accept) over a target (default:
    the _PlainTarget of ode_priors / sample_nn).  Tests drive it directly; run_hmc is the schedule around it."""

    def __init__(self, model, data, n_chains, noise_sigma=1.0, ode_priors=None, sample_nn=True, seed=0, solver="dopri5",
                 rtol=1e-6, atol=1e-8, dtype=torch.float32, jitter=0.1, noise="fixed", noise_prior=None, target=None):
        from inference.observation import ObservationModel
        from models.hybrid_ode_nn import _compute_device, _device_batch, _method
        self.om = ObservationModel(noise_sigma, noise, noise_prior)          # validates before any device is needed
        self.target = _PlainTarget(ode_priors, sample_nn) if target is None else target          # ... and so did the target
        model._check_supported()
        self.model, self.dt = model, dtype
        dev = self.dev = _compute_device()
        nl = model.nn_residual
        self.H, self.L = nl.hidden_dim, nl.hip_layers
        self.method = _method(solver)
        self.rtol, self.atol, self.seed, self.jitter = float(rtol), float(atol), int(seed) & (2 ** 64 - 1), float(jitter)
        C = self.C = int(n_chains)
        f64 = dict(dtype=torch.float64, device=dev)
        R = dict(dtype=dtype, device=dev)
        self.target.layout(self)
        self.ld = (self.D + 3) // 4 * 4
        with torch.no_grad():
            nn0, ode0 = model._params_on(dev)
        self.nn_base, self.ode_base = nn0.detach().to(dtype).contiguous(), ode0.detach().to(dtype).contiguous()
        z = self.target.start(self)
        self.z, self.p, self.g = z, torch.zeros(C, self.ld, **R), torch.zeros(C, self.ld, **R)
        self.z0, self.g0 = torch.zeros_like(z), torch.zeros_like(z)
        self.minv = torch.ones(self.ld, **R)
        self.U, self.U0, self.ke, self.ke0 = (torch.zeros(C, **f64) for _ in range(4))
        self.eps, self.log_eps = torch.zeros(C, **f64), torch.zeros(C, **f64)
        self.da = torch.zeros(C, 4, **f64)
        self.search = torch.zeros(C, 2, dtype=torch.int32, device=dev)
        self.failed = torch.zeros(C, dtype=torch.int32, device=dev)
        self.wf = torch.zeros(3, self.D, **f64)
        self.lik_scale = 0.5 / float(self.om.sigma[0]) ** 2
        self.loss_sum = torch.zeros(C, **f64)
        self.obs_kernel = False
        self.data, self.has_data = data, data is not None
        if self.has_data:
            self.x0, self.t, self.meal, self.tvns, self.gd = _device_batch(model, data, dev, dtype)
            self.N, self.T = self.x0.shape[0], self.t.shape[-1]
            if tuple(data["observations"].shape) != (self.N, self.T, 6):
                raise ValueError("observations must be [B, T, 6] on the grid of time_points")
            self.om.prepare(data["observations"], data.get("observation_mask"), dev, dtype)
            self.obs = self.om.obs
            # missing entries, per-state sigma or inferred noise: the observation kernel gives the negative log-likelihood itself
            # (lik_scale = 1).  Complete data with one fixed sigma stay on hode_mse_sets, bit for bit.
            self.obs_kernel = self.om.needs_kernel
            if self.obs_kernel:
                self.lik_scale = 1.0
                self.sse = torch.zeros(C, 6, **f64)
            self.status = torch.zeros(C, self.N, dtype=torch.int32, device=dev)
        self.gnn = self.gode = None

    # ------------------------------------------------------------------ the pieces of an iteration
    def evaluate(self, n_sets=None):
        """Likelihood sum of squares, its gradient and the solve statuses at the chains' coordinates, as the target maps them to
        parameters: of all chains, or of the first n_sets parameter sets (the NUTS driver's compacted active chains)."""
        if self.has_data:
            self.target.evaluate(self, self.C if n_sets is None else int(n_sets))

    def initial_jitter(self):
        self.target.initial_jitter(self)

    def _run_pieces(self, C, want, *, x0, ode_vec, nn_flat, max_traj=None, **run_kw):
        """loss_sum, the statuses and the gradients `want` of the first C chains over the pieces of the plan
        (models.hybrid_ode_nn._run_sets; this class supplies the cotangent of a piece).  The target names what the pieces solve:
        the x0 rows, the constants and the network vector; max_traj and run_kw go to _plan_sets and _run_sets (own_sets, own_x0)."""
        import models.hybrid_ode_nn as HN
        N = self.N
        plan = HN._plan_sets(self.dev, C, N, self.T, self.method, self.x0.element_size(), self.L, self.H, self.model.tape_steps,
                             max_traj=max_traj)
        solve = (x0, self.t, self.meal, self.tvns, self.gd, ode_vec, nn_flat, self.H, self.L, self.method, self.rtol, self.atol)
        lo, hi = plan[1][0][2:]
        self.loss_sum.zero_()
        stat = []
        cotangent = partial(self._mse_piece, stat)
        if self.obs_kernel:
            self.sse.zero_()
            flags = 0
            if self.om.marginal and hi - lo < N:
                # a set cut into pieces: its cotangent needs the sums of the WHOLE set, so the pieces run once without a tape first
                HN._run_sets(plan, partial(self._obs_piece, [], hode.capi.OBS_SUMS_ONLY), (False, False, False), *solve, **run_kw)
                flags = hode.capi.OBS_FROM_SSE
            cotangent = partial(self._obs_piece, stat, flags)
        out = HN._run_sets(plan, cotangent, want, *solve, **run_kw)
        self.status = (stat[0] if len(stat) == 1 else torch.cat(stat)).view(C, N)
        return out

    def _mse_piece(self, stat, sol, s0, s1, lo, hi):
        stat.append(sol.status)
        return hode.capi.mse_sets(sol.y.view(s1 - s0, -1), self.obs[lo:hi], self.lik_scale, self.loss_sum[s0:s1]).view_as(sol.y)

    def _obs_piece(self, stat, flags, sol, s0, s1, lo, hi):
        """The observation kernel on a piece.  OBS_SUMS_ONLY: the forward-only pass over slices of a set; OBS_FROM_SSE: their
        cotangents from the finished sums, whose nll is taken once per set."""
        stat.append(sol.status)
        ls = None if flags == hode.capi.OBS_SUMS_ONLY or (flags and lo) else self.loss_sum[s0:s1]
        gy = self.om.nll_sets(sol.y.view(s1 - s0, -1), ls, self.sse[s0:s1], lo, hi, flags)
        return None if gy is None else gy.view_as(sol.y)

    def leapfrog(self, flags, kick=0.0):
        d = self.has_data
        hode.capi.hmc_leapfrog(self.C, self.D, self.ld, flags, kick, self.eps, self.minv, self.z, self.p, self.g,
                               self.gnn if d else None, self.gode if d else None, self.P, self.loss_sum if d else None, self.lik_scale,
                               self.status if d else None, self.N if d else 0, self.U, self.ke, self.failed, self.ode_mask, self.mu,
                               self.sd, self.sample_nn, self.nn_p, self.ode_p)

    def refresh(self, it, jitter=None):
        hode.capi.hmc_refresh(self.C, self.D, self.ld, self.seed, it, self.jitter if jitter is None else jitter, self.minv, self.log_eps,
                              self.z, self.g, self.U, self.p, self.z0, self.g0, self.U0, self.ke0, self.eps, self.failed)

    def trajectory(self, n_leapfrog):
        """L leapfrog steps from (z, p) with the chains' eps: kick/2, (drift, gradient, kick) x L with the last kick halved."""
        A, K, Dr, E = hode.capi.HMC_ASSEMBLE, hode.capi.HMC_KICK, hode.capi.HMC_DRIFT, hode.capi.HMC_KE
        self.leapfrog(K | Dr, 0.5)
        for i in range(n_leapfrog):
            self.evaluate()
            last = i == n_leapfrog - 1
            self.leapfrog(A | K | (E if last else Dr), 0.5 if last else 1.0)

    def accept(self, mode, it, target_accept=0.8, draws=None, stats=None, n_slots=0, slot=-1):
        hode.capi.hmc_accept(self.C, self.D, self.ld, mode, self.seed, it, target_accept, self.z, self.z0, self.g, self.g0, self.U,
                             self.U0, self.ke0, self.ke, self.failed, self.log_eps, self.da, self.search, self.n_ode, self.mu, self.sd,
                             draws, stats, n_slots, slot)

    def gradient(self):
        """U and grad U at z (after moving z by hand): parameters -> solve -> assembly."""
        self.leapfrog(hode.capi.HMC_PARAMS)
        self.evaluate()
        self.failed.zero_()
        self.leapfrog(hode.capi.HMC_ASSEMBLE)

    def find_step_size(self, window):
        """Stan's initial step-size heuristic for every chain at once: one trial = one leapfrog step of all chains, at most
        _MAX_SEARCH trials; then dual averaging restarts from the found step (mu = log(10 eps))."""
        self.search.zero_()
        for k in range(_MAX_SEARCH):
            it = _SEARCH_ITER + 64 * window + k
            self.refresh(it, 0.0)
            self.trajectory(1)
            self.accept(hode.capi.HMC_SEARCH, it)
            if bool(self.search[:, 1].all()):
                break
        self.accept(hode.capi.HMC_DA_RESTART, 0)

    def welford(self, flags):
        hode.capi.hmc_welford(self.C, self.D, self.ld, flags, self.z, self.wf, self.minv)


# ---------------------------------------------------------------------------------------------------- diagnostics
def _split(x):
    """[M, N, ...] -> [2M, N // 2, ...] (the two halves of every chain)."""
    n = x.shape[1] // 2
    return torch.cat([x[:, :n], x[:, x.shape[1] - n:]], 0)


def _rhat(x):
    x = _split(x.double())
    n = x.shape[1]
    means = x.mean(1)
    W = x.var(1, unbiased=True).mean(0)
    B = n * means.var(0, unbiased=True)
    var_plus = (n - 1) / n * W + B / n
    return torch.sqrt(var_plus / W)


def _ess(x):
    """Multi-chain ESS of every coordinate (Geyer's initial monotone sequence, Vehtari et al. 2021), x [M, N, K]."""
    x = x.double()
    M, N = x.shape[:2]
    xc = x - x.mean(1, keepdim=True)
    f = torch.fft.rfft(xc, n=2 * N, dim=1)
    acov = torch.fft.irfft(f * f.conj(), n=2 * N, dim=1)[:, :N] / N                  # [M, N, K], biased
    mean_var = acov[:, 0].mean(0) * N / (N - 1)
    var_plus = mean_var * (N - 1) / N + (x.mean(1).var(0, unbiased=True) if M > 1 else 0)
    rho = 1.0 - (mean_var - acov.mean(0)) / var_plus                                  # [N, K]
    rho[0] = 1.0
    npair = N // 2
    Pk = rho[:2 * npair].reshape(npair, 2, -1).sum(1)                                 # [npair, K]
    keep = torch.cumprod((Pk > 0).to(torch.int64), 0).bool()                          # initial positive sequence
    Pk = torch.where(keep, Pk, torch.zeros_like(Pk))
    Pk = torch.cummin(Pk, 0).values                                                   # ... made monotone
    tau = -1.0 + 2.0 * (Pk * keep).sum(0)
    tau = torch.clamp(tau, min=1.0 / math.log10(M * N) if M * N > 10 else 1e-3)
    return M * N / tau


def _rank_normal(x):
    """Rank-normalised draws (ranks over all chains and draws, Blom's offset) for the bulk ESS."""
    M, N = x.shape[:2]
    flat = x.reshape(M * N, -1)
    r = torch.argsort(torch.argsort(flat, 0), 0).double() + 1.0
    return torch.special.ndtri((r - 0.375) / (M * N + 0.25)).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------- result
class HMCResult:
    """Draws of run_hmc.  `samples`: numpy arrays keyed like the reference's draws (`ode.<name>`, `nn.<parameter name>`),
    shaped [chains, draws, ...]; `flat()`: the same as [chains * draws, ...] (what reference posterior_summary takes);
    `stats`: accept_prob / log_posterior / divergent / failed_solve [chains, draws], step_size [chains], inv_mass [D];
    `rhat()` / `ess()`: split R-hat and multi-chain bulk ESS of every coordinate; `predict(...)`: posterior predictive;
    `noise_sigma(...)`: draws of the observation noise (inferred with noise="marginal", else the fixed values);
    `predictive_summary(...)`: the posterior predictive folded into per-entry summaries and scored (inference/predictive.py);
    `summary()`: mean / std / median / q025 / q975 / rhat / ess of every parameter (the reference's posterior_summary)."""

    def __init__(self, draws, ode_names, nn_names, stats, model=None, ode_base=None, nn_base=None, observation=None, data=None):
        self.draws = draws                          # [C, n, D] natural coordinates (device or CPU tensor)
        self.ode_names, self.nn_names = list(ode_names), list(nn_names)
        self.stats = stats
        self.model, self.ode_base, self.nn_base = model, ode_base, nn_base
        self.observation, self.data = observation, data      # the run's ObservationModel and batch (noise_sigma's defaults)
        self._samples = None

    @property
    def n_chains(self):
        return self.draws.shape[0]

    @property
    def n_draws(self):
        return self.draws.shape[1]

    @property
    def samples(self) -> Dict[str, np.ndarray]:
        if self._samples is None:
            d = self.draws.detach().cpu().numpy()
            C, n = d.shape[:2]
            out, off = {}, 0
            for name in self.ode_names:
                out[f"ode.{name}"] = d[:, :, off].copy()
                off += 1
            for name, shape in self.nn_names:
                k = int(np.prod(shape))
                if off + k > d.shape[2]:
                    break
                out[f"nn.{name}"] = d[:, :, off:off + k].reshape(C, n, *shape).copy()
                off += k
            self._samples = out
        return self._samples

    def flat(self) -> Dict[str, np.ndarray]:
        return {k: v.reshape(v.shape[0] * v.shape[1], *v.shape[2:]) for k, v in self.samples.items()}

    def rhat(self) -> torch.Tensor:
        """Split R-hat of every coordinate, [D] (fp64, on the draws' device)."""
        return _rhat(self.draws)

    def ess(self, kind="bulk") -> torch.Tensor:
        """Multi-chain ESS of every coordinate, [D], over split chains with Geyer's initial monotone sequence: "bulk" on the
        rank-normalised draws (Vehtari et al. 2021), "mean" on the draws themselves (the ESS of the posterior mean's MCSE)."""
        x = self.draws.double()
        return _ess(_split(_rank_normal(x) if kind == "bulk" else x))

    def summary(self) -> Dict[str, Dict[str, np.ndarray]]:
        """The reference's posterior_summary of all chains' draws, keyed like `samples`: {name: {mean, std, median, q025, q975,
        rhat, ess}}, each shaped like the parameter (std with ddof = 0, as np.std; the quantiles are numpy's "linear" ones; ess
        is the bulk ESS).  The quantiles come from the tail kernels over the [chains * draws, D] block (hode.capi.pred_tails /
        pred_quantiles, N = D); mean and std are fp64 on the device."""
        from inference.predictive import tail_size
        from models.hybrid_ode_nn import _compute_device
        levels = (0.025, 0.5, 0.975)
        x = self.draws.detach().to(_compute_device())
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float32)
        x = x.reshape(-1, x.shape[2]).contiguous()
        S, D = x.shape
        ts = hode.capi.pred_tail_state(D, tail_size(levels, S), x.dtype, x.device)
        hode.capi.pred_tails(x, ts)
        q, _ = hode.capi.pred_quantiles(ts, levels)
        xd = x.double()
        flat = {"mean": xd.mean(0), "std": xd.std(0, unbiased=False), "q025": q[0], "median": q[1], "q975": q[2],
                "rhat": self.rhat(), "ess": self.ess()}
        flat = {k: v.detach().double().cpu().numpy() for k, v in flat.items()}
        out, off = {}, 0
        for name in self.ode_names:
            out[f"ode.{name}"] = {k: v[off] for k, v in flat.items()}
            off += 1
        for name, shape in self.nn_names:
            k = int(np.prod(shape))
            if off + k > D:
                break
            out[f"nn.{name}"] = {key: v[off:off + k].reshape(shape) for key, v in flat.items()}
            off += k
        return out

    def _param_sets(self, thin=1):
        from models.ode_core import ODE_PARAM_NAMES
        d = self.draws[:, ::thin].reshape(-1, self.draws.shape[2]).to(torch.float32)
        S = d.shape[0]
        n_ode = len(self.ode_names)
        ode = self.ode_base.to(d.device, torch.float32).reshape(1, 17).repeat(S, 1)
        for i, n in enumerate(self.ode_names):
            ode[:, ODE_PARAM_NAMES.index(n)] = d[:, i]
        P = self.nn_base.numel()
        nn = d[:, n_ode:n_ode + P] if d.shape[1] >= n_ode + P else self.nn_base.to(d.device, torch.float32).reshape(1, P).repeat(S, 1)
        return S, nn.contiguous().reshape(-1), ode.reshape(-1).contiguous()

    def noise_sigma(self, data=None, thin=1, seed=0, solver="dopri5", rtol=1e-6, atol=1e-8):
        """Draws of the per-state observation noise sigma, [n_draws, 6] (fp64, on the compute device), one per kept draw (every
        `thin`-th of each chain).  noise="marginal": sigma_k^2 | theta, obs is inverse-gamma, drawn exactly from the sums of
        squares of the kept draws against `data` (default: the run's batch) -- ONE batched solve, the observation kernel in
        its sums-only mode, then `ObservationModel.sample_noise`; a state observed nowhere is drawn from its prior.
        noise="fixed": the fixed values repeated."""
        from inference.observation import ObservationModel
        from models.hybrid_ode_nn import _compute_device
        om = self.observation if self.observation is not None else ObservationModel()
        dev = _compute_device()
        S = self.draws[:, ::thin].shape[0] * self.draws[:, ::thin].shape[1]
        sse = torch.zeros(S, 6, dtype=torch.float64, device=dev)
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        if not om.marginal:
            return om.sample_noise(sse)
        data = self.data if data is None else data
        if data is None:
            raise ValueError("noise_sigma needs the batch the noise is inferred from")
        y = self._solve_draws(data["initial_state"], data["time_points"], data.get("external_inputs"), thin, solver, rtol, atol)
        bound = ObservationModel(om.sigma, om.noise, (om.a, om.b)).prepare(data["observations"], data.get("observation_mask"), dev,
                                                                             y.dtype)
        bound.nll_sets(y.reshape(S, -1), None, sse, flags=hode.capi.OBS_SUMS_ONLY)
        return bound.sample_noise(sse, gen)

    def predict(self, initial_state, t_span, external_inputs=None, thin=1, solver="dopri5", rtol=1e-6, atol=1e-8,
                observation_noise=False, data=None, seed=0):
        """Posterior predictive of the kept draws (every `thin`-th of each chain), ONE batched solve -> [n_draws, B, T, 6].
        observation_noise=True adds N(0, sigma_k^2) to every entry with the draws of `noise_sigma(data, thin, seed)`."""
        y = self._solve_draws(initial_state, t_span, external_inputs, thin, solver, rtol, atol)
        if observation_noise:
            sig = self.noise_sigma(data, thin, seed, solver, rtol, atol).to(y.dtype)
            gen = torch.Generator(device=y.device).manual_seed(int(seed) + 1)
            y = y + sig.view(-1, 1, 1, 6) * torch.randn(y.shape, dtype=y.dtype, device=y.device, generator=gen)
        return y.to(self.model.device)

    def predictive_summary(self, batch=None, thin=1, observation_noise=True, seed=0, n_bins=10, max_bytes=None, solver="dopri5",
                           rtol=1e-6, atol=1e-8, *, quantiles=None, loo=False, r_eff=1.0):
        """The posterior predictive of the kept draws (every `thin`-th of each chain, in `predict`'s order) on `batch` (default:
        the run's) as a `PredictiveSummary`: mean / std / PIT per entry and the scores against the batch's observations, folded
        piece by piece under max_bytes of trajectories instead of held as `predict`'s [n_draws, B, T, 6] block.
        observation_noise=True scores the predictive of the OBSERVATIONS: the draws of `noise_sigma(batch, thin, seed)` (the
        run's fixed values, or with noise="marginal" the inferred ones) enter the PIT, the log density and, by the law of total
        variance, std.  quantiles (fractions in (0, 1)): also the exact quantiles of the latent trajectories across the kept
        draws (`PredictiveSummary.quantiles`, `.band()`).  loo=True (needs observation_noise=True): also PSIS-LOO and WAIC of the
        pointwise log likelihood, `PredictiveSummary.loo`, for `inference.compare`; r_eff: the relative efficiency of the kept
        draws (1 = independent).  Serves run_hmc and run_nuts alike (both return this class)."""
        from inference import predictive as PR
        if self.model is None:
            raise ValueError("this result carries no model (built from arrays)")
        batch = self.data if batch is None else batch
        if batch is None:
            raise ValueError("predictive_summary needs a batch: the run had none")
        if loo and not observation_noise:
            raise ValueError("loo needs observation_noise=True: without observation noise there is no likelihood")
        S, nn_flat, ode_vec = self._param_sets(thin)
        sigma = self.noise_sigma(batch, thin, seed, solver, rtol, atol) if observation_noise else None
        return PR.predictive_summary(self.model, (nn_flat.view(S, -1), ode_vec.view(S, 17)), batch, sigma=sigma, n_bins=n_bins,
                                     max_bytes=PR._DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, solver=solver, rtol=rtol,
                                     atol=atol, quantiles=quantiles, loo=loo, r_eff=r_eff)

    def _solve_draws(self, initial_state, t_span, external_inputs, thin, solver, rtol, atol):
        """[n_draws, B, T, 6] on the compute device."""
        if self.model is None:
            raise ValueError("this result carries no model (built from arrays)")
        m = self.model
        S, nn_flat, ode_vec = self._param_sets(thin)
        x0 = initial_state.unsqueeze(0) if initial_state.dim() == 1 else initial_state
        B = x0.shape[0]
        rep = lambda v: None if v is None else torch.as_tensor(v).repeat(*([S] + [1] * (torch.as_tensor(v).dim() - 1)))  # noqa: E731
        t = torch.as_tensor(t_span)
        u = {k: rep(v) for k, v in (external_inputs or {}).items() if torch.as_tensor(v).dim() >= 1 and torch.as_tensor(v).numel() > 1}
        for k, v in (external_inputs or {}).items():
            if k not in u:
                u[k] = v
        with torch.no_grad():
            y = m._solve(x0.repeat(S, 1), rep(t) if t.dim() == 2 else t, u, solver, rtol, atol, n_sets=S, nn_flat=nn_flat,
                         ode_vec=ode_vec, differentiable=False)
        m._warn_failures(m.last_solve_info)
        return y.reshape(S, B, y.shape[1], 6)


# ---------------------------------------------------------------------------------------------------- entry point
def run_hmc(model, data: Optional[Dict[str, torch.Tensor]], num_samples: int = 1000, num_warmup: int = 500, n_chains: int = 64,
            n_leapfrog: int = 16, target_accept: float = 0.8, noise_sigma: float = 1.0,
            ode_priors: Optional[Dict[str, Tuple[float, float]]] = None, sample_nn: bool = True, thin: int = 1, seed: int = 0,
            solver: str = "dopri5", rtol: float = 1e-6, atol: float = 1e-8, device=None, dtype=torch.float32,
            jitter: float = 0.1, progress=None, noise: str = "fixed", noise_prior=None, initial_state=None,
            n_patients: Optional[int] = None) -> HMCResult:
    """Sample the posterior of `model` given the batch `data` (None: the prior alone) with n_chains chains.

    Observations that are NaN, or false in data["observation_mask"] (bool [B, T, 6]), are missing; a state may be observed
    nowhere.  noise_sigma: a scalar or one value per state.  noise="marginal" infers the noise instead: sigma_k^2 ~
    InvGamma(a_k, b_k) is integrated out (default a_k = 2, b_k = noise_sigma_k^2; noise_prior=(a, b) overrides) and the result's
    `noise_sigma()` draws it back (inference/observation.py).

    num_warmup iterations adapt the per-chain step size (dual averaging to target_accept) and the pooled diagonal mass matrix
    (Stan's windows); then num_samples iterations, every `thin`-th kept.  ode_priors: name -> (mean, std) of the sampled
    mechanistic constants (default: the reference's seven); sample_nn: sample every MLP weight (prior N(0, 1)).  `device` is
    accepted for run_nuts compatibility: the work runs on the HIP device.  `progress(it, stats)`, if given, is called once per
    iteration (one host synchronisation).

    initial_state: an `inference.initial_state.InitialStatePrior` makes the chosen components of every patient's initial state
    latent (sample_nn must be False; ode_priors={} samples the states alone; data=None needs n_patients) -> LatentStateResult."""
    return _run("hmc", model, data, initial_state, n_patients, ode_priors, sample_nn, n_chains=n_chains, n_leapfrog=n_leapfrog,
                num_samples=num_samples, num_warmup=num_warmup, thin=thin, target_accept=target_accept, progress=progress,
                noise_sigma=noise_sigma, seed=seed, solver=solver, rtol=rtol, atol=atol, dtype=dtype, jitter=jitter, noise=noise,
                noise_prior=noise_prior)


def _run(kind, model, data, initial_state, n_patients, ode_priors, sample_nn, **kw):
    """run_hmc (kind "hmc") and run_nuts ("nuts"): the plain target -> HMCResult, or with initial_state the latent one ->
    LatentStateResult; kw goes to _run_schedule."""
    if initial_state is None:
        s, draws, stats = _run_schedule(kind, model, data, ode_priors=ode_priors, sample_nn=sample_nn, **kw)
        return HMCResult(draws, s.ode_names, s.nn_names if s.sample_nn else [], stats, s.model, s.ode_base, s.nn_base, s.om, s.data)
    from inference.initial_state import LatentStateResult, _LatentTarget
    t = _LatentTarget(initial_state, data, n_patients, ode_priors=ode_priors, sample_nn=sample_nn)
    s, draws, stats = _run_schedule(kind, model, data, target=t, **kw)
    return LatentStateResult(draws, t.g_names, t.g_mu.cpu(), t.g_sd.cpu(), t.lat, stats, model, s.ode_base, s.nn_base, s.om, data)


def _run_schedule(kind, model, data, *, n_chains, num_samples, num_warmup, thin, target_accept, progress, n_leapfrog=16, max_tree_depth=10,
                  **sampler_kw):
    """The one driver of every entry point: the argument checks of the counts, the sampler of `kind` ("hmc": _Sampler, "nuts":
    _NutsSampler; sampler_kw holds its target and observation model), Stan's warm-up schedule and the sampling iterations around
    the kind's transition -- one iteration of all chains that adapts (warm) or records into slot `slot` of draws / stats
    [C, n_slots, n_stats] (-1: not kept).  -> (the sampler, draws, the stats dictionary); NUTS adds tree_depth, n_leapfrog and
    trajectories_solved [iterations] to it and leaf_steps to what `progress` is told."""
    nuts = kind == "nuts"
    if min(num_samples, n_chains, thin, 1 if nuts else n_leapfrog) < 1 or num_warmup < 0:
        raise ValueError(f"num_samples, n_chains, {'' if nuts else 'n_leapfrog, '}thin must be >= 1 and num_warmup >= 0")
    if not 0.0 < target_accept < 1.0:
        raise ValueError("target_accept must lie in (0, 1)")
    cap, solved = hode.capi, []
    if nuts:
        from inference.nuts import _NutsSampler
        s = _NutsSampler(model, data, n_chains, max_tree_depth, **sampler_kw)

        def transition(it, warm, slot):
            s.transition(it)
            s.finish(warm, target_accept, draws, stats, n_slots, slot)
            solved.append(s.solved)
    else:
        s = _Sampler(model, data, n_chains, **sampler_kw)

        def transition(it, warm, slot):
            s.refresh(it)
            s.trajectory(n_leapfrog)
            s.accept(cap.HMC_ADAPT if warm else cap.HMC_SAMPLE, it, target_accept, draws, stats, n_slots, slot)
    C, D = s.C, s.D
    n_slots = (num_samples + thin - 1) // thin
    draws = torch.empty(C, n_slots, D, dtype=s.dt, device=s.dev)
    stats = torch.empty(C, n_slots, 6 if nuts else 4, dtype=torch.float64, device=s.dev)
    s.initial_jitter()
    s.gradient()
    window = 0
    s.find_step_size(window)
    init, wins = _windows(num_warmup)
    ends = {b: a for a, b in wins}
    for it in range(num_warmup + num_samples):
        warm = it < num_warmup
        slot = -1
        if not warm and (it - num_warmup) % thin == 0:
            slot = (it - num_warmup) // thin
        transition(it, warm, slot)
        if warm and any(a <= it < b for a, b in wins):
            s.welford(cap.HMC_WELFORD_ACCUM)
        if warm and (it + 1) in ends:
            s.welford(cap.HMC_WELFORD_FINISH)          # new M^-1, then a new step size and a fresh dual averaging
            window += 1
            s.find_step_size(window)
        if warm and it + 1 == num_warmup:
            s.accept(cap.HMC_DA_FINISH, it)
        if progress is not None:
            progress(it, {"step_size": s.log_eps.exp().mean().item(), **({"leaf_steps": s.leaf_steps} if nuts else {})})
    st = stats.cpu().numpy()
    out = {"accept_prob": st[..., 0], "log_posterior": st[..., 1], "divergent": st[..., 2] > 0, "failed_solve": st[..., 3] > 0}
    if nuts:
        out.update(tree_depth=st[..., 4].astype(np.int64), n_leapfrog=st[..., 5].astype(np.int64))
    out.update(step_size=s.log_eps.exp().cpu().numpy(), inv_mass=s.minv[:D].double().cpu().numpy())
    if nuts:
        out["trajectories_solved"] = np.asarray(solved, dtype=np.int64)
    return s, draws, out
