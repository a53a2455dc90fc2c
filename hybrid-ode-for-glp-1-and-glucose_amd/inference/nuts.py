"""Multi-chain No-U-Turn sampling over a HybridODENN on the GPU: `run_nuts`, with the reference's entry point's leading
arguments (inference/mcmc.py:17: model, data, num_samples, num_warmup, target_accept, max_tree_depth, device).

The density, priors, coordinates, warm-up, driver (inference.hmc._run_schedule) and result are those of inference.hmc.run_hmc, and
so is the target that says what the coordinates mean; the transition is multinomial NUTS
with the generalised U-turn criterion (Hoffman & Gelman 2014; Betancourt 2017), so the trajectory length adapts per chain
and per iteration instead of a fixed n_leapfrog.  Every chain builds its tree one leaf per global step: a step is one
hode_nuts_pre, ONE taped forward solve + adjoint over the A chains whose trees are still growing (their positions ride in the
kernels' parameter-set dimension, in the slots hode_nuts_compact gave them), one hode_nuts_post and one hode_nuts_compact.
A chain whose tree has ended drops out of the solve, so an iteration costs sum_c leaves_c chain solves, not
C x max_c leaves_c.  The tree bookkeeping is csrc/hode_nuts.hip; tests/_nuts_reference.py restates it in numpy."""
from typing import Dict, Optional, Tuple

import torch

import hode
from inference.hmc import HMCResult, _run, _Sampler

__all__ = ["run_nuts"]


class _NutsSampler(_Sampler):
    """_Sampler's chains + the per-chain tree state of csrc/hode_nuts.hip.  `transition(it)` builds one tree per chain;
    `finish(...)` takes its proposal (and adapts / records).  Tests drive it directly with a fixed eps."""

    def __init__(self, model, data, n_chains, max_tree_depth=10, **kw):
        super().__init__(model, data, n_chains, **kw)
        if not 1 <= int(max_tree_depth) <= hode.capi.NUTS_MAX_DEPTH:
            raise ValueError(f"max_tree_depth must lie in [1, {hode.capi.NUTS_MAX_DEPTH}]")
        self.max_depth = int(max_tree_depth)
        C, ld, dev = self.C, self.ld, self.dev
        self.tree = torch.zeros(hode.capi.NUTS_ROWS, C, ld, dtype=self.dt, device=dev)
        self.ckpt = torch.zeros(C, self.max_depth, 2, ld, dtype=self.dt, device=dev)
        self.dst = torch.zeros(C, 8, dtype=torch.float64, device=dev)
        self.ist = torch.zeros(C, 8, dtype=torch.int32, device=dev)
        self.rank = torch.arange(C, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.solved = 0             # trajectories solved by the last transition (N x sum over leaf steps of the active chains)
        self.leaf_steps = 0         # global leaf steps of the last transition (= the most leaves of any chain)

    def transition(self, it):
        """Momentum refresh, then leaf steps until every chain's tree has ended; one host synchronisation per step (A)."""
        cap, d = hode.capi, self.has_data
        C, D, ld = self.C, self.D, self.ld
        self.refresh(it)
        cap.nuts_begin(C, D, ld, self.z, self.p, self.g, self.U, self.U0, self.ke0, self.tree, self.dst, self.ist)
        cap.nuts_compact(C, self.ist, self.rank, self.count)
        A, self.solved, self.leaf_steps = C, 0, 0
        while A > 0:
            cap.nuts_pre(C, D, ld, self.seed, it, self.eps, self.minv, self.tree, self.ist, self.rank, self.ode_mask, self.mu, self.sd,
                         self.sample_nn, self.P, self.nn_p if d else None, self.ode_p if d else None)
            self.evaluate(A)
            cap.nuts_post(C, D, ld, self.max_depth, self.seed, it, self.eps, self.minv, self.tree, self.ckpt, self.dst, self.ist, self.rank,
                          self.gnn if d else None, self.gode if d else None, self.P, self.loss_sum if d else None, self.lik_scale,
                          self.status if d else None, self.N if d else 0, self.ode_mask, self.sd, self.sample_nn)
            cap.nuts_compact(C, self.ist, self.rank, self.count)
            self.solved += A * self.N if d else 0
            self.leaf_steps += 1
            A = int(self.count.item())
            if A and self.leaf_steps >= 2 ** self.max_depth - 1:
                raise RuntimeError(f"hode_nuts: {A} trees still growing after {self.leaf_steps} leaf steps")

    def finish(self, adapt, target_accept=0.8, draws=None, stats=None, n_slots=0, slot=-1):
        hode.capi.nuts_finish(self.C, self.D, self.ld, adapt, target_accept, self.z, self.g, self.U, self.tree, self.dst, self.ist,
                              self.log_eps, self.da, self.n_ode, self.mu, self.sd, draws, stats, n_slots, slot)


def run_nuts(model, data: Optional[Dict[str, torch.Tensor]], num_samples: int = 1000, num_warmup: int = 500,
             target_accept: float = 0.8, max_tree_depth: int = 10, device=None, *, n_chains: int = 64, noise_sigma: float = 1.0,
             ode_priors: Optional[Dict[str, Tuple[float, float]]] = None, sample_nn: bool = True, thin: int = 1, seed: int = 0,
             solver: str = "dopri5", rtol: float = 1e-6, atol: float = 1e-8, dtype=torch.float32, jitter: float = 0.1,
             progress=None, noise: str = "fixed", noise_prior=None, initial_state=None, n_patients: Optional[int] = None) -> HMCResult:
    """Sample the posterior of `model` given the batch `data` (None: the prior alone) with n_chains chains of NUTS.

    The target, priors, observation model (missing observations, noise_sigma per state, noise="marginal" / noise_prior) and
    warm-up are run_hmc's: num_warmup iterations adapt the per-chain step size (dual averaging of the
    tree's accept statistic to target_accept) and the pooled diagonal mass matrix (Stan's windows); then num_samples
    iterations, every `thin`-th kept.  Each tree doubles at most max_tree_depth times.  `device` is accepted for the
    reference's signature: the work runs on the HIP device.  `progress(it, stats)`, if given, is called once per iteration.

    The result's stats add tree_depth and n_leapfrog [chains, draws] (int) to run_hmc's, accept_prob is the tree's accept
    statistic, and trajectories_solved [iterations] counts the solves of every sampling and warm-up iteration.

    initial_state: an `inference.initial_state.InitialStatePrior`, as in run_hmc -> LatentStateResult."""
    return _run("nuts", model, data, initial_state, n_patients, ode_priors, sample_nn, n_chains=n_chains, max_tree_depth=max_tree_depth,
                num_samples=num_samples, num_warmup=num_warmup, thin=thin, target_accept=target_accept, progress=progress,
                noise_sigma=noise_sigma, seed=seed, solver=solver, rtol=rtol, atol=atol, dtype=dtype, jitter=jitter, noise=noise,
                noise_prior=noise_prior)
