"""The observation model shared by the samplers and the training-side likelihood: missing observations, per-state noise, and
noise scales that are inferred instead of supplied (csrc/hode_obs.hip; include/hode.h, "Observation model").

Observations obs[N, T, 6] on the solve's grid.  Entry (i, t, k) is OBSERVED when it is finite and, with an
`observation_mask` (bool [N, T, 6]), when the mask is true there; a masked entry may hold anything, NaN included.
n_k = the number of observed entries of state k over the batch, SSE_k(theta) = the sum of (y - obs)^2 over them.

    noise="fixed"      -log p(obs | theta) = sum_k SSE_k / (2 sigma_k^2) + const;  noise_sigma a scalar or one value per state
    noise="marginal"   sigma_k^2 ~ InvGamma(a_k, b_k) integrated out:
                       -log p(obs | theta) = sum_{n_k > 0} (a_k + n_k / 2) log(b_k + SSE_k / 2) + const
                       default a_k = 2, b_k = noise_sigma_k^2 (prior mean of sigma_k^2 = noise_sigma_k^2); noise_prior=(a, b)
                       overrides it.  Afterwards sigma_k^2 | theta, obs ~ InvGamma(a_k + n_k / 2, b_k + SSE_k / 2) exactly:
                       `sample_noise` draws it from the sums of the kept theta draws, no sampler coordinate is spent on it.

`log_norm()` is the constant: log p(obs | theta) = -(nll + log_norm())."""
import math

import numpy as np
import torch

import hode

__all__ = ["ObservationModel"]

_MODES = ("fixed", "marginal")


def _six(v, what):
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 6)
    if a.size != 6 or not np.all(np.isfinite(a)) or not np.all(a > 0):
        raise ValueError(f"{what} must be positive: a scalar or one value per state")
    return a


class ObservationModel:
    """ObservationModel(noise_sigma=1.0, noise="fixed" | "marginal", noise_prior=None); `prepare(observations, mask, device,
    dtype)` binds it to a batch (device copies of obs and mask, the counts n_k), after which `nll_sets` runs the kernel."""

    def __init__(self, noise_sigma=1.0, noise="fixed", noise_prior=None):
        if noise not in _MODES:
            raise ValueError(f"noise must be one of {_MODES}, not {noise!r}")
        self.sigma = _six(noise_sigma, "noise_sigma")
        self.scalar_sigma = bool(np.all(self.sigma == self.sigma[0]))
        self.marginal = noise == "marginal"
        self.noise = noise
        if noise_prior is not None:
            if not self.marginal:
                raise ValueError('noise_prior needs noise="marginal"')
            if len(noise_prior) != 2:
                raise ValueError("noise_prior must be (a, b): the shape and scale of the inverse-gamma prior of sigma^2")
            self.a, self.b = _six(noise_prior[0], "noise_prior a"), _six(noise_prior[1], "noise_prior b")
        else:
            self.a, self.b = np.full(6, 2.0), self.sigma ** 2
        self.w = 1.0 / self.sigma ** 2
        self.obs = self.mask = self.n = self._src = None
        self.complete = None

    # ------------------------------------------------------------------ binding to a batch
    def prepare(self, observations, mask=None, device=None, dtype=None):
        """Bind to observations [N, T, 6] (+ an optional bool mask of the same shape): obs as [N, T*6] in `dtype` on `device`,
        the mask as uint8 [N, T*6] (None when every entry is observed), n_k.  Returns self."""
        if self.obs is not None and self._src[0] is observations and self._src[1] is mask and self._src[2:] == (device, dtype):
            return self                                    # the same batch again (a training loop): nothing to count
        obs = torch.as_tensor(observations)
        if obs.dim() != 3 or obs.shape[2] != 6:
            raise ValueError("observations must be [B, T, 6] on the grid of time_points")
        dev = obs.device if device is None else torch.device(device)
        obs = obs.to(dev, obs.dtype if dtype is None else dtype)
        seen = torch.isfinite(obs)
        if mask is not None:
            m = torch.as_tensor(mask).to(dev)
            if m.shape != obs.shape:
                raise ValueError("observation_mask must have the shape of observations")
            seen = seen & m.bool()
        n = seen.sum((0, 1)).cpu().numpy().astype(np.float64)          # counted once: it depends on the data only
        if n.sum() == 0:
            raise ValueError("no observed entry: every observation is missing or masked")
        self.n, self._src = n, (observations, mask, device, dtype)
        self.complete = bool(n.sum() == obs.numel())
        self.shape = tuple(obs.shape)
        self.obs = obs.reshape(obs.shape[0], -1).contiguous()
        self.mask = None if self.complete else seen.reshape(obs.shape[0], -1).to(torch.uint8).contiguous()
        return self

    @property
    def needs_kernel(self):
        """False when the plain sum of squares (hode_mse_sets with one scale) is the whole likelihood."""
        return self.marginal or not self.scalar_sigma or not self.complete

    def nll_sets(self, y, loss_sum, sse, lo=0, hi=None, flags=0, want_grad=True):
        """-log p(obs[lo:hi] | y) up to log_norm() for every set of y [n_sets, (hi - lo) * T * 6], through the kernel: sse
        fp64[n_sets, 6] and loss_sum fp64[n_sets] (or None) are ACCUMULATED; returns the cotangent gy (or None)."""
        if self.obs is None:
            raise RuntimeError("ObservationModel.prepare(observations, ...) first")
        hi = self.obs.shape[0] if hi is None else hi
        kw = dict(a=self.a, b=self.b, n=self.n) if self.marginal else dict(w=self.w)
        return hode.capi.obs_nll_sets(y, self.obs[lo:hi], None if self.mask is None else self.mask[lo:hi],
                                      hode.capi.OBS_MARGINAL if self.marginal else hode.capi.OBS_FIXED, sse, loss_sum, flags=flags,
                                      want_grad=want_grad, **kw)

    # ------------------------------------------------------------------ the noise given theta
    def posterior_params(self, sse):
        """(shape, scale) [..., 6] of sigma_k^2 | theta, obs ~ InvGamma for sums sse [..., 6] (marginal mode)."""
        dev = sse.device
        a = torch.as_tensor(self.a + 0.5 * self.n, dtype=torch.float64, device=dev)
        b = torch.as_tensor(self.b, dtype=torch.float64, device=dev) + 0.5 * sse.double()
        return a.expand_as(b), b

    def sample_noise(self, sse, generator=None):
        """One draw of sigma [..., 6] per row of sse [..., 6] (on sse's device): marginal mode draws sigma_k^2 from its
        inverse-gamma posterior (from the prior for a state with n_k = 0, whose sum is 0); fixed mode repeats noise_sigma."""
        if not self.marginal:
            return torch.as_tensor(self.sigma, dtype=torch.float64, device=sse.device).expand(sse.shape).clone()
        if self.n is None:
            raise RuntimeError("ObservationModel.prepare(observations, ...) first")
        a, b = self.posterior_params(sse)
        gam = torch._standard_gamma(a.contiguous(), generator=generator)          # sigma^2 = b / Gamma(a, 1)
        return torch.sqrt(b / gam)

    def log_norm(self):
        """The theta-independent part of -log p(obs | theta): log p = -(nll + log_norm())."""
        if self.n is None:
            raise RuntimeError("ObservationModel.prepare(observations, ...) first")
        n = self.n
        if not self.marginal:
            return float(np.sum(n * (np.log(self.sigma) + 0.5 * math.log(2 * math.pi))))
        on = n > 0
        a, b = self.a[on], self.b[on]
        lg = np.vectorize(math.lgamma)
        return float(np.sum(0.5 * n[on] * math.log(2 * math.pi) - a * np.log(b) + lg(a) - lg(a + 0.5 * n[on])))


class _ObsNllFn(torch.autograd.Function):
    """nll(y) of one parameter set through the kernel: forward keeps the cotangent, backward scales it."""

    @staticmethod
    def forward(ctx, y, om):
        sse = torch.zeros(1, 6, dtype=torch.float64, device=y.device)
        loss = torch.zeros(1, dtype=torch.float64, device=y.device)
        gy = om.nll_sets(y.detach().reshape(1, -1), loss, sse, want_grad=ctx.needs_input_grad[0])
        ctx.gy = None if gy is None else gy.view_as(y)
        ctx.sse = sse
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gy, ctx.gy = ctx.gy, None
        return (gy * g.to(gy.dtype)), None
