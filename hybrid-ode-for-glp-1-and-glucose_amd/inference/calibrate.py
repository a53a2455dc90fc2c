"""Per-patient calibration of a HybridODENN's mechanistic constants: `fit_patients`, a batched Levenberg-Marquardt fit of every
patient's own constants (and optionally initial states) to that patient's record, with a Laplace approximation at the fit.

The reference's manuscript reports "online updating for per-subject adaptation" and calls the model "minimal, identifiable";
both need the Jacobian of a trajectory with respect to a handful of constants.  Here it comes from the tangent-linear pass over
the forward's tape (hode.solve_jvp): exact for the discrete scheme, K directions for about the cost of K forward solves.

Objective of patient b (independent across patients), in fit coordinates z (theta = c + s z):
    F_b(z) = 1/2 sum_{t,i observed} ((y_b(t)_i - obs_b(t)_i) / sigma_i)^2  +  1/2 sum_{k with a prior} z_k^2
With a prior (mu, sd) on coordinate k: c = mu, s = sd, so F is the negative log posterior (MAP).  Without one: c = 0,
s = the starting value (z = theta / theta_init; 1 when that is 0) and no penalty (least squares).  NaN observations are
missing (sparse CGM, glucose-only records).

One LM iteration = one taped solve over all patients + one JVP with K directions + one trial solve; the damped normal equations
are batched fp64 linear algebra on [B, K, K]; damping, acceptance and convergence are per patient.  The LM core
(`levenberg_marquardt`) is pure torch around a residual-and-Jacobian callback."""
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

import hode

from .hmc import REFERENCE_PRIORS

__all__ = ["fit_patients", "CalibrationResult", "levenberg_marquardt"]

ST_CONVERGED, ST_MAX_ITER, ST_SOLVE_FAILED = 0, 1, 2


def levenberg_marquardt(fn: Callable, z0: torch.Tensor, prior_w: torch.Tensor, max_iter: int = 50, lam0: float = 1e-3,
                        gtol: float = 1e-14, xtol: float = 1e-10):
    """Batched, per-patient Levenberg-Marquardt on F_b(z) = 1/2 |r_b(z)|^2 + 1/2 sum_k prior_w[k] z_k^2.

    fn(z [B,K], want_jac) -> (r [B,M], J [B,M,K] or None, ok [B] bool): whitened residuals, their Jacobian d r / d z (when
    want_jac) and whether the model could be evaluated for the patient.  Every iteration calls fn(z, True) once at the current
    point and fn(z_trial, False) once.  Damping: Marquardt's, lam diag(A) with a floor, updated by Nielsen's gain-ratio rule.  A patient stops with status 0 when
    |grad|_inf <= gtol |grad at start|_inf, when the undamped Gauss-Newton step is below xtol (xtol + |z|), or when no damping
    makes progress any more (lam > 1e16) with that step below 1e-7 (1 + |z|) (F cannot resolve it); status 1 when max_iter
    steps were taken or progress stopped further out; status 2 when fn fails at its current point.
    Returns dict(z, F, A = J^T J + diag(prior_w) at the final point, JtJ, status, n_iter); all per patient."""
    z = z0.detach().clone()
    B, K = z.shape
    dev, dt = z.device, z.dtype
    pw = prior_w.to(device=dev, dtype=dt).reshape(1, K)
    lam = torch.full((B,), float(lam0), dtype=dt, device=dev)
    nu = torch.full((B,), 2.0, dtype=dt, device=dev)
    status = torch.full((B,), ST_MAX_ITER, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    n_iter = torch.zeros(B, dtype=torch.int32, device=dev)
    tiny = torch.finfo(dt).tiny
    g0 = None
    eye = torch.eye(K, dtype=dt, device=dev)

    def objective(r, zz):
        return 0.5 * _tree_sum(r * r) + 0.5 * _tree_sum(pw * zz * zz)

    for it in range(max_iter + 1):
        r, J, ok = fn(z, True)
        bad = ~ok & ~done
        status[bad] = ST_SOLVE_FAILED
        done |= bad
        J = torch.where(ok.reshape(B, 1, 1), J, torch.zeros((), dtype=dt, device=dev))
        r = torch.where(ok.reshape(B, 1), r, torch.zeros((), dtype=dt, device=dev))
        F = objective(r, z)
        JtJ = _tree_sum(J.unsqueeze(3) * J.unsqueeze(2))
        A = JtJ + torch.diag_embed(pw.expand(B, K))
        g = _tree_sum(J * r.unsqueeze(2)) + pw * z
        gn = g.abs().amax(1)
        if g0 is None:
            g0 = gn.clone()
        dg = torch.diagonal(A, dim1=1, dim2=2)
        dg = dg.clamp_min(1e-12 * dg.amax(1, keepdim=True) + tiny)
        # the undamped (Gauss-Newton) step: below xtol the patient sits at its minimum to the precision of its own conditioning
        # (a gradient test alone stops an ill-conditioned patient early along its weakest direction)
        ok_a = torch.isfinite(A).flatten(1).all(1)
        A_gn = torch.where(ok_a.reshape(B, 1, 1), A + 1e-14 * torch.diag_embed(dg), eye)
        step_gn = torch.linalg.solve(A_gn, torch.where(ok_a.reshape(B, 1), g, torch.zeros((), dtype=dt, device=dev)))
        norm = lambda v: _tree_sum(v * v).sqrt()            # noqa: E731
        near = ok_a & (norm(step_gn) <= xtol * (xtol + norm(z)))
        conv = ~done & ((gn <= gtol * g0.clamp_min(tiny)) | near)
        status[conv] = ST_CONVERGED
        done |= conv
        if it == max_iter or bool(done.all()):
            break
        M = A + lam.reshape(B, 1, 1) * torch.diag_embed(dg)
        M = torch.where(done.reshape(B, 1, 1), eye, M)                  # (patients that stopped: a harmless identity system)
        delta = -torch.linalg.solve(M, torch.where(done.reshape(B, 1), torch.zeros((), dtype=dt, device=dev), g))
        z_try = z + delta
        r_t, _, ok_t = fn(z_try, False)
        F_t = objective(r_t, z_try)
        moving = ~done
        acc = moving & ok_t & torch.isfinite(F_t) & (F_t < F)
        n_iter += moving.to(torch.int32)
        z = torch.where(acc.reshape(B, 1), z_try, z)
        # gain ratio: actual over predicted decrease of the quadratic model, -g.delta - 1/2 delta.A.delta
        pred = -_tree_sum(g * delta) - 0.5 * _tree_sum(delta * _tree_sum((A * delta.unsqueeze(1)).transpose(1, 2)))
        rho = (F - F_t) / pred.clamp_min(tiny)
        shrink = torch.clamp(1.0 - (2.0 * rho - 1.0) ** 3, min=1.0 / 3.0)
        lam = torch.where(acc, (lam * shrink).clamp_min(1e-12), torch.where(moving, lam * nu, lam))
        nu = torch.where(acc, torch.full_like(nu, 2.0), torch.where(moving, nu * 2.0, nu))
        # no damping makes progress any more: stop.  Converged when the Gauss-Newton step is below the resolution of F itself
        # (a decrease of 1/2 step.A.step under one rounding of F cannot be seen), status 1 otherwise
        stuck = moving & ~acc & (lam > 1e16)
        status[stuck & ok_a & (norm(step_gn) <= 1e-7 * (1.0 + norm(z)))] = ST_CONVERGED
        done |= stuck
    return dict(z=z, F=F, A=A, JtJ=JtJ, status=status, n_iter=n_iter)


def _tree_sum(x):
    """Sum over dim 1 in a fixed pairwise order made of elementwise additions: a patient's bits do not depend on who else is in the
    batch (a batched GEMM or a library reduction may pick its summation order by the batch size, and fifty LM steps of an
    ill-conditioned patient carry that last bit into the eighth digit of the fit)."""
    while x.shape[1] > 1:
        h = x.shape[1] // 2
        y = x[:, :h] + x[:, h:2 * h]
        x = torch.cat([y, x[:, 2 * h:]], 1) if x.shape[1] > 2 * h else y
    return x[:, 0]


def _finite_rows(A):
    """[B] patients whose K x K matrix is finite, and the batch with every other matrix replaced by the identity (a patient
    whose fit diverged must not make the batched LAPACK call fail for the others)."""
    ok = torch.isfinite(A).flatten(1).all(1)
    eye = torch.eye(A.shape[-1], dtype=A.dtype, device=A.device)
    return ok, torch.where(ok.reshape(-1, 1, 1), A, eye)


def laplace_covariance(A: torch.Tensor, prior_w: torch.Tensor) -> torch.Tensor:
    """A^-1 (pseudo-inverse when some coordinate has no prior: J^T J may be singular for an unidentifiable constant), per
    patient on the host's LAPACK (K x K, once per fit); NaN for a patient whose A is not finite."""
    ok, Ah = _finite_rows(A.detach().cpu())
    inv = torch.linalg.inv(Ah) if bool((prior_w > 0).all()) else torch.linalg.pinv(Ah, hermitian=True)
    return torch.where(ok.reshape(-1, 1, 1), inv, torch.full((), float("nan"), dtype=inv.dtype)).to(A.device)


def fisher_eigvals(JtJ: torch.Tensor) -> torch.Tensor:
    """Ascending eigenvalues of each J^T W J (host LAPACK, each matrix scaled to unit norm first); NaN where not finite."""
    ok, Mh = _finite_rows(JtJ.detach().cpu())
    sc = Mh.abs().amax((1, 2), keepdim=True).clamp_min(torch.finfo(Mh.dtype).tiny)
    ev = torch.linalg.eigvalsh(Mh / sc) * sc.reshape(-1, 1)
    return torch.where(ok.reshape(-1, 1), ev, torch.full((), float("nan"), dtype=ev.dtype)).to(JtJ.device)


@dataclass
class CalibrationResult:
    """fit_patients' result.  `params`: name -> [B] in natural units (ODE constant names, `x0:<state>` for initial states);
    `cov` [B,K,K] the Laplace covariance in natural units (`std`, `corr` from it); `fim_eigvals` [B,K] the eigenvalues of the
    Fisher information J^T W J in fit coordinates (prior-standardised, or relative to the starting value without a prior),
    ascending; `status` [B] 0 converged, 1 max_iter reached, 2 the solve failed at the fit; `n_iter` [B] LM steps taken;
    `objective` [B] the final F_b (module docstring)."""
    names: Tuple[str, ...]
    params: Dict[str, torch.Tensor]
    z: torch.Tensor
    cov: torch.Tensor
    std: torch.Tensor
    corr: torch.Tensor
    fim_eigvals: torch.Tensor
    status: torch.Tensor
    n_iter: torch.Tensor
    objective: torch.Tensor
    _predict: Optional[Callable] = field(default=None, repr=False)

    def predict(self, t_span=None, external_inputs=None, initial_state=None) -> torch.Tensor:
        """Trajectories [B,T,6] of every patient with its fitted constants (and fitted initial states), by default on the
        batch's own grid and inputs."""
        return self._predict(t_span, external_inputs, initial_state)


class _PatientSolver:
    """The batch on the device, once: per-patient constants ride in the kernels' parameter-set dimension (n_sets = B, one
    network copy per patient, as HMC runs its chains)."""

    def __init__(self, model, batch, names, dtype, solver, rtol, atol, max_steps):
        from models.hybrid_ode_nn import STATE_NAMES, _compute_device, _device_batch, _method, _taped_steps
        from models.ode_core import ODE_PARAM_NAMES
        model._check_supported()
        self.dev = dev = _compute_device()
        self.dt = dtype
        self.x0, self.t, self.meal, self.tvns, self.gd = _device_batch(model, batch, dev, dtype)
        self.B, self.T = self.x0.shape[0], self.t.shape[-1]
        nl = model.nn_residual
        self.H, self.L = nl.hidden_dim, nl.hip_layers
        self.method = _method(solver)
        self.rtol, self.atol = float(rtol), float(atol)
        with torch.no_grad():
            nn_flat, ode_vec = model._params_on(dev)
        self.nn = nn_flat.detach().to(dtype).repeat(self.B).contiguous()
        self.ode_base = ode_vec.detach().to(dtype).contiguous()
        self.cols = []                        # ("ode", index) / ("x0", index) per fit coordinate
        for n in names:
            if n.startswith("x0:"):
                if n[3:] not in STATE_NAMES:
                    raise ValueError(f"unknown state {n[3:]!r}; known: {list(STATE_NAMES)}")
                self.cols.append(("x0", STATE_NAMES.index(n[3:])))
            else:
                if n not in ODE_PARAM_NAMES:
                    raise ValueError(f"unknown mechanistic constant {n!r}; known: {list(ODE_PARAM_NAMES)}")
                self.cols.append(("ode", ODE_PARAM_NAMES.index(n)))
        K = len(self.cols)
        self.v_ode = torch.zeros(self.B, K, 17, dtype=dtype, device=dev)
        self.v_x0 = torch.zeros(self.B, K, 6, dtype=dtype, device=dev)
        for k, (kind, j) in enumerate(self.cols):
            (self.v_ode if kind == "ode" else self.v_x0)[:, k, j] = 1.0
        self.has_ode = any(c[0] == "ode" for c in self.cols)
        self.has_x0 = any(c[0] == "x0" for c in self.cols)
        self.max_steps = int(max_steps) if max_steps is not None else _taped_steps(
            self.B, self.T, self.method, self.x0.element_size(), self.L, self.H, model.tape_steps)
        self.tape = None

    def theta0(self):
        """[B,K] the starting values: the model's constants, the batch's initial states."""
        return torch.stack([self.ode_base[j].expand(self.B) if kind == "ode" else self.x0[:, j] for kind, j in self.cols], 1)

    def solve(self, theta, want_jac, x0=None, t=None, ins=None):
        B = self.B
        ode = self.ode_base.reshape(1, 17).repeat(B, 1)
        xs = (self.x0 if x0 is None else x0.to(self.dev, self.dt)).clone()
        for k, (kind, j) in enumerate(self.cols):
            if kind == "ode":
                ode[:, j] = theta[:, k]
            else:
                xs[:, j] = theta[:, k]
        meal, tvns, gd = (self.meal, self.tvns, self.gd) if ins is None else ins
        sol = hode.solve_fwd(xs.contiguous(), self.t if t is None else t, meal, tvns, gd, ode.reshape(-1).contiguous(), self.nn,
                             self.H, self.L, method=self.method, rtol=self.rtol, atol=self.atol, max_steps=self.max_steps,
                             n_sets=B, want_tape=want_jac and self.tape is None, tape=self.tape if want_jac else None)
        if want_jac:
            self.tape = sol.tape
            S = hode.solve_jvp(sol, self.v_ode if self.has_ode else None, self.v_x0 if self.has_x0 else None)
            return sol, S
        return sol, None


def fit_patients(model, batch: Dict[str, torch.Tensor], params: Sequence[str] = tuple(REFERENCE_PRIORS),
                 fit_initial: Sequence[str] = (), noise_sigma=0.1, priors: Optional[Dict[str, Tuple[float, float]]] = REFERENCE_PRIORS,
                 max_iter: int = 50, solver: str = "dopri5", rtol: float = 1e-6, atol: float = 1e-8, dtype=torch.float64,
                 init: Optional[Dict[str, torch.Tensor]] = None, max_steps: Optional[int] = None, lam0: float = 1e-3,
                 gtol: float = 1e-14, xtol: float = 1e-10) -> CalibrationResult:
    """Fit every patient's own mechanistic constants `params` (and initial states `fit_initial`, state names such as "GLP1")
    to that patient's observations: an independent MAP fit per patient under `priors` (name -> (mu, sd); initial states as
    "x0:<state>"), or least squares with priors=None.

    batch: the dict run_hmc takes -- initial_state [B,6], observations [B,T,6] (NaN = missing), time_points [T] or [B,T],
    external_inputs (optional).  noise_sigma: a scalar or one value per state.  The fit starts at the model's constants and the
    batch's initial states (`init`: name -> scalar or [B] overrides).  Everything else of the model (the network, the other
    constants) is held fixed.  See the module docstring for the objective and CalibrationResult for what is returned."""
    names = tuple(params) + tuple(f"x0:{s}" for s in fit_initial)
    if not names:
        raise ValueError("fit_patients needs at least one constant or initial state to fit")
    ps = _PatientSolver(model, batch, names, dtype, solver, rtol, atol, max_steps)
    dev, B, K, T = ps.dev, ps.B, len(names), ps.T
    obs = torch.as_tensor(batch["observations"]).to(dev, dtype).reshape(B, T, 6)
    mask = torch.isfinite(obs)
    obs0 = torch.where(mask, obs, torch.zeros((), dtype=dtype, device=dev))
    sig = torch.as_tensor(noise_sigma, dtype=dtype).to(dev).reshape(-1)
    if sig.numel() not in (1, 6) or not bool((sig > 0).all()):
        raise ValueError("noise_sigma must be positive: a scalar or one value per state")
    w = (1.0 / sig).expand(6)
    theta0 = ps.theta0()
    for n, v in (init or {}).items():
        theta0[:, names.index(n)] = torch.as_tensor(v, dtype=dtype).to(dev).reshape(-1).expand(B)
    pri = priors or {}
    has = torch.tensor([n in pri for n in names], device=dev)
    mu = torch.tensor([float(pri[n][0]) if n in pri else 0.0 for n in names], dtype=dtype, device=dev).expand(B, K)
    sd = torch.tensor([float(pri[n][1]) if n in pri else 1.0 for n in names], dtype=dtype, device=dev).expand(B, K)
    rel = torch.where(theta0 != 0, theta0, torch.ones((), dtype=dtype, device=dev))
    c = torch.where(has, mu, torch.zeros((), dtype=dtype, device=dev))
    s = torch.where(has, sd, rel)
    prior_w = has.to(dtype)

    def fn(z, want_jac):
        sol, S = ps.solve(c + s * z, want_jac)
        ok = sol.status == 0
        r = torch.where(mask, (sol.y - obs0) * w, torch.zeros((), dtype=dtype, device=dev)).reshape(B, -1)
        J = None
        if want_jac:
            Sw = torch.where(mask.unsqueeze(1), S * w, torch.zeros((), dtype=dtype, device=dev))
            J = Sw.reshape(B, K, -1).transpose(1, 2) * s.unsqueeze(1)
        return r, J, ok

    out = levenberg_marquardt(fn, (theta0 - c) / s, prior_w, max_iter=max_iter, lam0=lam0, gtol=gtol, xtol=xtol)
    z = out["z"]
    theta = c + s * z
    cov_z = laplace_covariance(out["A"], prior_w)
    cov = s.unsqueeze(2) * cov_z * s.unsqueeze(1)
    std = torch.diagonal(cov, dim1=1, dim2=2).clamp_min(0).sqrt()
    corr = cov / (std.unsqueeze(2) * std.unsqueeze(1)).clamp_min(torch.finfo(dtype).tiny)
    fim = fisher_eigvals(out["JtJ"])

    def predict(t_span=None, external_inputs=None, initial_state=None):
        t = ps.t if t_span is None else torch.as_tensor(t_span).to(dev, dtype).contiguous()
        ins = None
        if external_inputs is not None:
            _, _, u = model._prep_inputs(torch.zeros(B, 6), t, external_inputs, dev)
            ins = tuple(None if u[k] is None else u[k].to(dtype).contiguous() for k in ("meal", "tVNS", "GD"))
        x0 = None if initial_state is None else torch.as_tensor(initial_state)
        with torch.no_grad():
            sol, _ = ps.solve(theta, False, x0=x0, t=t, ins=ins)
        return sol.y

    return CalibrationResult(names=names, params={n: theta[:, k] for k, n in enumerate(names)}, z=z, cov=cov, std=std, corr=corr,
                             fim_eigvals=fim, status=out["status"], n_iter=out["n_iter"], objective=out["F"], _predict=predict)
