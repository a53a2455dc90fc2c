"""ctypes binding of the C ABI declared in include/hode.h.  Tensors in, tensors out (device memory
owned by torch's allocator, work enqueued on torch's current stream)."""
import ctypes as C
import os

import torch

from ._abi import EXT_SYMBOLS, SYMBOLS, HodeError, bind  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("HODE_LIB") or os.path.join(_HERE, "libhode.so")   # HODE_LIB: development builds
_lib = None
_fns = {}                                     # (family, dtype or None) -> the declared ctypes function

METHOD_DP54 = 0
METHOD_RK4 = 1

ST_OK, ST_MAXSTEPS, ST_UNDERFLOW, ST_NONFINITE = 0, 1, 2, 3
_ERR = {-1: "HODE_EINVAL (bad argument)", -2: "HODE_EUNSUPPORTED (shape outside the supported range: H<=128, L<=8, activation code <= 3)",
        -3: "HODE_ELAUNCH (HIP launch failed)"}

INPUT_KEYS = ("meal", "tVNS", "GD")


def lib_path():
    return _SO


def load():
    """Load libhode.so.  Raises (loudly) when it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise HodeError(f"{_SO} not found: build it with `python __graft_entry__.py` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback for the hot path")
        if not os.environ.get("HODE_LIB") and not os.environ.get("HODE_ALLOW_STALE"):
            from . import _build
            if not _build.is_current():
                raise HodeError(f"{_SO} was not built from the kernel sources next to it (binary {_build.binary_stamp()}, sources "
                                f"{_build.source_stamp()}): rebuild with `python __graft_entry__.py` (or `make -C {_build.CSRC}`); "
                                "HODE_ALLOW_STALE=1 loads it anyway")
        if os.environ.get("HODE_LIB") and not os.environ.get("HODE_ALLOW_STALE") and os.path.exists(_SO + ".srcsha"):
            # a development library that carries a source stamp (make lab writes one) must have been built from THESE sources:
            # the bitwise lab-versus-product tests would otherwise compare against last week's kernels without saying so
            from . import _build
            want = _build.lab_source_stamp()
            if want is not None and os.path.abspath(_SO) == os.path.abspath(_build.LAB_SO) and _build.binary_stamp(_SO) != want:
                raise HodeError(f"{_SO} is stale (binary {_build.binary_stamp(_SO)}, sources {want}): `make -C {_build.CSRC} lab`; "
                                "HODE_ALLOW_STALE=1 loads it anyway")
        lib = C.CDLL(_SO)
        _fns.update(bind(lib, _SO))            # restype and argtypes of every symbol of include/hode.h
        _lib = lib
    return _lib


def version():
    return load().hode_version().decode()


ACT_RELU, ACT_TANH, ACT_ELU, ACT_LEAKY_RELU = 0, 1, 2, 3
NN_SHARED = 1 << 16          # HODE_LAYERS_NN_SHARED (hode_solve_fwd_* only)


def layers(L, act=ACT_RELU):
    """The `L` argument of the C ABI: hidden layers in bits 0..7, activation code in bits 8..15 (include/hode.h HODE_LAYERS)."""
    return (L & 0xff) | (act << 8)


def n_params(H, L):
    L &= 0xff                                  # (L may carry an activation code)
    return 9 * H + H + (L - 1) * (H * H + H) + 6 * H + 6


def _check(rc, what):
    if rc != 0:
        raise HodeError(f"{what} failed: {_ERR.get(rc, rc)}")


def _need_gpu(t):
    if not t.is_cuda:
        raise HodeError("hode kernels need tensors on a HIP device (no CPU fallback)")


def _ptr(t):
    """For raw calls of a library function by hand (tests do): the wrappers below pass tensors as they are."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, dtype, *args):
    """Enqueue hode_<name>_f32 / _f64 (by dtype; None: the one symbol hode_<name>) on torch's current stream.  Arguments are plain
    values -- ints, floats, tensors, None, host arrays -- marshalled and dtype-checked by the argtypes of hode/_abi.py."""
    try:
        fn = _fns[name, dtype]
    except KeyError:                            # the library is not loaded yet, or there is no such instantiation
        if _lib is not None:
            raise HodeError(f"unsupported dtype {dtype}") from None
        load()
        return _call(name, dtype, *args)
    try:
        rc = fn(_stream(), *args)
    except C.ArgumentError as e:                # ctypes relabels what a parameter's from_param raised: give it its type back
        raise (HodeError if "HodeError" in str(e) else TypeError)(f"hode_{name}: {e}") from None
    if rc != 0:
        _check(rc, f"hode_{name}")


def _need_real(dtype):
    if dtype not in (torch.float32, torch.float64):
        raise HodeError(f"unsupported dtype {dtype}")


def _prep(t, dtype, dev):
    return None if t is None else t.to(device=dev, dtype=dtype).contiguous()


def _mode(t, B, T):
    """models/hybrid_ode_nn.py:217-231: dim()==2 time varying [B,T]; dim()==1 constant [B]."""
    if t is None:
        return 0
    if t.dim() == 2:
        if tuple(t.shape) != (B, T):
            raise HodeError(f"time-varying input must be [B,T]=({B},{T}), got {tuple(t.shape)}")
        return 2
    if tuple(t.shape) != (B,):
        raise HodeError(f"constant input must be [B]=({B},), got {tuple(t.shape)}")
    return 1


def selftest_xlane(device="cuda"):
    out = torch.zeros(64 * 12, dtype=torch.int32, device=device)
    _call("selftest_xlane", None, out)
    return out.view(64, 12)


def rhs_fwd(x, t, meal, tvns, gd, ode_p, nn_p, H, L):
    _need_gpu(x)
    dt, dev = x.dtype, x.device
    x = x.contiguous()
    B = x.shape[0]
    t, meal, tvns, gd = (_prep(v, dt, dev) for v in (t, meal, tvns, gd))
    ode_p, nn_p = _prep(ode_p, dt, dev), _prep(nn_p, dt, dev)
    assert nn_p.numel() == n_params(H, L) and ode_p.numel() == 17
    out = torch.empty(B, 6, dtype=dt, device=dev)
    _call("rhs_fwd", dt, B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, out)
    return out


class Solve:
    """Result of solve_fwd: trajectories + per-trajectory diagnostics (+ tape for the adjoint)."""
    __slots__ = ("y", "status", "nsteps", "nfev", "tape", "max_steps", "ctx")


def tape_nbytes(B, max_steps, elem_size, L, H=64):
    return load().hode_tape_bytes_hl(B, max_steps, elem_size, H, L)


def solve_fwd(x0, t, meal, tvns, gd, ode_p, nn_p, H, L, method=METHOD_DP54, rtol=1e-6, atol=1e-8,
              max_steps=None, n_sets=1, want_tape=False, tape=None, nn_shared=False):
    """Forward solve.  want_tape=True records what the adjoint needs; pass `tape=` (a uint8 tensor of at least
    tape_nbytes(...) bytes, e.g. the `.tape` of an earlier solution of the same shape) to reuse the buffer
    instead of allocating several GB per call.
    nn_shared=True: `nn_p` is ONE network used by all n_sets sets of ODE constants (HODE_LAYERS_NN_SHARED; forward only)."""
    _need_gpu(x0)
    dt, dev = x0.dtype, x0.device
    x0 = x0.contiguous()
    B = x0.shape[0]
    t = _prep(t, dt, dev)
    T = t.shape[-1]
    t_batched = int(t.dim() == 2)
    if t_batched and t.shape[0] != B:
        raise HodeError("batched time grid must be [B,T]")
    meal, tvns, gd = (_prep(v, dt, dev) for v in (meal, tvns, gd))
    ode_p, nn_p = _prep(ode_p, dt, dev), _prep(nn_p, dt, dev)
    if nn_p.numel() != (1 if nn_shared else n_sets) * n_params(H, L) or ode_p.numel() != 17 * n_sets:
        raise HodeError("parameter vector size does not match (H, L, n_sets)")
    if nn_shared and (want_tape or tape is not None):
        raise HodeError("nn_shared is a forward-only option (the adjoint returns one gradient row per parameter set)")
    if max_steps is None:
        # accepted-step budget per trajectory.  With a tape every step costs 6*(L+1)*256 B of HBM (stage
        # tape), so the default is tighter there; a trajectory that needs more reports status 1.
        if method == METHOD_RK4:
            max_steps = max(T - 1, 1)
        elif want_tape or tape is not None:
            max_steps = (T - 1) + max(32, (T - 1) // 4)
        else:
            max_steps = 8 * (T - 1) + 64
    s = Solve()
    s.y = torch.empty(B, T, 6, dtype=dt, device=dev)
    s.status = torch.empty(B, dtype=torch.int32, device=dev)
    s.nsteps = torch.empty(B, dtype=torch.int32, device=dev)
    s.nfev = torch.empty(B, dtype=torch.int32, device=dev)
    s.max_steps = max_steps
    s.tape = None
    if want_tape or tape is not None:
        nbytes = load().hode_tape_bytes_hl(B, max_steps, x0.element_size(), H, L)
        if tape is not None:
            if tape.dtype != torch.uint8 or not tape.is_cuda or tape.numel() < nbytes or tape.data_ptr() % 256:
                raise HodeError(f"tape buffer must be a 256-byte aligned uint8 device tensor of >= {nbytes} bytes")
            s.tape = tape
        else:
            s.tape = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call("solve_fwd", dt, B, T, x0, t, t_batched, meal, _mode(meal, B, T), tvns, _mode(tvns, B, T), gd, _mode(gd, B, T), ode_p, nn_p,
          n_sets, H, L | (NN_SHARED if nn_shared else 0), method, rtol, atol, max_steps, s.y, s.status, s.nsteps, s.nfev, s.tape)
    s.ctx = (t, t_batched, meal, tvns, gd, ode_p, nn_p, n_sets, H, L, method)
    return s


def solve_bwd(sol, gy, want_gnn=True, want_gode=False):
    """Reverse-time discrete adjoint over the tape of `sol` (made with want_tape=True).
    Returns (gx0[B,6], gnn[n_sets*P] or None, gode[n_sets*17] or None)."""
    return _solve_bwd(sol, gy, want_gnn, want_gode, None)[:3]


def solve_bwd_inputs(sol, gy, want_gnn=True, want_gode=False, want_inputs=INPUT_KEYS):
    """solve_bwd() + the gradients of the external inputs (hode_solve_bwd_inputs_*, include/hode.h).
    Returns (gx0, gnn, gode, {"meal", "tVNS", "GD"}): an entry is None for an input the solve did not have or that is not in
    `want_inputs`, else a tensor shaped like the input ([B] constant, [B,T] on the grid)."""
    return _solve_bwd(sol, gy, want_gnn, want_gode, tuple(want_inputs))


def _solve_bwd(sol, gy, want_gnn, want_gode, want_inputs):
    if sol.tape is None:
        raise HodeError("solve_bwd needs a solution computed with want_tape=True")
    t, t_batched, meal, tvns, gd, ode_p, nn_p, n_sets, H, L, method = sol.ctx
    dt, dev = sol.y.dtype, sol.y.device
    B, T = sol.y.shape[:2]
    gy = gy.to(device=dev, dtype=dt).contiguous()
    if tuple(gy.shape) != (B, T, 6):
        raise HodeError("gy must be [B,T,6]")
    gx0 = torch.empty(B, 6, dtype=dt, device=dev)
    gnn = torch.zeros(nn_p.numel(), dtype=dt, device=dev) if want_gnn else None
    gode = torch.zeros(17 * n_sets, dtype=dt, device=dev) if want_gode else None
    args = _taped_args(sol) + (sol.tape, gy, gx0, gnn, gode)
    if want_inputs is None:
        _call("solve_bwd", dt, *args)
        return gx0, gnn, gode, None
    gin = {k: (torch.empty_like(u) if (u is not None and k in want_inputs) else None)
           for k, u in zip(INPUT_KEYS, (meal, tvns, gd))}
    _call("solve_bwd_inputs", dt, *args, *(gin[k] for k in INPUT_KEYS))
    return gx0, gnn, gode, gin


def _taped_args(sol):
    """The arguments that hode_solve_bwd_*, hode_solve_bwd_inputs_* and hode_solve_jvp*_ share: the solve, up to its tape."""
    t, t_batched, meal, tvns, gd, ode_p, nn_p, n_sets, H, L, method = sol.ctx
    B, T = sol.y.shape[:2]
    return (B, T, t, t_batched, meal, _mode(meal, B, T), tvns, _mode(tvns, B, T), gd, _mode(gd, B, T), ode_p, nn_p, n_sets, H, L,
            method, sol.max_steps, sol.nsteps, sol.status)


def solve_jvp(sol, v_ode=None, v_x0=None):
    """Tangent-linear pass over the tape of `sol` (made with want_tape=True; hode_solve_jvp_any_*, include/hode.h: every network
    solve_fwd can tape -- the tuned shapes through the kernel of hode_solve_jvp_*, every other through the generic one).
    v_ode [n_sets,K,17] (directions in the ODE constants of each parameter set) and/or v_x0 [B,K,6] (in the initial states).
    Returns dy[B,K,T,6] = (dy/d ode_p) v_ode + (dy/d x0) v_x0 -- the exact derivative of the discrete scheme the forward ran."""
    if sol.tape is None:
        raise HodeError("solve_jvp needs a solution computed with want_tape=True")
    if v_ode is None and v_x0 is None:
        raise HodeError("solve_jvp needs v_ode and/or v_x0")
    t, t_batched, meal, tvns, gd, ode_p, nn_p, n_sets, H, L, method = sol.ctx
    dt, dev = sol.y.dtype, sol.y.device
    B, T = sol.y.shape[:2]
    v_ode, v_x0 = _prep(v_ode, dt, dev), _prep(v_x0, dt, dev)
    ref = v_ode if v_ode is not None else v_x0
    if ref.dim() != 3:
        raise HodeError("directions must be [n_sets,K,17] / [B,K,6]")
    K = ref.shape[1]
    if v_ode is not None and tuple(v_ode.shape) != (n_sets, K, 17):
        raise HodeError(f"v_ode must be [n_sets,K,17]=({n_sets},K,17), got {tuple(v_ode.shape)}")
    if v_x0 is not None and tuple(v_x0.shape) != (B, K, 6):
        raise HodeError(f"v_x0 must be [B,K,6]=({B},K,6), got {tuple(v_x0.shape)}")
    dy = torch.empty(B, K, T, 6, dtype=dt, device=dev)
    _call("solve_jvp_any", dt, *_taped_args(sol), sol.tape, K, v_ode, v_x0, dy)
    return dy


def rhs_bwd(x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, want_gt=False, want_gnn=True, want_gode=False):
    return _rhs_bwd(x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, want_gt, want_gnn, want_gode, None)[:4]


def rhs_bwd_inputs(x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, want_gt=False, want_gnn=True, want_gode=False,
                   want_inputs=INPUT_KEYS):
    """rhs_bwd() + the gradients of the external inputs (hode_rhs_bwd_inputs_*): returns (gx, gt, gnn, gode,
    {"meal", "tVNS", "GD"}), an entry [B] for an input that is given and wanted, else None."""
    return _rhs_bwd(x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, want_gt, want_gnn, want_gode, tuple(want_inputs))


def _rhs_bwd(x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, want_gt, want_gnn, want_gode, want_inputs):
    _need_gpu(x)
    dt, dev = x.dtype, x.device
    x = x.contiguous()
    B = x.shape[0]
    t, meal, tvns, gd, gout = (_prep(v, dt, dev) for v in (t, meal, tvns, gd, gout))
    ode_p, nn_p = _prep(ode_p, dt, dev), _prep(nn_p, dt, dev)
    gx = torch.empty(B, 6, dtype=dt, device=dev)
    gt = torch.empty(B, dtype=dt, device=dev) if want_gt else None
    gnn = torch.zeros(nn_p.numel(), dtype=dt, device=dev) if want_gnn else None
    gode = torch.zeros(17, dtype=dt, device=dev) if want_gode else None
    args = (B, x, t, meal, tvns, gd, ode_p, nn_p, H, L, gout, gx, gt, gnn, gode)
    if want_inputs is None:
        _call("rhs_bwd", dt, *args)
        return gx, gt, gnn, gode, None
    gin = {k: (torch.empty(B, dtype=dt, device=dev) if (u is not None and k in want_inputs) else None)
           for k, u in zip(INPUT_KEYS, (meal, tvns, gd))}
    _call("rhs_bwd_inputs", dt, *args, *(gin[k] for k in INPUT_KEYS))
    return gx, gt, gnn, gode, gin


def adam_step(p, g, m, v, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, max_norm=0.0, grad_scale=1.0,
              weight_decay=0.0, scratch=None):
    """In-place fused clip + Adam on flat fp32 vectors (train/train_hybrid.py:255-261)."""
    for a in (p, g, m, v):
        _need_gpu(a)
        if a.dtype != torch.float32 or not a.is_contiguous():
            raise HodeError("adam_step needs contiguous fp32 tensors")
    if scratch is None:
        scratch = torch.empty(2, dtype=torch.float32, device=p.device)
    _call("adam_step_f32", None, p.numel(), p, g, m, v, lr, beta1, beta2, eps, step, max_norm, grad_scale, weight_decay, scratch)
    return scratch


def mse_fwd_bwd(y, obs, scale, loss_sum=None, want_grad=True):
    """sum((y-obs)^2) accumulated into loss_sum (fp64[1]) and gy = 2*scale*(y-obs) in one pass."""
    _need_gpu(y)
    y = y.contiguous()
    obs = obs.to(device=y.device, dtype=torch.float32).contiguous()
    if y.dtype != torch.float32 or y.shape != obs.shape:
        raise HodeError("mse_fwd_bwd needs fp32 tensors of equal shape")
    if loss_sum is None:
        loss_sum = torch.zeros(1, dtype=torch.float64, device=y.device)
    gy = torch.empty_like(y) if want_grad else None
    _call("mse_fwd_bwd_f32", None, y.numel(), y, obs, scale, loss_sum, gy)
    return loss_sum, gy


# --------------------------------------------------------------------------------------------- MCMC (include/hode.h "MCMC")
HMC_ASSEMBLE, HMC_KICK, HMC_DRIFT, HMC_KE, HMC_PARAMS = 1, 2, 4, 8, 16
HMC_SAMPLE, HMC_ADAPT, HMC_SEARCH, HMC_DA_RESTART, HMC_DA_FINISH = 0, 1, 2, 3, 4
HMC_WELFORD_ACCUM, HMC_WELFORD_FINISH = 1, 2


def mse_sets(y, obs, scale, loss_sum, want_grad=True):
    """Per-set sum of squares: y[n_sets, ...] against ONE obs shared by every set (obs.numel() = the per-set length);
    loss_sum fp64[n_sets] ACCUMULATED, returns gy = 2*scale*(y-obs) (or None)."""
    _need_gpu(y)
    y = y.contiguous()
    n_sets = y.shape[0]
    obs = obs.to(device=y.device, dtype=y.dtype).contiguous()
    if y.numel() != n_sets * obs.numel() or loss_sum.dtype != torch.float64 or loss_sum.numel() < n_sets:
        raise HodeError("mse_sets: y must be [n_sets, len(obs)] and loss_sum fp64[n_sets]")
    gy = torch.empty_like(y) if want_grad else None
    _call("mse_sets", y.dtype, n_sets, obs.numel(), y, obs, scale, loss_sum, gy)
    return gy


OBS_FIXED, OBS_MARGINAL = 0, 1
OBS_SUMS_ONLY, OBS_FROM_SSE = 1, 2


def _six(v):
    return None if v is None else (C.c_double * 6)(*[float(x) for x in v])


def obs_nll_sets(y, obs, mask, mode, sse, loss_sum=None, w=None, a=None, b=None, n=None, flags=0, want_grad=True):
    """The observation model's negative log-likelihood per set (include/hode.h "Observation model"): y[n_sets, ...] against ONE
    obs shared by every set; mask uint8 like obs or None; mode OBS_FIXED (w = 1/sigma^2 per state) or OBS_MARGINAL (a, b, n per
    state), six host floats each; sse fp64[n_sets, 6] and loss_sum fp64[n_sets] (or None) ACCUMULATED; flags 0 / OBS_SUMS_ONLY /
    OBS_FROM_SSE.  Returns gy (None with want_grad=False or OBS_SUMS_ONLY)."""
    _need_gpu(y)
    y = y.contiguous()
    n_sets = y.shape[0]
    obs = obs.to(device=y.device, dtype=y.dtype).contiguous()
    if y.numel() != n_sets * obs.numel() or sse.dtype != torch.float64 or sse.numel() < 6 * n_sets or not sse.is_contiguous():
        raise HodeError("obs_nll_sets: y must be [n_sets, len(obs)] and sse fp64[n_sets, 6]")
    if loss_sum is not None and (loss_sum.dtype != torch.float64 or loss_sum.numel() < n_sets):
        raise HodeError("obs_nll_sets: loss_sum must be fp64[n_sets]")
    if mask is not None:
        mask = mask.to(device=y.device).contiguous()
        if mask.dtype != torch.uint8 or mask.numel() != obs.numel():
            raise HodeError("obs_nll_sets: mask must be uint8 with the shape of obs")
    gy = torch.empty_like(y) if want_grad and flags != OBS_SUMS_ONLY else None
    _call("obs_nll_sets", y.dtype, n_sets, obs.numel(), y, obs, mask, mode, flags, _six(w), _six(a), _six(b), _six(n), sse, loss_sum, gy)
    return gy


SOBOL_MAX_D = 32


def sobol_indices(Y, D, second_order=True, R=100, seed=0, conf_z=1.959963984540054):
    """Sobol indices of the outputs of a Saltelli design (include/hode.h "Sobol indices"): Y [N * nb, M] on the device, fp32 or
    fp64, nb = 2 D + 2 with second_order and D + 2 without, row i * nb + b = block b (A, AB_1..AB_D, [BA_1..BA_D,] B) of base
    sample i; the rows may be strided (Y.stride(0) >= M, unit stride along the columns), so a slice of columns goes in as it is.
    R bootstrap resamples (Philox stream 7 of `seed`), conf = conf_z * their ddof-1 standard deviation.  Returns a dict of fp64
    device tensors: S1, ST, S1_conf, ST_conf [M, D]; S2, S2_conf [M, D, D] (None without second_order; NaN off the pairs
    j < k); variance [M].  The conf entries are NaN for R < 2."""
    _need_gpu(Y)
    if Y.dim() != 2 or Y.shape[1] < 1:
        raise HodeError("sobol_indices: Y must be [rows, M] with M >= 1")
    if Y.stride(1) != 1 or Y.stride(0) < Y.shape[1]:
        Y = Y.contiguous()
    nb = 2 * D + 2 if second_order else D + 2
    rows, M = Y.shape
    if D > SOBOL_MAX_D:
        raise HodeError(f"sobol_indices: D = {D} parameters, the kernel takes up to {SOBOL_MAX_D} (HODE_SOBOL_MAX_D)")
    if D < 1 or rows < nb or rows % nb:
        raise HodeError(f"sobol_indices: {rows} rows are not a positive multiple of the {nb} blocks of a design in D = {D}")
    dev = Y.device
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)                     # noqa: E731
    out = {"S1": new(M, D), "ST": new(M, D), "S2": new(M, D, D) if second_order else None,
           "S1_conf": new(M, D), "ST_conf": new(M, D), "S2_conf": new(M, D, D) if second_order else None, "variance": new(M)}
    _call("sobol_indices", Y.dtype, rows // nb, D, M, Y, Y.stride(0), int(bool(second_order)), int(R), int(seed), conf_z,
          out["S1"], out["ST"], out["S2"], out["S1_conf"], out["ST_conf"], out["S2_conf"], out["variance"])
    return out


PF_MAX_PARTICLES, PF_MAX_AUX, PF_COLS = 4096, 17, 16
PF_LINK = {"additive": 0, "log": 1}
PF_STATS = ("log_evidence", "ess", "resampled", "alive")          # stats columns 0..3; 4..9 the means, 10..15 the variances


def _need_vectors(what, dev, dtype, named):
    for name, v, n in named:
        if v.dtype != dtype or v.device != dev or v.numel() != n or not v.is_contiguous():
            raise HodeError(f"{what}: {name} must be a contiguous {'fp64' if dtype == torch.float64 else 'int32'} device tensor of "
                            f"{n} elements")


def _obs_mask_status(what, obs, mask, status, B, n, n_name, dev, dtype):
    obs = obs.to(device=dev, dtype=dtype).contiguous()
    if obs.numel() != 6 * B:
        raise HodeError(f"{what}: obs must be [B, 6]")
    if mask is not None:
        mask = mask.to(device=dev).contiguous()
        if mask.dtype != torch.uint8 or mask.numel() != 6 * B:
            raise HodeError(f"{what}: mask must be uint8 [B, 6]")
    if status is not None:
        status = status.to(device=dev).contiguous()
        if status.dtype != torch.int32 or status.numel() != B * n:
            raise HodeError(f"{what}: status must be int32 [B, {n_name}]")
    return obs, mask, status


def _is_buffer(t, dtype, dev, shape=None, numel=None):
    return (t.dtype == dtype and t.device == dev and t.is_contiguous()
            and (tuple(t.shape) == tuple(shape) if numel is None else t.numel() == numel))


def pf_step(x_in, obs, sigma, q, dt, lw, step, seed=0, id0=0, link=1, ess_frac=0.5, status=None, mask=None, aux_in=None, out=None):
    """One step of the bootstrap particle filter (include/hode.h "Particle filter"): x_in [B, N, 6] fp32 or fp64 on the device,
    obs [B, 6] (NaN = missing), mask uint8 [B, 6] or None, sigma / q fp64 [6] and dt fp64 [B] on the device, lw fp64 [B, N]
    UPDATED IN PLACE, status int32 [B, N] or None, aux_in [B, N, n_aux] (n_aux <= 17) or None: a payload gathered with the particle.
    `out`: (x_out, anc, stats, aux_out) buffers to write into (a loop reuses them), else they are allocated.
    Returns (x_out [B, N, 6], anc int32 [B, N], stats fp64 [B, 16], aux_out or None)."""
    _need_gpu(x_in)
    if x_in.dim() != 3 or x_in.shape[2] != 6 or not x_in.is_contiguous():
        raise HodeError("pf_step: x_in must be a contiguous [B, N, 6]")
    B, N = int(x_in.shape[0]), int(x_in.shape[1])
    dev, dt_ = x_in.device, x_in.dtype
    if N > PF_MAX_PARTICLES:
        raise HodeError(f"pf_step: N = {N} particles, the kernel takes up to {PF_MAX_PARTICLES} (HODE_PF_MAX_PARTICLES)")
    obs, mask, status = _obs_mask_status("pf_step", obs, mask, status, B, N, "N", dev, dt_)
    _need_vectors("pf_step", dev, torch.float64, (("sigma", sigma, 6), ("q", q, 6), ("dt", dt, B), ("lw", lw, B * N)))
    n_aux = 0
    if aux_in is not None:
        if aux_in.dim() != 3 or tuple(aux_in.shape[:2]) != (B, N) or aux_in.dtype != dt_ or aux_in.device != dev or not aux_in.is_contiguous():
            raise HodeError("pf_step: aux_in must be a contiguous [B, N, n_aux] of x_in's dtype")
        n_aux = int(aux_in.shape[2])
    if out is None:
        out = (torch.empty_like(x_in), torch.empty(B, N, dtype=torch.int32, device=dev),
               torch.empty(B, PF_COLS, dtype=torch.float64, device=dev), None if aux_in is None else torch.empty_like(aux_in))
    x_out, anc, stats, aux_out = out
    _call("pf_step", dt_, B, N, int(step), int(seed), int(id0), x_in, status, obs, mask, sigma, q, dt, int(link), float(ess_frac), lw,
          x_out, anc, stats, n_aux, aux_in, aux_out)
    return x_out, anc, stats, aux_out


def pf_smooth(hist, lwh, pred, q, dt, M, seed=0, id0=0, link=1, out=None):
    """Backward-simulation smoothing over a stored filter (include/hode.h "Particle smoother"): hist / pred [S, B, N, 6] fp32 or
    fp64 on the device (the particles after each step, and the state each was carried to before the noise), lwh fp64 [S, B, N],
    q fp64 [6], dt fp64 [S, B]; M trajectories per patient.  `out`: (idx, paths) buffers to write into, else they are allocated.
    Returns (idx int32 [S, B, M], paths [S, B, M, 6])."""
    _need_gpu(hist)
    if hist.dim() != 4 or hist.shape[3] != 6 or not hist.is_contiguous():
        raise HodeError("pf_smooth: hist must be a contiguous [S, B, N, 6]")
    S, B, N = (int(v) for v in hist.shape[:3])
    dev, dt_ = hist.device, hist.dtype
    M = int(M)
    if M < 1:
        raise HodeError("pf_smooth: M must be at least 1")
    if N > PF_MAX_PARTICLES:
        raise HodeError(f"pf_smooth: N = {N} particles, the kernel takes up to {PF_MAX_PARTICLES} (HODE_PF_MAX_PARTICLES)")
    if pred.shape != hist.shape or pred.dtype != dt_ or pred.device != dev or not pred.is_contiguous():
        raise HodeError("pf_smooth: pred must be a contiguous [S, B, N, 6] of hist's dtype")
    _need_vectors("pf_smooth", dev, torch.float64, (("lwh", lwh, S * B * N), ("q", q, 6), ("dt", dt, S * B)))
    if out is None:
        out = (torch.empty(S, B, M, dtype=torch.int32, device=dev), torch.empty(S, B, M, 6, dtype=dt_, device=dev))
    idx, paths = out
    if not (_is_buffer(idx, torch.int32, dev, (S, B, M)) and _is_buffer(paths, dt_, dev, (S, B, M, 6))):
        raise HodeError("pf_smooth: out must be (idx int32 [S, B, M], paths [S, B, M, 6] of hist's dtype), contiguous")
    _call("pf_smooth", dt_, B, N, M, S, int(seed), int(id0), hist, lwh, pred, q, dt, int(link), idx, paths)
    return idx, paths


PF_MOVE = {"carried": 0, "identity": 1, "log": 2}


def pf_params(lw, aux, mode, walk, dt, step, shrink, seed=0, id0=0, out=None):
    """The parameter move of the particle filter (include/hode.h "Particle filter: parameter move"), after a pf_step: lw fp64
    [B, N] as the step left it (read only), aux [B, N, n_aux] fp32 or fp64 (1 <= n_aux <= 17) MOVED IN PLACE, mode int32 [n_aux]
    (PF_MOVE: 0 carried, 1 identity link, 2 log link), walk fp64 [n_aux] and dt fp64 [B], all on the device; shrink in [0, 1].
    `out`: a pstats buffer to write into (a loop reuses it), else it is allocated.
    Returns pstats fp64 [B, 2 * n_aux]: (mean, variance) in link space of every selected column before the move, NaN otherwise."""
    _need_gpu(aux)
    if aux.dim() != 3 or not aux.is_contiguous() or not 1 <= aux.shape[2] <= PF_MAX_AUX:
        raise HodeError(f"pf_params: aux must be a contiguous [B, N, n_aux] with 1 <= n_aux <= {PF_MAX_AUX}")
    B, N, n_aux = (int(v) for v in aux.shape)
    dev = aux.device
    if N > PF_MAX_PARTICLES:
        raise HodeError(f"pf_params: N = {N} particles, the kernel takes up to {PF_MAX_PARTICLES} (HODE_PF_MAX_PARTICLES)")
    _need_vectors("pf_params", dev, torch.float64, (("lw", lw, B * N), ("walk", walk, n_aux), ("dt", dt, B)))
    _need_vectors("pf_params", dev, torch.int32, (("mode", mode, n_aux),))
    shrink = float(shrink)
    if not 0.0 <= shrink <= 1.0:
        raise HodeError("pf_params: shrink must lie in [0, 1]")
    if out is None:
        out = torch.empty(B, 2 * n_aux, dtype=torch.float64, device=dev)
    if not _is_buffer(out, torch.float64, dev, numel=2 * B * n_aux):
        raise HodeError("pf_params: out must be a contiguous fp64 [B, 2 * n_aux] on aux's device")
    _call("pf_params", aux.dtype, B, N, int(step), int(seed), int(id0), lw, n_aux, aux, mode, walk, dt, shrink, out)
    return out


UKF_COLS = 16
UKF_STATS = ("log_evidence", "nis", "n_seen", "alive")            # stats columns 0..3; 4..9 the means, 10..15 the variances


def ukf_weights(n, alpha=1.0, beta=0.0, kappa=1.0):
    """(gamma, wm0, wc0, wi) of the scaled unscented transform in n dimensions: lambda = alpha^2 (n + kappa) - n,
    gamma = sqrt(n + lambda), the centre point's weights wm0 = lambda / (n + lambda) for the mean and wc0 = wm0 + 1 - alpha^2 + beta
    for the covariance, every other point's wi = 1 / (2 (n + lambda))."""
    n, alpha, beta, kappa = int(n), float(alpha), float(beta), float(kappa)
    lam = alpha * alpha * (n + kappa) - n
    if not n + lam > 0.0:
        raise HodeError(f"ukf_weights: n + lambda = {n + lam} must be positive (alpha = {alpha}, kappa = {kappa}, n = {n})")
    wm0 = lam / (n + lam)
    return (n + lam) ** 0.5, wm0, wm0 + 1.0 - alpha * alpha + beta, 1.0 / (2.0 * (n + lam))


def ukf_step(x_in, aux_in, mode, obs, sigma, q, walk, dt, alive, mean, cov, weights, predict=True, link=1, status=None, mask=None,
             out=None):
    """One step of the unscented Kalman filter (include/hode.h "Unscented Kalman filter"): x_in [B, K, 6] fp32 or fp64 on the
    device and aux_in [B, K, 17] of its dtype (the solve's output rows and the ode_p rows they were solved with), K = 2 (6 + P) + 1;
    mode: 17 ints on the HOST (PF_MOVE: 0 carried, 1 identity link, 2 log link), P of them non-zero; obs [B, 6] (NaN = missing),
    mask uint8 [B, 6] or None, status int32 [B, K] or None; sigma / q fp64 [6], walk fp64 [17], dt fp64 [B] on the device;
    alive int32 [B], mean fp64 [B, n] and cov fp64 [B, n, n] UPDATED IN PLACE (mean and cov are read only with predict=False);
    weights = (gamma, wm0, wc0, wi), e.g. ukf_weights(n).  `out`: (x_out, aux_out, stats) buffers to write into (a loop reuses
    them), else they are allocated.  Returns (x_out [B, K, 6], aux_out [B, K, 17], stats fp64 [B, 16])."""
    _need_gpu(x_in)
    mode = [int(v) for v in (mode.tolist() if hasattr(mode, "tolist") else mode)]
    if len(mode) != PF_MAX_AUX or any(v not in (0, 1, 2) for v in mode):
        raise HodeError(f"ukf_step: mode must be {PF_MAX_AUX} host integers in 0..2 (PF_MOVE)")
    n = 6 + sum(1 for v in mode if v)
    K = 2 * n + 1
    if x_in.dim() != 3 or tuple(x_in.shape[1:]) != (K, 6) or not x_in.is_contiguous():
        raise HodeError(f"ukf_step: x_in must be a contiguous [B, K, 6] with K = 2 (6 + P) + 1 = {K}")
    B = int(x_in.shape[0])
    dev, dt_ = x_in.device, x_in.dtype
    if tuple(aux_in.shape) != (B, K, PF_MAX_AUX) or aux_in.dtype != dt_ or aux_in.device != dev or not aux_in.is_contiguous():
        raise HodeError(f"ukf_step: aux_in must be a contiguous [B, K, {PF_MAX_AUX}] of x_in's dtype")
    obs, mask, status = _obs_mask_status("ukf_step", obs, mask, status, B, K, "K", dev, dt_)
    _need_vectors("ukf_step", dev, torch.float64, (("sigma", sigma, 6), ("q", q, 6), ("walk", walk, PF_MAX_AUX), ("dt", dt, B),
                                                   ("mean", mean, B * n), ("cov", cov, B * n * n)))
    _need_vectors("ukf_step", dev, torch.int32, (("alive", alive, B),))
    gamma, wm0, wc0, wi = (float(v) for v in weights)
    if out is None:
        out = (torch.empty_like(x_in), torch.empty_like(aux_in), torch.empty(B, UKF_COLS, dtype=torch.float64, device=dev))
    x_out, aux_out, stats = out
    if not (_is_buffer(x_out, dt_, dev, x_in.shape) and _is_buffer(aux_out, dt_, dev, aux_in.shape)
            and _is_buffer(stats, torch.float64, dev, numel=B * UKF_COLS)):
        raise HodeError("ukf_step: out must be (x_out like x_in, aux_out like aux_in, stats fp64 [B, 16]), contiguous")
    if x_out.data_ptr() == x_in.data_ptr() or aux_out.data_ptr() == aux_in.data_ptr():
        raise HodeError("ukf_step: x_out may not alias x_in, aux_out may not alias aux_in")
    _call("ukf_step", dt_, B, 1 if predict else 0, int(link), (C.c_int32 * PF_MAX_AUX)(*mode), gamma, wm0, wc0, wi, x_in, status, aux_in,
          obs, mask, sigma, q, walk, dt, alive, mean, cov, x_out, aux_out, stats)
    return x_out, aux_out, stats


def ukf_smooth(history, ode_history, propagated, mean, cov, alive, mode, q, walk, dt, weights, link=1, out=None):
    """The unscented RTS smoother over a stored filter (include/hode_ukf_smooth.h): history / propagated [S, B, K, 6]
    fp32 or fp64 on the device (the points every step emitted, and the rows every step was handed) and ode_history [S, B, K, 17] of
    their dtype; mean fp64 [S, B, n], cov fp64 [S, B, n, n] and alive int32 [S, B] after every step; mode: 17 ints on the HOST
    (PF_MOVE), K = 2 n + 1 with n = 6 + the non-zero ones; q fp64 [6], walk fp64 [17], dt fp64 [S, B] on the device;
    weights = (gamma, wm0, wc0, wi).  `out`: the six buffers to write into, else they are allocated.
    Returns (mean_s [S, B, n], cov_s [S, B, n, n], gain [S-1, B, n, n], pred_mean [S-1, B, n], pred_cov [S-1, B, n, n],
    moments [S, B, 12]), all fp64."""
    _need_gpu(history)
    mode = [int(v) for v in (mode.tolist() if hasattr(mode, "tolist") else mode)]
    if len(mode) != PF_MAX_AUX or any(v not in (0, 1, 2) for v in mode):
        raise HodeError(f"ukf_smooth: mode must be {PF_MAX_AUX} host integers in 0..2 (PF_MOVE)")
    n = 6 + sum(1 for v in mode if v)
    K = 2 * n + 1
    if history.dim() != 4 or tuple(history.shape[2:]) != (K, 6) or not history.is_contiguous():
        raise HodeError(f"ukf_smooth: history must be a contiguous [S, B, K, 6] with K = 2 (6 + P) + 1 = {K}")
    S, B = int(history.shape[0]), int(history.shape[1])
    dev, dt_ = history.device, history.dtype
    if S < 1 or B < 1:
        raise HodeError("ukf_smooth: history must hold at least one step of at least one patient")
    if propagated.shape != history.shape or propagated.dtype != dt_ or propagated.device != dev or not propagated.is_contiguous():
        raise HodeError("ukf_smooth: propagated must be a contiguous [S, B, K, 6] of history's dtype")
    if (tuple(ode_history.shape) != (S, B, K, PF_MAX_AUX) or ode_history.dtype != dt_ or ode_history.device != dev
            or not ode_history.is_contiguous()):
        raise HodeError(f"ukf_smooth: ode_history must be a contiguous [S, B, K, {PF_MAX_AUX}] of history's dtype")
    _need_vectors("ukf_smooth", dev, torch.float64, (("mean", mean, S * B * n), ("cov", cov, S * B * n * n), ("q", q, 6),
                                                     ("walk", walk, PF_MAX_AUX), ("dt", dt, S * B)))
    _need_vectors("ukf_smooth", dev, torch.int32, (("alive", alive, S * B),))
    gamma, wm0, wc0, wi = (float(v) for v in weights)
    shapes = ((S, B, n), (S, B, n, n), (S - 1, B, n, n), (S - 1, B, n), (S - 1, B, n, n), (S, B, 12))
    if out is None:
        out = tuple(torch.empty(sh, dtype=torch.float64, device=dev) for sh in shapes)
    if len(out) != 6 or not all(_is_buffer(t, torch.float64, dev, sh) for t, sh in zip(out, shapes)):
        raise HodeError("ukf_smooth: out must be (mean_s [S, B, n], cov_s [S, B, n, n], gain [S-1, B, n, n], pred_mean [S-1, B, n], "
                        "pred_cov [S-1, B, n, n], moments [S, B, 12]), contiguous fp64 on history's device")
    ins = {t.data_ptr() for t in (history, ode_history, propagated, mean, cov, alive, q, walk, dt)}
    outs = [t.data_ptr() for t in out if t.numel()]
    if any(p in ins for p in outs) or len(set(outs)) != len(outs):
        raise HodeError("ukf_smooth: an output may not alias an input or another output")
    _call("ukf_smooth", dt_, S, B, int(link), (C.c_int32 * PF_MAX_AUX)(*mode), gamma, wm0, wc0, wi, history, ode_history, propagated,
          mean, cov, alive, q, walk, dt, *out)
    return tuple(out)


UKF_EM_SUMS, UKF_EM_FIT = 37, 29
UKF_EM_SUM_AT = {"A": slice(0, 23), "N": 23, "D": 24, "R": slice(25, 31), "M": slice(31, 37)}      # the layout of `sums`


def _em_head(what, mode, mean_s, cov_s, alive):
    """(mode, S, B, n, K, device) of the smoothed run every EM entry starts from (include/hode_ukf_em.h)."""
    _need_gpu(mean_s)
    mode = [int(v) for v in (mode.tolist() if hasattr(mode, "tolist") else mode)]
    if len(mode) != PF_MAX_AUX or any(v not in (0, 1, 2) for v in mode):
        raise HodeError(f"{what}: mode must be {PF_MAX_AUX} host integers in 0..2 (PF_MOVE)")
    n = 6 + sum(1 for v in mode if v)
    if mean_s.dim() != 3 or mean_s.shape[2] != n or mean_s.shape[0] < 1 or mean_s.shape[1] < 1:
        raise HodeError(f"{what}: mean_s must be [S, B, n] with n = 6 + P = {n}, S >= 1, B >= 1")
    S, B = int(mean_s.shape[0]), int(mean_s.shape[1])
    dev = mean_s.device
    _need_vectors(what, dev, torch.float64, (("mean_s", mean_s, S * B * n), ("cov_s", cov_s, S * B * n * n)))
    _need_vectors(what, dev, torch.int32, (("alive", alive, S * B),))
    return mode, S, B, n, 2 * n + 1, dev


def _em_distinct(what, ins, outs):
    ins = {t.data_ptr() for t in ins if t is not None and t.numel()}
    outs = [t.data_ptr() for t in outs if t.numel()]
    if any(p in ins for p in outs) or len(set(outs)) != len(outs):
        raise HodeError(f"{what}: an output may not alias an input or another output")


def ukf_em_points(mean_s, cov_s, alive, ode_history, mode, weights, link=1, out=None):
    """The sigma points of the smoothed moments of every pair's first step (include/hode_ukf_em.h): mean_s fp64 [S, B, n], cov_s
    fp64 [S, B, n, n], alive int32 [S, B] and ode_history [S, B, K, 17] fp32 or fp64 on the device, step-major; mode: 17 ints on
    the HOST (PF_MOVE); weights = (gamma, wm0, wc0, wi).  `out`: the three buffers to write into, else they are allocated.
    Returns (x_em [S-1, B*K, 6], aux_em [S-1, B*K, 17] of ode_history's dtype, chol fp64 [S-1, B, n, n])."""
    mode, S, B, n, K, dev = _em_head("ukf_em_points", mode, mean_s, cov_s, alive)
    dt_ = ode_history.dtype
    _need_real(dt_)
    if tuple(ode_history.shape) != (S, B, K, PF_MAX_AUX) or ode_history.device != dev or not ode_history.is_contiguous():
        raise HodeError(f"ukf_em_points: ode_history must be a contiguous [S, B, K, {PF_MAX_AUX}] with K = 2 n + 1 = {K}")
    shapes = (((S - 1, B * K, 6), dt_), ((S - 1, B * K, PF_MAX_AUX), dt_), ((S - 1, B, n, n), torch.float64))
    if out is None:
        out = tuple(torch.empty(sh, dtype=d, device=dev) for sh, d in shapes)
    if len(out) != 3 or not all(_is_buffer(t, d, dev, sh) for t, (sh, d) in zip(out, shapes)):
        raise HodeError("ukf_em_points: out must be (x_em [S-1, B*K, 6], aux_em [S-1, B*K, 17] of ode_history's dtype, chol fp64 "
                        "[S-1, B, n, n]), contiguous on the device")
    _em_distinct("ukf_em_points", (mean_s, cov_s, alive, ode_history), out)
    _call("ukf_em_points", dt_, S, B, int(link), (C.c_int32 * PF_MAX_AUX)(*mode), float(weights[0]), mean_s, cov_s, alive, ode_history,
          *out)
    return tuple(out)


def ukf_em_stats(prop_em, status, chol, mean_s, cov_s, gain, alive, obs, mask, moments, mode, weights, link=1, out=None):
    """The expected squared residuals of one E-step (include/hode_ukf_em.h): prop_em [S-1, B*K, 6] fp32 or fp64, the end of the
    solve of ukf_em_points' rows over every pair's segment, and status int32 [S-1, B*K]; chol as ukf_em_points gave it; mean_s,
    cov_s, gain fp64 [S-1, B, n, n], moments fp64 [S, B, 12]: the smoother's; alive int32 [S, B]; obs [B, S, 6] of prop_em's dtype
    (PATIENT-major: the record's rows at the steps; NaN = missing) and mask uint8 [B, S, 6] or None.
    Returns (e2 fp64 [S-1, B, n], pair_ok int32 [S-1, B], r2 fp64 [S, B, 6], seen int32 [S, B])."""
    mode, S, B, n, K, dev = _em_head("ukf_em_stats", mode, mean_s, cov_s, alive)
    dt_ = prop_em.dtype
    _need_real(dt_)
    if tuple(prop_em.shape) != (S - 1, B * K, 6) or prop_em.device != dev or not prop_em.is_contiguous():
        raise HodeError(f"ukf_em_stats: prop_em must be a contiguous [S-1, B*K, 6] with K = 2 n + 1 = {K}")
    if tuple(obs.shape) != (B, S, 6) or obs.dtype != dt_ or obs.device != dev or not obs.is_contiguous():
        raise HodeError("ukf_em_stats: obs must be a contiguous [B, S, 6] of prop_em's dtype")
    if mask is not None and (tuple(mask.shape) != (B, S, 6) or mask.dtype != torch.uint8 or mask.device != dev or not mask.is_contiguous()):
        raise HodeError("ukf_em_stats: mask must be a contiguous uint8 [B, S, 6] or None")
    _need_vectors("ukf_em_stats", dev, torch.int32, (("status", status, (S - 1) * B * K),))
    _need_vectors("ukf_em_stats", dev, torch.float64, (("chol", chol, (S - 1) * B * n * n), ("gain", gain, (S - 1) * B * n * n),
                                                       ("moments", moments, S * B * 12)))
    shapes = (((S - 1, B, n), torch.float64), ((S - 1, B), torch.int32), ((S, B, 6), torch.float64), ((S, B), torch.int32))
    if out is None:
        out = tuple(torch.empty(sh, dtype=d, device=dev) for sh, d in shapes)
    if len(out) != 4 or not all(_is_buffer(t, d, dev, sh) for t, (sh, d) in zip(out, shapes)):
        raise HodeError("ukf_em_stats: out must be (e2 fp64 [S-1, B, n], pair_ok int32 [S-1, B], r2 fp64 [S, B, 6], seen int32 [S, B]), "
                        "contiguous on the device")
    _em_distinct("ukf_em_stats", (prop_em, status, chol, mean_s, cov_s, gain, alive, obs, mask, moments), out)
    gamma, wm0, wc0, wi = (float(v) for v in weights)
    _call("ukf_em_stats", dt_, S, B, int(link), (C.c_int32 * PF_MAX_AUX)(*mode), gamma, wm0, wc0, wi, prop_em, status, chol, mean_s, cov_s,
          gain, alive, obs, mask, moments, *out)
    return tuple(out)


def ukf_em_mstep(e2, pair_ok, r2, seen, dt, q, walk, sigma, mode, fit_mask, floor, link=1, sums=None, check_dt=True):
    """Reduce one E-step and update the noise IN PLACE (include/hode_ukf_em.h): e2 fp64 [S-1, B, n], pair_ok int32 [S-1, B],
    r2 fp64 [S, B, 6], seen int32 [S, B] as ukf_em_stats gave them, dt fp64 [S, B] (row 0 is not read); q fp64 [6], walk fp64 [17],
    sigma fp64 [6] on the device; mode, fit_mask (29 flags: q, walk by column, sigma) and floor (29 values >= 0) on the HOST.
    check_dt: read dt back once and refuse a dt <= 0 past row 0 (a caller that knows its grid passes False).
    Returns sums fp64 [37] (UKF_EM_SUM_AT): A by coordinate, N, D, R, M."""
    _need_gpu(r2)
    mode = [int(v) for v in (mode.tolist() if hasattr(mode, "tolist") else mode)]
    if len(mode) != PF_MAX_AUX or any(v not in (0, 1, 2) for v in mode):
        raise HodeError(f"ukf_em_mstep: mode must be {PF_MAX_AUX} host integers in 0..2 (PF_MOVE)")
    n = 6 + sum(1 for v in mode if v)
    if r2.dim() != 3 or r2.shape[2] != 6 or r2.shape[0] < 1 or r2.shape[1] < 1:
        raise HodeError("ukf_em_mstep: r2 must be [S, B, 6] with S >= 1, B >= 1")
    S, B, dev = int(r2.shape[0]), int(r2.shape[1]), r2.device
    fit_mask = [int(bool(v)) for v in (fit_mask.tolist() if hasattr(fit_mask, "tolist") else fit_mask)]
    floor = [float(v) for v in (floor.tolist() if hasattr(floor, "tolist") else floor)]
    if len(fit_mask) != UKF_EM_FIT or len(floor) != UKF_EM_FIT or not all(0.0 <= v < float("inf") for v in floor):
        raise HodeError(f"ukf_em_mstep: fit_mask and floor must hold {UKF_EM_FIT} host values (q [6], walk [17], sigma [6]), floor >= 0")
    _need_vectors("ukf_em_mstep", dev, torch.float64, (("e2", e2, (S - 1) * B * n), ("r2", r2, S * B * 6), ("dt", dt, S * B), ("q", q, 6),
                                                       ("walk", walk, PF_MAX_AUX), ("sigma", sigma, 6)))
    _need_vectors("ukf_em_mstep", dev, torch.int32, (("pair_ok", pair_ok, (S - 1) * B), ("seen", seen, S * B)))
    if sums is None:
        sums = torch.empty(UKF_EM_SUMS, dtype=torch.float64, device=dev)
    if not _is_buffer(sums, torch.float64, dev, numel=UKF_EM_SUMS):
        raise HodeError(f"ukf_em_mstep: sums must be a contiguous fp64 [{UKF_EM_SUMS}] on the device")
    _em_distinct("ukf_em_mstep", (e2, pair_ok, r2, seen, dt), (q, walk, sigma, sums))
    if check_dt and S > 1 and not bool((dt.view(S, B)[1:] > 0).all()):
        raise HodeError("ukf_em_mstep: every dt past row 0 must be positive")
    _call("ukf_em_mstep", None, S, B, int(link), (C.c_int32 * PF_MAX_AUX)(*mode), (C.c_int32 * UKF_EM_FIT)(*fit_mask),
          (C.c_double * UKF_EM_FIT)(*floor), e2, pair_ok, r2, seen, dt, q, walk, sigma, sums)
    return sums


PRED_MAX_BINS, PRED_FIXED_COLS, PRED_SCORE_BLOCKS = 32, 16, 128
PRED_STATE = ("n", "mean", "m2", "pit", "lmax", "lsum")


def pred_state(N, device):
    """A fresh running state of N entries (include/hode.h "Posterior-predictive summaries"): all zero, lmax = -inf."""
    z = lambda: torch.zeros(N, dtype=torch.float64, device=device)                               # noqa: E731
    return {"n": torch.zeros(N, dtype=torch.int32, device=device), "mean": z(), "m2": z(), "pit": z(),
            "lmax": torch.full((N,), float("-inf"), dtype=torch.float64, device=device), "lsum": z()}


def _pred_check_state(state, N, what):
    for k in PRED_STATE:
        t = state[k]
        if t.dtype != (torch.int32 if k == "n" else torch.float64) or t.numel() != N or not t.is_contiguous() or not t.is_cuda:
            raise HodeError(f"{what}: state[{k!r}] must be a contiguous device tensor of {N} {'int32' if k == 'n' else 'float64'}")


def _dense_rows(y, S, N):
    return y if y[0].is_contiguous() and (S == 1 or y.stride(0) == N) else y.contiguous()


def _need_obs_mask(what, obs, mask, N, dtype, dev, whose):
    if obs is not None and (obs.dtype != dtype or obs.numel() != N or not obs.is_contiguous() or obs.device != dev):
        raise HodeError(f"{what}: obs must be a contiguous device tensor of N entries in {whose} dtype")
    if mask is not None and (obs is None or mask.dtype != torch.uint8 or mask.numel() != N or not mask.is_contiguous()):
        raise HodeError(f"{what}: mask must be uint8 with the shape of obs")


def _status_rows(what, status, S, N, dev):
    if status is None:
        return None, N
    status = status.to(device=dev, dtype=torch.int32).contiguous()
    if status.dim() != 2 or status.shape[0] != S or status.shape[1] < 1 or N % status.shape[1]:
        raise HodeError(f"{what}: status must be [n_draws, n_traj] with n_traj dividing N")
    return status, N // status.shape[1]


def pred_fold(y, state, obs=None, mask=None, sigma=None, status=None):
    """Fold the draws y [n_draws, ...] (N entries each, fp32 or fp64, used where it lies when its rows are dense) into `state`
    (pred_state) in draw order; obs [N] in y's dtype and mask uint8 [N] or None; sigma fp64 [n_draws, 6] on the device or None;
    status int32 [n_draws, n_traj] or None (a non-zero entry skips that draw's trajectory)."""
    _need_gpu(y)
    S = y.shape[0]
    N = state["n"].numel()
    if y.dim() < 2 or y.numel() != S * N:
        raise HodeError(f"pred_fold: y must be [n_draws, {N} entries]")
    y = _dense_rows(y, S, N)
    _pred_check_state(state, N, "pred_fold")
    _need_obs_mask("pred_fold", obs, mask, N, y.dtype, y.device, "y's")
    if sigma is not None:
        sigma = sigma.to(device=y.device, dtype=torch.float64).contiguous()
        if tuple(sigma.shape) != (S, 6):
            raise HodeError("pred_fold: sigma must be [n_draws, 6]")
    status, row_len = _status_rows("pred_fold", status, S, N, y.device)
    _call("pred_fold", y.dtype, S, N, y, obs, mask, sigma, status, row_len, *[state[k] for k in PRED_STATE])


def pred_score(state, dtype, obs=None, mask=None, extra_var=None, thr=(0.0,)):
    """Score a finished state: returns (mean, sd, pit) [N] in `dtype` and the table fp64 [6, PRED_FIXED_COLS + 2 len(thr)] of
    include/hode.h; extra_var six host floats or None, thr the host thresholds of the calibration counts."""
    N = state["n"].numel()
    _need_gpu(state["n"])
    _pred_check_state(state, N, "pred_score")
    dev = state["n"].device
    nb = len(thr)
    if not 1 <= nb <= PRED_MAX_BINS:
        raise HodeError(f"pred_score: {nb} bins, the kernel takes 1..{PRED_MAX_BINS} (HODE_PRED_MAX_BINS)")
    _need_obs_mask("pred_score", obs, mask, N, dtype, dev, "the working")
    K = PRED_FIXED_COLS + 2 * nb
    out = [torch.empty(N, dtype=dtype, device=dev) for _ in range(3)]
    table = torch.empty(6, K, dtype=torch.float64, device=dev)
    work = torch.empty(PRED_SCORE_BLOCKS * 6 * K, dtype=torch.float64, device=dev)
    _call("pred_score", dtype, N, *[state[k] for k in PRED_STATE], obs, mask, _six(extra_var), (C.c_double * nb)(*[float(x) for x in thr]),
          nb, *out, table, work)
    return out[0], out[1], out[2], table


PRED_MAX_LEVELS, PRED_BAND_COLS = 16, 4


def pred_tail_state(N, K, dtype, device):
    """A fresh tail state of N entries that keeps the K smallest and the K largest values of each (include/hode.h "Posterior
    bands"): cnt = 0; the buffers lo, hi [K, N] in `dtype` need no initialisation."""
    _need_real(dtype)
    if int(N) < 1 or int(K) < 1:
        raise HodeError("pred_tail_state: N >= 1 and K >= 1")
    return {"cnt": torch.zeros(int(N), dtype=torch.int32, device=device),
            "lo": torch.empty(int(K), int(N), dtype=dtype, device=device), "hi": torch.empty(int(K), int(N), dtype=dtype, device=device)}


def _pred_check_tail_state(tstate, what):
    cnt, lo, hi = tstate["cnt"], tstate["lo"], tstate["hi"]
    N = cnt.numel()
    ok = cnt.dtype == torch.int32 and cnt.is_cuda and cnt.is_contiguous() and N >= 1 and lo.dim() == 2 and lo.shape[0] >= 1
    ok = ok and lo.dtype in (torch.float32, torch.float64)
    for t in (lo, hi):
        ok = ok and t.dtype == lo.dtype and tuple(t.shape) == (lo.shape[0], N) and t.is_contiguous() and t.device == cnt.device
    if not ok:
        raise HodeError(f"{what}: the tail state must be contiguous device tensors cnt int32 [N], lo and hi [K, N] of one float dtype")
    return N, lo.shape[0]


def pred_tails(y, tstate, status=None):
    """Take the draws y [n_draws, ...] (N entries each, in the dtype of the state's buffers, used where it lies when its rows are
    dense) into the tail state (pred_tail_state) in draw order; status int32 [n_draws, n_traj] or None as in pred_fold."""
    _need_gpu(y)
    N, K = _pred_check_tail_state(tstate, "pred_tails")
    S = y.shape[0]
    if y.dim() < 2 or y.numel() != S * N or y.dtype != tstate["lo"].dtype or y.device != tstate["cnt"].device:
        raise HodeError(f"pred_tails: y must be [n_draws, {N} entries] in the dtype and on the device of the state")
    y = _dense_rows(y, S, N)
    status, row_len = _status_rows("pred_tails", status, S, N, y.device)
    _call("pred_tails", y.dtype, S, N, y, status, row_len, K, tstate["cnt"], tstate["lo"], tstate["hi"])


def pred_quantiles(tstate, levels, obs=None, mask=None, band=False):
    """The quantiles of a tail state at `levels` (host fractions strictly inside (0, 1), ascending, at most PRED_MAX_LEVELS):
    returns (out [len(levels), N] in the state's dtype, band_table).  band=True also scores the band [levels[0], levels[-1]]
    against obs [N] (mask uint8 [N] or None) into the fp64 table [6, PRED_BAND_COLS] of include/hode.h; otherwise band_table
    is None.  The state's buffers are sorted in place and stay valid for further pred_tails calls."""
    N, K = _pred_check_tail_state(tstate, "pred_quantiles")
    dev, dtype = tstate["cnt"].device, tstate["lo"].dtype
    lv = [float(q) for q in levels]
    if not 1 <= len(lv) <= PRED_MAX_LEVELS:
        raise HodeError(f"pred_quantiles: {len(lv)} levels, the kernel takes 1..{PRED_MAX_LEVELS} (HODE_PRED_MAX_LEVELS)")
    if not all(0.0 < q < 1.0 for q in lv) or any(b <= a for a, b in zip(lv, lv[1:])):
        raise HodeError("pred_quantiles: levels must lie strictly inside (0, 1) and ascend")
    _need_obs_mask("pred_quantiles", obs, mask, N, dtype, dev, "the state's")
    table = work = None
    if band:
        if obs is None or N % 6 or not lv[0] < 0.5 < lv[-1]:
            raise HodeError("pred_quantiles: a band table needs obs, N % 6 == 0 and levels[0] < 1/2 < levels[-1]")
        table = torch.empty(6, PRED_BAND_COLS, dtype=torch.float64, device=dev)
        work = torch.empty(PRED_SCORE_BLOCKS * 6 * PRED_BAND_COLS, dtype=torch.float64, device=dev)
    out = torch.empty(len(lv), N, dtype=dtype, device=dev)
    _call("pred_quantiles", dtype, N, K, tstate["cnt"], tstate["lo"], tstate["hi"], len(lv), (C.c_double * len(lv))(*lv), out, obs, mask,
          table, work)
    return out, table


def pred_tail_values(tstate):
    """(lower, upper), each [K, N], of a tail state that pred_quantiles has sorted: the min(cnt, K) smallest and the min(cnt, K)
    largest values of every entry, ascending, NaN in the slots past them."""
    _, K = _pred_check_tail_state(tstate, "pred_tail_values")
    lo, hi = tstate["lo"], tstate["hi"]
    m = tstate["cnt"].clamp(max=K).to(torch.int64).unsqueeze(0)                                   # values held per entry
    r = torch.arange(K, device=lo.device).unsqueeze(1)                                            # ascending rank
    nan = torch.full((), float("nan"), dtype=lo.dtype, device=lo.device)
    # lo is sorted largest first, hi smallest first
    return torch.where(r < m, lo.gather(0, (m - 1 - r).clamp(min=0)), nan), torch.where(r < m, hi, nan)


PRED_LOO_COLS = 13
PRED_LOO_STATE = ("cnt", "lmean", "lm2", "pmax", "psum", "top", "rmax", "rsum")
PRED_LOO_OUTPUTS = ("elpd_loo", "pareto_k", "elpd_waic", "p_waic", "lppd")


def pred_loo_state(N, K, device):
    """A fresh LOO state of N entries that keeps the K largest log importance ratios of each (include/hode.h "Model
    comparison"): all zero except pmax = rmax = -inf; top [K, N] needs no initialisation."""
    N, K = int(N), int(K)
    if N < 6 or N % 6 or K < 2:
        raise HodeError("pred_loo_state: N a positive multiple of 6 and K >= 2")
    z = lambda: torch.zeros(N, dtype=torch.float64, device=device)                               # noqa: E731
    ninf = lambda: torch.full((N,), float("-inf"), dtype=torch.float64, device=device)           # noqa: E731
    return {"cnt": torch.zeros(N, dtype=torch.int32, device=device), "lmean": z(), "lm2": z(), "pmax": ninf(), "psum": z(),
            "top": torch.empty(K, N, dtype=torch.float64, device=device), "rmax": ninf(), "rsum": z()}


def _pred_check_loo_state(lstate, what):
    cnt, top = lstate["cnt"], lstate["top"]
    N = cnt.numel()
    ok = cnt.dtype == torch.int32 and cnt.is_cuda and cnt.is_contiguous() and top.dim() == 2
    for k in PRED_LOO_STATE[1:]:
        t = lstate[k]
        ok = ok and t.dtype == torch.float64 and t.is_contiguous() and t.device == cnt.device
        ok = ok and (tuple(t.shape) == (top.shape[0], N) if k == "top" else t.numel() == N)
    if not ok or N < 6 or N % 6 or top.shape[0] < 2:
        raise HodeError(f"{what}: the LOO state must be contiguous device tensors cnt int32 [N], top float64 [K, N] and six float64 [N], "
                        "N a multiple of 6 and K >= 2")
    return N, top.shape[0]


def pred_loo_fold(y, lstate, obs, mask, sigma, status=None):
    """Fold the pointwise log likelihood of the draws y [n_draws, ...] (N entries each, fp32 or fp64, used where it lies when its
    rows are dense) into the LOO state (pred_loo_state) in draw order; obs [N] in y's dtype, mask uint8 [N] or None, sigma fp64
    [n_draws, 6] and status int32 [n_draws, n_traj] or None as in pred_fold -- but obs and sigma are required."""
    _need_gpu(y)
    N, K = _pred_check_loo_state(lstate, "pred_loo_fold")
    S = y.shape[0]
    if y.dim() < 2 or y.numel() != S * N or y.device != lstate["cnt"].device:
        raise HodeError(f"pred_loo_fold: y must be [n_draws, {N} entries] on the device of the state")
    y = _dense_rows(y, S, N)
    if obs is None or sigma is None:
        raise HodeError("pred_loo_fold: obs and sigma are required (without observation noise there is no likelihood)")
    _need_obs_mask("pred_loo_fold", obs, mask, N, y.dtype, y.device, "y's")
    sigma = sigma.to(device=y.device, dtype=torch.float64).contiguous()
    if tuple(sigma.shape) != (S, 6):
        raise HodeError("pred_loo_fold: sigma must be [n_draws, 6]")
    status, row_len = _status_rows("pred_loo_fold", status, S, N, y.device)
    _call("pred_loo_fold", y.dtype, S, N, y, obs, mask, sigma, status, row_len, K, *[lstate[k] for k in PRED_LOO_STATE])


def pred_loo_fit_rows(K):
    """Rows of the finish's scratch buffer fit[rows][N] for a state of K slots: (K - 1) + 30 + floor(sqrt(K - 1))."""
    import math
    return (int(K) - 1) + 30 + math.isqrt(int(K) - 1)


def pred_loo_finish(lstate, dtype, r_eff=1.0):
    """PSIS-LOO and WAIC of a LOO state: returns ({elpd_loo, pareto_k, elpd_waic, p_waic, lppd}, each [N] in `dtype`, NaN where
    undefined, and the table fp64 [6, PRED_LOO_COLS] of include/hode.h).  r_eff: the relative efficiency of the draws, a host
    scalar in (0, 1].  The state's top is sorted in place and stays valid for further pred_loo_fold calls."""
    N, K = _pred_check_loo_state(lstate, "pred_loo_finish")
    _need_real(dtype)
    r_eff = float(r_eff)
    if not 0.0 < r_eff <= 1.0:
        raise HodeError("pred_loo_finish: r_eff must lie in (0, 1]")
    dev = lstate["cnt"].device
    out = {k: torch.empty(N, dtype=dtype, device=dev) for k in PRED_LOO_OUTPUTS}
    table = torch.empty(6, PRED_LOO_COLS, dtype=torch.float64, device=dev)
    fit = torch.empty(pred_loo_fit_rows(K), N, dtype=torch.float64, device=dev)
    work = torch.empty(PRED_SCORE_BLOCKS * 6 * PRED_LOO_COLS, dtype=torch.float64, device=dev)
    _call("pred_loo_finish", dtype, N, K, r_eff, *[lstate[k] for k in PRED_LOO_STATE], *[out[k] for k in PRED_LOO_OUTPUTS], table, fit,
          work)
    return out, table


def pred_loo_top_values(lstate):
    """[K, N]: the min(cnt, K) largest log importance ratios of every entry of a state that pred_loo_finish has sorted, ascending,
    NaN in the slots past them."""
    _, K = _pred_check_loo_state(lstate, "pred_loo_top_values")
    top = lstate["top"]
    m = lstate["cnt"].clamp(max=K).to(torch.int64).unsqueeze(0)
    r = torch.arange(K, device=top.device).unsqueeze(1)
    return torch.where(r < m, top, torch.full((), float("nan"), dtype=top.dtype, device=top.device))


def hmc_refresh(C_, D, ld, seed, it, jitter, minv, log_eps, z, g, U, p, z0, g0, U0, ke0, eps, failed):
    _call("hmc_refresh", z.dtype, C_, D, ld, seed, it, jitter, minv, log_eps, z, g, U, p, z0, g0, U0, ke0, eps, failed)


def hmc_leapfrog(C_, D, ld, flags, kick, eps, minv, z, p, g, gnn, gode, P, loss_sum, lik_scale, status, n_traj, U, ke, failed,
                 ode_mask, mu, sd, sample_nn, nn_p, ode_p):
    _call("hmc_leapfrog", z.dtype, C_, D, ld, flags, kick, eps, minv, z, p, g, gnn, gode, P, loss_sum, lik_scale, status, n_traj, U, ke,
          failed, ode_mask, mu, sd, int(sample_nn), nn_p, ode_p)


def hmc_accept(C_, D, ld, mode, seed, it, target_accept, z, z0, g, g0, U, U0, ke0, ke, failed, log_eps, da, search, n_ode, mu, sd,
               draws=None, stats=None, n_slots=0, slot=-1):
    _call("hmc_accept", z.dtype, C_, D, ld, mode, seed, it, target_accept, z, z0, g, g0, U, U0, ke0, ke, failed, log_eps, da, search,
          n_ode, mu, sd, draws, stats, n_slots, slot)


def hmc_welford(C_, D, ld, flags, z, wf, minv):
    _call("hmc_welford", minv.dtype, C_, D, ld, flags, z, wf, minv)


def pop_params(A, B, K, ld, coords, ode_mask, mu0, sd0, tau0, tau_log_sd, ode_base, ode_p):
    """The population map of the first A rows of coords [., ld] into ode_p [A * B, 17] (include/hode.h "Population model")."""
    _call("pop_params", coords.dtype, A, B, K, ld, coords, ode_mask, mu0, sd0, tau0, tau_log_sd, ode_base, ode_p)


def pop_grad(A, B, K, ld, coords, gode, ode_mask, sd0, tau0, tau_log_sd, glik):
    """The transposed population map: gode [A * B, 17] -> the likelihood gradient glik [A, ld] of the first A rows of coords."""
    _call("pop_grad", coords.dtype, A, B, K, ld, coords, gode, ode_mask, sd0, tau0, tau_log_sd, glik)


X0_LINK_IDENTITY, X0_LINK_LOG = 0, 1


def x0_params(A, B, n_lat, ld, off, coords, lat_mask, link, m, s, x0_base, x0_out, K=0, ode_mask=0, mu=None, sd=None, ode_base=None,
              ode_p=None):
    """The initial-state map of the first A rows of coords [., ld] into x0_out [A * B, 6] and, with ode_p, the rows' global
    constants into ode_p [A, 17] (include/hode.h "Initial-state model")."""
    _call("x0_params", coords.dtype, A, B, n_lat, ld, off, coords, lat_mask, link, m, s, x0_base, x0_out, K, ode_mask, mu, sd, ode_base,
          ode_p)


def x0_grad(A, B, n_lat, ld, off, coords, lat_mask, link, m, s, gx0, glik, K=0, ode_mask=0, sd=None, gode=None):
    """The transposed initial-state map: gx0 [A * B, 6] (and gode [A, 17]) -> the entries of the likelihood gradient glik [A, ld]
    that the layer owns; nothing else of glik is touched."""
    _call("x0_grad", coords.dtype, A, B, n_lat, ld, off, coords, lat_mask, link, m, s, gx0, K, ode_mask, sd, gode, glik)


NUTS_ROWS, NUTS_MAX_DEPTH = 15, 30


def nuts_begin(C_, D, ld, z, p, g, U, U0, ke0, tree, dst, ist):
    _call("nuts_begin", z.dtype, C_, D, ld, z, p, g, U, U0, ke0, tree, dst, ist)


def nuts_pre(C_, D, ld, seed, it, eps, minv, tree, ist, rank, ode_mask, mu, sd, sample_nn, P, nn_p, ode_p):
    _call("nuts_pre", tree.dtype, C_, D, ld, seed, it, eps, minv, tree, ist, rank, ode_mask, mu, sd, int(sample_nn), P, nn_p, ode_p)


def nuts_post(C_, D, ld, max_depth, seed, it, eps, minv, tree, ckpt, dst, ist, rank, gnn, gode, P, loss_sum, lik_scale, status, n_traj,
              ode_mask, sd, sample_nn):
    _call("nuts_post", tree.dtype, C_, D, ld, max_depth, seed, it, eps, minv, tree, ckpt, dst, ist, rank, gnn, gode, P, loss_sum,
          lik_scale, status, n_traj, ode_mask, sd, int(sample_nn))


def nuts_compact(C_, ist, rank, count):
    _call("nuts_compact", None, C_, ist, rank, count)


def nuts_finish(C_, D, ld, adapt, target_accept, z, g, U, tree, dst, ist, log_eps, da, n_ode, mu, sd, draws=None, stats=None, n_slots=0,
                slot=-1):
    _call("nuts_finish", z.dtype, C_, D, ld, int(adapt), target_accept, z, g, U, tree, dst, ist, log_eps, da, n_ode, mu, sd, draws,
          stats, n_slots, slot)


# --------------------------------------------------------------------------------------------- data side
FOURGI_NPAR = 26
FOURGI_SCRATCH_BYTES = 98304
FOURGI_COLUMNS = ["subject_id", "time_hours", "time_minutes", "glucose_mmol_L", "insulin_pmol_L", "glp1_pmol_L",
                  "glucagon_pmol_L", "gip_pmol_L", "meal_indicator"]


def fourgi_default_params(patient_type="T2DM"):
    """The reference's parameter set (data/generate4GI.py:15-64) as a list of 26 floats (host call, no GPU needed)."""
    buf = (C.c_double * FOURGI_NPAR)()
    _check(load().hode_4gi_default_params(_ptype(patient_type), buf), "hode_4gi_default_params")      # a host call: no stream
    return list(buf)


def _ptype(patient_type):
    if patient_type in ("T2DM", 0):
        return 0
    if patient_type in ("HV", 1):
        return 1
    raise HodeError(f"patient_type must be 'T2DM' or 'HV', got {patient_type!r}")


def _par_host(par):
    if par is None:
        return None
    if len(par) != FOURGI_NPAR:
        raise HodeError(f"par must hold {FOURGI_NPAR} values")
    return (C.c_double * FOURGI_NPAR)(*[float(v) for v in par])


def fourgi_generate(bsl, T, interval_min, meal_time, meal_size, patient_type="T2DM", par=None, z=None, noise_cv=0.0,
                    subject0=0, rtol=1e-10, atol=1e-12, max_steps=100000, z_tcb=None):
    """K7.  bsl[B,5] (device, fp64) -> (table[B*T,9] fp64, status[B] int32).  meal_time/meal_size: [n] or [B,n].
    Noise draws: z[B,5,T] (numpy-stream order, transposed here) or z_tcb[T,5,B] (the kernel's layout, used as is)."""
    _need_gpu(bsl)
    dev = bsl.device
    bsl = bsl.to(torch.float64).contiguous().view(-1, 5)
    B = bsl.shape[0]
    mt = torch.as_tensor(meal_time, dtype=torch.float64, device=dev).contiguous()
    ms = torch.as_tensor(meal_size, dtype=torch.float64, device=dev).contiguous()
    if mt.shape != ms.shape or mt.dim() not in (1, 2) or (mt.dim() == 2 and mt.shape[0] != B):
        raise HodeError(f"meal_time / meal_size must both be [n_meals] or [B,n_meals], got {tuple(mt.shape)} / {tuple(ms.shape)}")
    n_meals = mt.shape[-1]
    if z is not None:
        # z[B,5,T] is the order FourGIModel.generate_dataset consumes numpy's stream in; the kernel wants [T,5,B]
        if tuple(z.shape) != (B, 5, T):
            raise HodeError(f"z must be [B,5,T]=({B},5,{T}), got {tuple(z.shape)}")
        z = z.to(device=dev, dtype=torch.float64).permute(2, 1, 0).contiguous()
    elif z_tcb is not None:
        if tuple(z_tcb.shape) != (T, 5, B):
            raise HodeError(f"z_tcb must be [T,5,B]=({T},5,{B}), got {tuple(z_tcb.shape)}")
        z = z_tcb.to(device=dev, dtype=torch.float64).contiguous()
    table = torch.empty(B * T, 9, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _call("4gi_generate_f64", None, B, T, interval_min, _ptype(patient_type), _par_host(par), bsl, n_meals, mt if n_meals else None,
          ms if n_meals else None, int(mt.dim() == 2), z, noise_cv, subject0, rtol, atol, max_steps, table, status)
    return table, status


def fourgi_rhs(bsl, y, meal, patient_type="T2DM", par=None):
    _need_gpu(y)
    dev = y.device
    y = y.to(torch.float64).contiguous().view(-1, 8)
    B = y.shape[0]
    bsl = bsl.to(device=dev, dtype=torch.float64).contiguous().view(-1, 5)
    meal = meal.to(device=dev, dtype=torch.float64).contiguous().view(-1)
    assert bsl.shape[0] == B and meal.shape[0] == B
    d = torch.empty_like(y)
    _call("4gi_rhs_f64", None, B, _ptype(patient_type), _par_host(par), bsl, y, meal, d)
    return d


def _window_args(table, row0, seq_len, check_bounds):
    _need_gpu(table)
    if table.dtype != torch.float64 or table.dim() != 2:
        raise HodeError("table must be a 2-D float64 tensor")
    row0 = row0.to(device=table.device, dtype=torch.int64).contiguous()
    N, S = row0.numel(), int(seq_len)
    # checked on the host BEFORE the launch (two device reductions + a sync); callers that built row0 from the table's
    # own subject ranges (GlucoseDataset) pass check_bounds=False
    if check_bounds and N and (int(row0.min()) < 0 or int(row0.max()) + S > table.shape[0]):
        raise HodeError("window outside the table")
    return table.contiguous(), row0, N, S, table.device


def fourgi_window_moments(table, cols, row0, seq_len, check_bounds=True):
    """Mergeable statistics of one shard's windows -> tensor[13] = {count, mean[6], M2[6]} on the device."""
    table, row0, N, S, dev = _window_args(table, row0, seq_len, check_bounds)
    mom = torch.empty(13, dtype=torch.float64, device=dev)
    scratch = torch.empty(FOURGI_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    g = lambda k: int(cols.get(k, -1))                                                            # noqa: E731
    _call("4gi_window_moments_f64", None, table, table.shape[1], g("glucose"), g("insulin"), g("glucagon"), g("glp1"), g("ge"), g("ffa"),
          row0, N, S, mom, scratch)
    return mom


def combine_moments(moments):
    """moments[R,13] (one row per shard, rank order) -> (mean[6], std[6]) float64 CPU tensors: Chan's pairwise merge,
    applied in rank order so that every rank gets the same bits; std = sqrt(M2 / n) + 1e-6 (train_hybrid.py:124-127)."""
    m = torch.as_tensor(moments, dtype=torch.float64).cpu().reshape(-1, 13)
    n, mean, m2 = 0.0, torch.zeros(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
    for r in range(m.shape[0]):
        nb = float(m[r, 0])
        if nb == 0:
            continue
        d = m[r, 1:7] - mean
        tot = n + nb
        m2 = m2 + m[r, 7:13] + d * d * (n * nb / tot)
        mean = mean + d * (nb / tot)
        n = tot
    if n == 0:
        return torch.zeros(6, dtype=torch.float64), torch.ones(6, dtype=torch.float64)
    return mean, torch.sqrt(m2 / n) + 1e-6


def fourgi_windows(table, cols, time_div, row0, seq_len, normalize=True, mean_std=None, check_bounds=True):
    """K8.  table[rows,ncols] fp64 (device); cols: dict time/glucose/insulin/glucagon/glp1 (+ optional ge/ffa/meal/tvns)
    -> column index; row0[N] int64 (device).  -> states[N,S,6], meal[N,S], tvns[N,S], time[N,S] (fp32), mean_std[12] (fp64)."""
    table, row0, N, S, dev = _window_args(table, row0, seq_len, check_bounds)
    states = torch.empty(N, S, 6, dtype=torch.float32, device=dev)
    meal, tvns, time = (torch.empty(N, S, dtype=torch.float32, device=dev) for _ in range(3))
    if mean_std is not None:                            # statistics given (HODE_4GI_NORM_GIVEN)
        mean_std = torch.as_tensor(mean_std, dtype=torch.float64).to(dev).contiguous().clone()
        if mean_std.numel() != 12:
            raise HodeError("mean_std must hold 6 means and 6 stds")
        normalize = 2
    else:
        mean_std = torch.empty(12, dtype=torch.float64, device=dev)
        normalize = int(bool(normalize))
    scratch = torch.empty(FOURGI_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    g = lambda k: int(cols.get(k, -1))                                                            # noqa: E731
    _call("4gi_windows_f32", None, table, table.shape[1], g("time"), time_div, g("glucose"), g("insulin"), g("glucagon"), g("glp1"),
          g("ge"), g("ffa"), g("meal"), g("tvns"), row0, N, S, normalize, states, meal, tvns, time, mean_std, scratch)
    return states, meal, tvns, time, mean_std
