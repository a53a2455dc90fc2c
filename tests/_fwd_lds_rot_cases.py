"""The cases of tests/test_fwd_lds_rot_gpu.py, shared with tools/record_fwd_lds_rot.py (which records what the library of the
commit BEFORE a change of the forward kernels' hidden layer gives for them): the paths of solve_fwd_kernel that the fixtures of
tests/golden/fwd_asm_merge/ do not reach.

  gd / gd_tape   the Hill term on (gd_mode 2, a value per grid point): the rolled-stage instantiation, the hidden layers inside
                 `#pragma unroll 1` loops; plain, and taped with its adjoint
  multi          B = 8 200 two-point-style solves (T = 3) of ONE parameter set: the smallest batch above the 8 192 threshold of the
                 MULTI routing, so every wave integrates two trajectories one after the other with the same weight registers (and
                 whatever per-wave LDS the kernel keeps)
  gd_l3 / gd_tape_l3 / multi_l3   the same three with TWO hidden matrices (L = 3), and
  rk4_gd_l4      RK4 with the Hill term at L = 4: with three hidden matrices the DP5(4) instantiations above have no register for the
                 LDS-fed layer (FwdRot, csrc/hode_solve_fwd.hip, keeps mlp_hidden_blk there); these four are the Hill-term, taping
                 and MULTI instantiations that DO take it
  sets           three parameter sets in one launch, as the Sobol leg launches them
  zero_in        first-layer weights and bias zero, so the input of the first hidden matrix is all zeros; H = 16, so three of the four
                 16-lane rows are padding

Networks are cut out of the golden 64 x 4 network as in _fwd_asm_merge_cases; the inputs of the small cases are stored in the
fixtures.  The 8 200 trajectories of `multi` are made from their indices by exact integer and single float32 operations (no
random generator, no libm), so recorder and test build the same bits; its fixture keeps 64 rows of the result and the sha256
of all of it."""
import hashlib
import os

import numpy as np

import _fwd_asm_merge_cases as A

H0, L0 = A.H0, A.L0
FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_lds_rot")
MULTI_B, MULTI_T = 8200, 3
MULTI_ROWS = np.array(list(range(0, MULTI_B, 131))[:62] + [MULTI_B - 2, MULTI_B - 1])     # both trajectories of a wave, first and last wave


def fixture(name):
    return os.path.join(FIXTURE_DIR, name + ".npz")


def unit(idx, salt):
    """idx (integers) -> float32 in [0, 1) with 24 significant bits: a multiplicative hash, exact in every step."""
    v = (np.asarray(idx, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    return ((v >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def multi_inputs():
    b = np.arange(MULTI_B)
    base = np.array([5., 60., 80., 10., 0., 1.], dtype=np.float32)
    u = np.stack([unit(b * 6 + c, 1) for c in range(6)], axis=1)                                  # [B, 6]
    x0 = (base[None, :] * (np.float32(0.95) + np.float32(0.1) * u)).astype(np.float32)
    t = (np.arange(MULTI_T, dtype=np.float32) * np.float32(1.0 / 16.0)).astype(np.float32)
    k = b[:, None] * MULTI_T + np.arange(MULTI_T)[None, :]
    meal = (np.float32(2.0) * unit(k, 2)).astype(np.float32)
    tvns = (unit(k, 3) > np.float32(0.7)).astype(np.float32)
    return dict(x0=x0, t=t, meal=meal, tvns=tvns)


def zero_input_network(nn_flat, H, L):
    nn = A.sub_network(nn_flat, H, L).copy()
    nn[:9 * H + H] = 0.0                      # W1 and b1: relu(0) = 0 enters the first hidden matrix
    return nn


def run(hode, torch, inp, nn, ode, H, L, taped=False, n_sets=1, method=0):
    """One solve, DP5(4) unless method = 1 (RK4), and, taped, its adjoint for the stored cotangent -> {name: numpy array}."""
    f = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    sol = hode.solve_fwd(f(inp["x0"]), f(inp["t"]), f(inp["meal"]), f(inp["tvns"]), f(inp.get("gd")), f(ode), f(nn), H, L, method=method,
                         n_sets=n_sets, want_tape=taped)
    out = {k: getattr(sol, k).cpu().numpy() for k in ("y", "status", "nsteps", "nfev")}
    if taped:
        gx0, gnn, _ = hode.solve_bwd(sol, f(inp["c"]))
        out["gx0"], out["gnn"] = gx0.cpu().numpy(), gnn.cpu().numpy()
    return out


def multi_digest(out):
    """What the `multi` fixture keeps of a full result."""
    r = MULTI_ROWS
    return dict(y=out["y"][r].copy(), status=out["status"][r].copy(), nsteps=out["nsteps"][r].copy(), nfev=out["nfev"][r].copy(),
                y_sha256=np.frombuffer(hashlib.sha256(np.ascontiguousarray(out["y"]).tobytes()).digest(), dtype=np.uint8).copy())
