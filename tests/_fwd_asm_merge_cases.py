"""The cases of tests/test_fwd_asm_merge_gpu.py, shared with tools/record_fwd_asm_merge.py (which records what the library
of the commit BEFORE the change gives for them): the smallest shapes at which the fp32 register path of csrc/hode_mlp.h --
mlp_hidden_blk, out_rot, the state broadcasts -- can go wrong.

The networks are cut out of the golden 64 x 4 network (tests/golden/g0_weights_h64_l4.npz): the leading H units of the first
layer, of the first L - 1 hidden matrices and of the output layer.  No random numbers, so the test and the recorder cannot
disagree about them; the inputs are stored in the fixtures."""
import os

import numpy as np

H0, L0 = 64, 4
FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_asm_merge")

# name, B, T, H, L, method (0 = DP5(4), 1 = RK4), taped, what
SOLVE_CASES = [
    ("base_l1", 3, 12, 64, 1, 0, False),      # T = 12: the y staging (6 reals per row) crosses its 64-real boundary in the 11th row
    ("base_l2", 3, 12, 64, 2, 0, False),
    ("base_l3", 3, 12, 64, 3, 0, False),
    ("base_l4", 3, 12, 64, 4, 0, False),
    ("h48_l4", 3, 12, 48, 4, 0, False),       # lanes 48..63 padded with zeros
    ("rk4_tape", 3, 5, 64, 4, 1, True),
    ("dp54_tape", 3, 5, 64, 4, 0, True),
]
REJECT_RTOL, REJECT_ATOL = 1e-8, 1e-10        # the rejected-steps case: one trajectory, one meal pulse


def sub_network(nn_flat, H, L):
    """Parameters [W1 (H x 9), b1 (H), (W (H x H), b (H)) x (L - 1), Wout (6 x H), bout (6)] of the H x L corner of the golden network."""
    nn_flat = np.asarray(nn_flat, dtype=np.float32)
    assert nn_flat.size == 9 * H0 + H0 + (L0 - 1) * (H0 * H0 + H0) + 6 * H0 + 6 and H <= H0 and 1 <= L <= L0
    o = 0
    W1 = nn_flat[o:o + 9 * H0].reshape(H0, 9); o += 9 * H0
    b1 = nn_flat[o:o + H0]; o += H0
    parts = [W1[:H].ravel(), b1[:H]]
    for l in range(L0 - 1):
        W = nn_flat[o:o + H0 * H0].reshape(H0, H0); o += H0 * H0
        b = nn_flat[o:o + H0]; o += H0
        if l < L - 1:
            parts += [W[:H, :H].ravel(), b[:H]]
    Wo = nn_flat[o:o + 6 * H0].reshape(6, H0); o += 6 * H0
    parts += [Wo[:, :H].ravel(), nn_flat[o:o + 6]]
    out = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)
    assert out.size == 9 * H + H + (L - 1) * (H * H + H) + 6 * H + 6
    return out


def make_inputs(B, T, seed):
    """A physiological cohort on a 5-minute grid with random meals and tVNS (recorder only: the test reads them from the fixture)."""
    g = np.random.default_rng(seed)
    base = np.array([5., 60., 80., 10., 0., 1.], dtype=np.float32)
    x0 = (base * (1 + 0.05 * g.standard_normal((B, 6)))).astype(np.float32)
    t = (np.arange(T) / 12.0).astype(np.float32)
    meal = (2.0 * g.random((B, T))).astype(np.float32)
    tvns = (g.random((B, T)) > 0.7).astype(np.float32)
    return x0, t, meal, tvns


def fixture(name):
    return os.path.join(FIXTURE_DIR, name + ".npz")


def run_solve(hode, torch, inp, nn, ode, H, L, method, taped, rtol=1e-6, atol=1e-8):
    """One solve (and, taped, its adjoint for the stored cotangent) -> {name: numpy array}."""
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    sol = hode.solve_fwd(f(inp["x0"]), f(inp["t"]), f(inp["meal"]), f(inp["tvns"]), None, f(ode), f(nn), H, L, method=method,
                         rtol=rtol, atol=atol, want_tape=taped)
    out = {k: getattr(sol, k).cpu().numpy() for k in ("y", "status", "nsteps", "nfev")}
    if taped and "c" in inp:
        gx0, gnn, _ = hode.solve_bwd(sol, f(inp["c"]))
        out["gx0"], out["gnn"] = gx0.cpu().numpy(), gnn.cpu().numpy()
    return out, sol


def run_rhs(hode, torch, inp, nn, ode):
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    return {"f": hode.rhs_fwd(f(inp["x"]), f(inp["t"]), f(inp["meal"]), f(inp["tvns"]), None, f(ode), f(nn), H0, L0).cpu().numpy()}


def run_jvp(hode, torch, inp, nn, ode):
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    out, sol = run_solve(hode, torch, inp, nn, ode, H0, L0, 0, True)
    out["dy"] = hode.solve_jvp(sol, v_ode=f(inp["v_ode"]), v_x0=f(inp["v_x0"])).cpu().numpy()
    return out
