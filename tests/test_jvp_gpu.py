"""GPU tests of the tangent-linear solve (hode.solve_jvp, csrc/hode_solve_jvp.hip) and HybridODENN.sensitivities.

The JVP and the adjoint (hode.solve_bwd) differentiate the same discrete scheme over the same tape, so
<gy, J v> = <J^T gy, v> holds to rounding: that duality against already validated code is the main check.  Finite differences
(RK4: exact for the discrete map; DP5(4) at a tight tolerance: the converged solution), the row and failure rules, bit
reproducibility and the read-only tape complete it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dt=torch.float64):
    return None if a is None else torch.as_tensor(np.asarray(a)).to("cuda", dt).contiguous()


def rand_net(H, L, rng):
    parts = [rng.standard_normal((H, 9)) * 0.03, rng.standard_normal(H) * 0.3]
    for _ in range(L - 1):
        parts += [rng.standard_normal((H, H)) * 0.8 / np.sqrt(H), rng.standard_normal(H) * 0.1]
    parts += [rng.standard_normal((6, H)) * 0.005 / np.sqrt(H), rng.standard_normal(6) * 0.001]
    return np.concatenate([p.ravel() for p in parts])


def case(H=64, L=4, B=8, T=25, modes=(2, 2, 2), t_batched=False, n_sets=1, seed=0, g0=None):
    """Initial states around the basal point, a 0..120 grid, meal pulses / tVNS / GD in the given modes, and n_sets parameter
    sets (constants and networks perturbed per set)."""
    rng = np.random.default_rng(seed)
    x0 = np.array([5.0, 60.0, 80.0, 10.0, 0.0, 1.0]) * (1 + 0.05 * rng.standard_normal((B, 6)))
    t = np.linspace(0.0, 120.0, T)
    if t_batched:
        t = t[None] * (1 + 0.1 * rng.random((B, 1)))
    u = []
    for q, mode in enumerate(modes):
        gen = [lambda s: 0.05 * (rng.random(s) < 0.2), lambda s: rng.random(s), lambda s: rng.uniform(0, 1500, s) * (rng.random(s) < 0.8)][q]
        u.append(None if mode == 0 else gen((B,)) if mode == 1 else gen((B, T)))
    nn = g0["nn"] if (g0 is not None and (H, L) == (g0["H"], g0["L"])) else rand_net(H, L, rng)
    ode = g0["ode"] if g0 is not None else np.load(os.path.join(ROOT, "tests", "golden", "g0_weights_h64_l4.npz"))["ode"]
    nn = np.concatenate([nn * (1 + 0.02 * rng.standard_normal(nn.shape)) if s else nn for s in range(n_sets)])
    ode = np.concatenate([ode * (1 + 0.05 * rng.standard_normal(17)) if s else ode for s in range(n_sets)])
    return dict(x0=x0, t=t, u=u, nn=nn, ode=ode, H=H, L=L, n_sets=n_sets, B=B, T=T)


def solve(c, dt=torch.float64, method=0, rtol=1e-6, atol=1e-8, x0=None, ode=None, want_tape=True, max_steps=None):
    import hode
    return hode.solve_fwd(dev(c["x0"] if x0 is None else x0, dt), dev(c["t"], dt), *(dev(v, dt) for v in c["u"]),
                          dev(c["ode"] if ode is None else ode, dt), dev(c["nn"], dt), c["H"], c["L"], method=method, rtol=rtol,
                          atol=atol, n_sets=c["n_sets"], want_tape=want_tape, max_steps=max_steps)


def directions(c, K, seed, dt=torch.float64):
    rng = np.random.default_rng(seed)
    v_ode = rng.standard_normal((c["n_sets"], K, 17)) * np.abs(c["ode"]).reshape(c["n_sets"], 1, 17)
    v_x0 = rng.standard_normal((c["B"], K, 6))
    return dev(v_ode, dt), dev(v_x0, dt)


def check_duality(c, dt, tol, K=3, method=0, seed=1):
    import hode
    sol = solve(c, dt, method, max_steps=3000)
    assert int(sol.status.max()) == 0
    v_ode, v_x0 = directions(c, K, seed, dt)
    dy = hode.solve_jvp(sol, v_ode, v_x0)
    assert dy.shape == (c["B"], K, c["T"], 6) and bool(torch.isfinite(dy).all())
    gy = dev(np.random.default_rng(seed + 7).standard_normal((c["B"], c["T"], 6)), dt)
    gx0, _, gode = hode.solve_bwd(sol, gy, want_gnn=False, want_gode=True)
    gode = gode.view(c["n_sets"], 17)
    for k in range(K):
        lhs = gy.double() * dy[:, k].double()
        r0, r1 = gx0.double() * v_x0[:, k].double(), gode.double() * v_ode[:, k].double()
        scale = float(lhs.abs().sum() + r0.abs().sum() + r1.abs().sum())
        err = abs(float(lhs.sum() - r0.sum() - r1.sum()))
        assert err <= tol * scale, (k, err / scale)
    # each part on its own
    for vo, vx in ((v_ode, None), (None, v_x0)):
        dyp = hode.solve_jvp(sol, vo, vx)
        rhs = (gode * vo[:, 0]).sum() if vo is not None else (gx0 * vx[:, 0]).sum()
        lhs = (gy * dyp[:, 0]).sum()
        assert abs(float(lhs - rhs)) <= tol * float((gy * dyp[:, 0]).abs().sum() + 1e-300) * 10


# ------------------------------------------------------------------ 1. duality with the adjoint on the same tape
DUAL = {
    "h64l4_modes222_shared": dict(H=64, L=4, modes=(2, 2, 2)),
    "h64l4_sets_batched_modes111": dict(H=64, L=4, modes=(1, 1, 1), t_batched=True, n_sets=8),
    "h32l2_no_inputs": dict(H=32, L=2, modes=(0, 0, 0)),
    "h64l1_modes201": dict(H=64, L=1, modes=(2, 0, 1)),
    "h48l3_modes120_batched": dict(H=48, L=3, modes=(1, 2, 0), t_batched=True, n_sets=2),
}


@pytest.mark.parametrize("name", list(DUAL))
def test_jvp_is_the_transpose_of_the_adjoint_fp64(name, g0):
    check_duality(case(g0=g0, **DUAL[name]), torch.float64, 1e-11)


def test_jvp_is_the_transpose_of_the_adjoint_rk4_fp64(g0):
    check_duality(case(g0=g0, modes=(2, 2, 2)), torch.float64, 1e-11, method=1)


@pytest.mark.parametrize("HL", [(64, 4), (32, 2)])
def test_jvp_is_the_transpose_of_the_adjoint_fp32(HL, g0):
    check_duality(case(g0=g0, H=HL[0], L=HL[1], modes=(2, 2, 2), n_sets=2, B=16), torch.float32, 1e-4, K=9)


# ------------------------------------------------------------------ 2. duality against the CPU oracle's adjoint
def test_jvp_against_the_oracle_adjoint(g0):
    import hode
    from oracle import oracle as O
    c = case(g0=g0, B=4, modes=(2, 2, 2))
    sol = solve(c)
    v_ode, v_x0 = directions(c, 2, 3)
    dy = hode.solve_jvp(sol, v_ode, v_x0).cpu().numpy()
    rng = np.random.default_rng(5)
    for b in range(c["B"]):
        u = [None if v is None else v[b:b + 1] for v in c["u"]]
        ref = O.solve(c["x0"][b:b + 1], c["t"], *u, c["ode"], c["nn"], 64, 4, dtype=np.float64, want_tape=True)
        assert int(ref.status[0]) == 0 and int(ref.nsteps[0]) == int(sol.nsteps[b])
        gy = rng.standard_normal((1, c["T"], 6))
        gx0, _, gode = O.solve_bwd(ref, gy, want_gnn=False, want_gode=True)
        for k in range(2):
            lhs = float((gy[0] * dy[b, k]).sum())
            rhs = float((gx0[0] * v_x0[b, k].cpu().numpy()).sum() + (gode * v_ode[0, k].cpu().numpy()).sum())
            assert abs(lhs - rhs) <= 1e-9 * float(np.abs(gy[0] * dy[b, k]).sum()), (b, k, lhs, rhs)


# ------------------------------------------------------------------ 3. / 4. finite differences
def test_rk4_jvp_matches_central_differences(g0):
    import hode
    c = case(g0=g0, B=4, modes=(2, 2, 2))
    sol = solve(c, method=1)
    K = 17 + 6
    v_ode = torch.zeros(1, K, 17, dtype=torch.float64, device="cuda")
    v_x0 = torch.zeros(4, K, 6, dtype=torch.float64, device="cuda")
    for j in range(17):
        v_ode[0, j, j] = 1.0
    for j in range(6):
        v_x0[:, 17 + j, j] = 1.0
    dy = hode.solve_jvp(sol, v_ode, v_x0).cpu().numpy()
    for j in range(K):
        if j < 17:
            h = 1e-5 * abs(c["ode"][j])
            e = np.zeros(17)
            e[j] = h
            yp, ym = solve(c, method=1, ode=c["ode"] + e).y, solve(c, method=1, ode=c["ode"] - e).y
        else:
            h = 1e-5 * max(abs(c["x0"][:, j - 17]).max(), 1.0)
            e = np.zeros(6)
            e[j - 17] = h
            yp, ym = solve(c, method=1, x0=c["x0"] + e).y, solve(c, method=1, x0=c["x0"] - e).y
        fd = ((yp - ym) / (2 * h)).cpu().numpy()
        if np.abs(fd).max() == 0:
            assert np.abs(dy[:, j]).max() == 0, j
            continue
        rel = np.linalg.norm(dy[:, j] - fd) / np.linalg.norm(fd)
        assert rel < 1e-7, (j, rel)


def test_dp5_jvp_matches_differences_of_converged_solutions(g0):
    import hode
    c = case(g0=g0, B=4, modes=(2, 2, 2))
    kw = dict(rtol=1e-10, atol=1e-12, max_steps=4000)
    sol = solve(c, **kw)
    assert int(sol.status.max()) == 0
    idx = [0, 1, 2, 5, 8, 9, 10, 11, 12, 13, 16]
    v_ode = torch.zeros(1, len(idx), 17, dtype=torch.float64, device="cuda")
    for k, j in enumerate(idx):
        v_ode[0, k, j] = 1.0
    dy = hode.solve_jvp(sol, v_ode, None).cpu().numpy()
    def central(j, h):
        e = np.zeros(17)
        e[j] = h
        return ((solve(c, ode=c["ode"] + e, want_tape=False, **kw).y - solve(c, ode=c["ode"] - e, want_tape=False, **kw).y) / (2 * h)).cpu().numpy()
    for k, j in enumerate(idx):
        # Richardson: (4 D(h/2) - D(h)) / 3 cancels the h^2 term, so a step large against the adaptive solver's noise fits
        h = 2e-2 * abs(c["ode"][j])
        fd = (4 * central(j, h / 2) - central(j, h)) / 3
        rel = np.linalg.norm(dy[:, k] - fd) / np.linalg.norm(fd)
        assert rel < 1e-5, (j, rel)


# ------------------------------------------------------------------ 5. rows and failures
def test_rows_follow_y_repeated_times_and_failures(g0):
    import hode
    c = case(g0=g0, B=6, T=9, modes=(2, 2, 2))
    c["t"] = np.array([0., 15., 30., 30., 30., 45., 60., 75., 90.])          # rows 2..4 repeat one time
    sol = solve(c)
    assert int(sol.status.max()) == 0
    v_ode, v_x0 = directions(c, 2, 11)
    dy = hode.solve_jvp(sol, v_ode, v_x0)
    assert torch.equal(dy[:, :, 0], v_x0)
    assert torch.equal(dy[:, :, 3], dy[:, :, 2]) and torch.equal(dy[:, :, 4], dy[:, :, 2])
    assert bool((dy[:, :, 5] != dy[:, :, 4]).any())
    # statuses 1 (step budget), 2 (a state on the pole G = -K_m), 3 (NaN in x0; NaN in a meal row half way)
    x0 = c["x0"].copy()
    x0[1, 0] = -c["ode"][9]
    x0[2, 2] = np.nan
    c["u"][0] = c["u"][0].copy()
    c["u"][0][3, 6] = np.nan
    sol = solve(c, x0=x0)
    st = sol.status.cpu().numpy()
    assert st[1] == 2 and st[2] == 3 and st[3] == 3 and (st[[0, 4, 5]] == 0).all(), st
    dyf = hode.solve_jvp(sol, v_ode, v_x0)
    y = sol.y.cpu().numpy()
    for b in range(6):
        zero_rows = np.all(y[b] == 0, axis=1)
        if st[b] != 0:
            first = int(np.argmax(zero_rows))
            assert first > 0 and zero_rows[first:].all()
            assert bool((dyf[b, :, first:] == 0).all()), b
        assert torch.equal(dyf[b, :, 0], v_x0[b])
    assert bool(torch.isfinite(dyf[[0, 3, 4, 5]]).all())
    assert bool((dyf[3, :, 1:6] != 0).any())
    ok = [0, 4, 5]
    c2 = dict(c, x0=x0[ok], u=[v[ok] for v in c["u"]], B=3)
    assert torch.equal(dyf[ok], hode.solve_jvp(solve(c2), v_ode, v_x0[ok]))
    sol = solve(c, max_steps=3)                                             # status 1
    assert (sol.status.cpu().numpy() == 1).all()
    dyf = hode.solve_jvp(sol, v_ode, v_x0)
    y = sol.y.cpu().numpy()
    for b in range(6):
        first = int(np.argmax(np.all(y[b] == 0, axis=1)))
        assert first > 0 and bool((dyf[b, :, first:] == 0).all()) and bool((dyf[b, :, :first] != 0).any())


# ------------------------------------------------------------------ 6. bits and the tape
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_bits_tiles_linearity_and_read_only_tape(dt, g0):
    import hode
    c = case(g0=g0, B=8, modes=(2, 2, 2), n_sets=2)
    sol = solve(c, dt)
    K = 11
    v_ode, v_x0 = directions(c, K, 21, dt)
    gy = dev(np.random.default_rng(3).standard_normal((8, c["T"], 6)), dt)
    g_before = hode.solve_bwd(sol, gy, want_gnn=True, want_gode=True)
    tape = sol.tape.clone()
    dy = hode.solve_jvp(sol, v_ode, v_x0)
    assert torch.equal(sol.tape, tape)
    assert torch.equal(dy, hode.solve_jvp(sol, v_ode, v_x0))
    for k in range(K):
        assert torch.equal(dy[:, k:k + 1], hode.solve_jvp(sol, v_ode[:, k:k + 1].contiguous(), v_x0[:, k:k + 1].contiguous())), k
    a, b = 0.7, -1.3
    mix = hode.solve_jvp(sol, (a * v_ode[:, :1] + b * v_ode[:, 1:2]).contiguous(), (a * v_x0[:, :1] + b * v_x0[:, 1:2]).contiguous())
    lin = a * dy[:, :1] + b * dy[:, 1:2]
    tol = 1e-5 if dt == torch.float32 else 1e-12
    assert float((mix - lin).norm() / lin.norm()) < tol
    g_after = hode.solve_bwd(sol, gy, want_gnn=True, want_gode=True)
    for x, y in zip(g_before, g_after):
        assert torch.equal(x, y)


def test_no_tape_is_an_error(g0):
    import hode
    sol = solve(case(g0=g0, B=2), want_tape=False)
    with pytest.raises(hode.HodeError):
        hode.solve_jvp(sol, None, torch.zeros(2, 1, 6, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------ 7. the class surface
def test_sensitivities_equal_the_c_abi():
    import hode
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN()
    c = case(B=6, modes=(2, 2, 1))
    x0 = torch.tensor(c["x0"], dtype=torch.float32)
    t = torch.tensor(c["t"], dtype=torch.float32)
    ext = {"meal": torch.tensor(c["u"][0]).float(), "tVNS": torch.tensor(c["u"][1]).float(), "GD": torch.tensor(c["u"][2]).float()}
    wrt = ("a_GI", "V_max", "x0:GLP1", "ode_k_L", "x0:G")
    nn_flat, ode_vec = m._params_on(torch.device("cuda"))
    H, L = m.nn_residual.hidden_dim, m.nn_residual.hip_layers
    for dt in (torch.float32, torch.float64):
        for sets in (None, {"k_I": torch.linspace(0.02, 0.03, 6)}):
            y, S = m.sensitivities(x0, t, ext, wrt=wrt, ode_sets=sets, dtype=dt, max_steps=200)
            n = 6 if sets else 1
            ode = ode_vec.to(dt).repeat(n, 1)
            if sets:
                ode[:, 1] = sets["k_I"].to("cuda", dt)
            sol = hode.solve_fwd(x0.to("cuda", dt), t.to("cuda", dt), *(ext[k].to("cuda", dt) for k in ("meal", "tVNS", "GD")),
                                 ode.reshape(-1).contiguous(), nn_flat.detach().to(dt).repeat(n).contiguous(), H, L, n_sets=n,
                                 want_tape=True, max_steps=200)
            v_ode = torch.zeros(n, 5, 17, dtype=dt, device="cuda")
            v_x0 = torch.zeros(6, 5, 6, dtype=dt, device="cuda")
            v_ode[:, 0, 0] = v_ode[:, 1, 8] = v_ode[:, 3, 10] = 1.0
            v_x0[:, 2, 3] = v_x0[:, 4, 0] = 1.0
            want = hode.solve_jvp(sol, v_ode, v_x0)
            assert torch.equal(y.to("cuda"), sol.y) and torch.equal(S.to("cuda"), want), (dt, sets is None)
            assert bool((S[:, 2, 0, 3] == 1).all()) and bool((S[:, 0, 0] == 0).all())
    with pytest.raises(ValueError):
        m.sensitivities(x0, t, ext, wrt=("x0:nope",))
