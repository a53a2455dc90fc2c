"""GPU tests of the input gradients: d/d{meal, tVNS, GD} of the RHS (K5) and of the solve (K4), through the C ABI
(hode.rhs_bwd_inputs / hode.solve_bwd_inputs) and through the class surface (HybridODENN.forward / ode_residual).

Fixture G10 (tests/golden/g10_input_grads.npz, tools/capture_golden_inputs.py): torch fp64 autograd through the reference's
modules -- (a) ode_residual at random states, (b) a classic RK4 loop with inputs lerped on the grid."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("meal", "tVNS", "GD")
NETS = {"h64l4": (64, 4, 0), "h128l5": (128, 5, 0), "h96l6tanh": (96, 6, 1)}


def relnorm(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_input_grads.npz"))


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.asarray(a)).to("cuda", dt).contiguous()


def net(G, tag, dt=torch.float64):
    import hode
    H, L, act = NETS[tag]
    return dev(G[f"{tag}_nn_flat"], dt), dev(G[f"{tag}_ode"], dt), H, hode.capi.layers(L, act)


# ------------------------------------------------------------------ 1. K5
@pytest.mark.parametrize("tag", list(NETS))
def test_rhs_input_grads_match_reference_autograd(G, tag):
    import hode
    for dt, tol in ((torch.float64, 1e-10), (torch.float32, 1e-5)):
        nn, ode, H, L = net(G, tag, dt)
        a = lambda k: dev(G[f"a_{tag}_{k}"], dt)          # noqa: E731
        gx, gt, gnn, gode, gin = hode.rhs_bwd_inputs(a("x"), a("t"), a("meal"), a("tVNS"), a("GD"), ode, nn, H, L, a("w"),
                                                     want_gnn=False)
        for k in KEYS:
            assert relnorm(gin[k].cpu().numpy(), G[f"a_{tag}_g_{k}"]) < tol, (dt, k)
        # the other outputs are those of rhs_bwd
        gx2, _, _, _ = hode.rhs_bwd(a("x"), a("t"), a("meal"), a("tVNS"), a("GD"), ode, nn, H, L, a("w"), want_gnn=False)
        assert torch.equal(gx, gx2)


def test_rhs_input_grads_match_central_differences(G):
    import hode
    tag = "h64l4"
    nn, ode, H, L = net(G, tag)
    a = lambda k: dev(G[f"a_{tag}_{k}"])                   # noqa: E731
    u = {k: a(k) for k in KEYS}
    w = a("w")
    _, _, _, _, gin = hode.rhs_bwd_inputs(a("x"), a("t"), u["meal"], u["tVNS"], u["GD"], ode, nn, H, L, w, want_gnn=False)
    # (the input terms are ~1e-6 of f: steps large enough that rounding in f does not swamp the difference; meal enters linearly,
    #  the Hill term of GD is smooth on [50, 1050])
    for k, rel_eps in (("meal", 1e-3), ("tVNS", 1e-2), ("GD", 1e-3)):
        eps = rel_eps * float(u[k].abs().max())
        up, dn = dict(u), dict(u)
        up[k], dn[k] = u[k] + eps, u[k] - eps
        f = lambda v: (hode.rhs_fwd(a("x"), a("t"), v["meal"], v["tVNS"], v["GD"], ode, nn, H, L) * w).sum(1)   # noqa: E731
        fd = ((f(up) - f(dn)) / (2 * eps)).cpu().numpy()
        ok = np.abs(gin[k].cpu().numpy() - fd) <= 1e-4 * np.abs(fd) + 1e-12
        # (tVNS: a step of 1e-2 may carry a sample across a ReLU kink of the network -- a few samples, not the rule)
        assert ok.mean() >= (0.9 if k == "tVNS" else 1.0), (k, np.flatnonzero(~ok))


# ------------------------------------------------------------------ 2. K4, RK4 against the fixture
@pytest.mark.parametrize("tag", ["h64l4", "h128l5"])
@pytest.mark.parametrize("mode", ["series", "const"])
def test_rk4_solve_input_grads_match_reference(G, tag, mode):
    import hode
    nn, ode, H, L = net(G, tag)
    b = lambda k: dev(G[f"b_{tag}_{k}"])                   # noqa: E731
    u = {k: b(f"{mode}_{k}") for k in KEYS}
    sol = hode.solve_fwd(b("x0"), b("t"), u["meal"], u["tVNS"], u["GD"], ode, nn, H, L, method=hode.METHOD_RK4, want_tape=True)
    assert int(sol.status.max()) == 0
    assert relnorm(sol.y.cpu().numpy(), G[f"b_{tag}_{mode}_y"]) < 1e-12
    _, _, _, gin = hode.solve_bwd_inputs(sol, b("gy"), want_gnn=False)
    for k in KEYS:
        assert gin[k].shape == u[k].shape
        assert relnorm(gin[k].cpu().numpy(), G[f"b_{tag}_{mode}_g_{k}"]) < 1e-9, k


# ------------------------------------------------------------------ 3./4. DP5(4): finite differences, fp32 against fp64
def _dp5_case(seed=0, B=4, T=13):
    g = np.random.default_rng(seed)
    x0 = np.array([5., 60., 80., 10., 0.5, 1.]) * (1 + 0.1 * g.standard_normal((B, 6)))
    t = np.linspace(0, 3, T)
    u = {"meal": 3 * g.random((B, T)), "tVNS": g.random((B, T)), "GD": 200 + 600 * g.random((B, T))}
    gy = g.standard_normal((B, T, 6))
    return x0, t, u, gy


def test_dp5_directional_derivative_matches_oracle_central_differences(G):
    import hode
    from oracle import oracle as O                         # checker only
    tag = "h64l4"
    nn, ode, H, L = net(G, tag)
    x0, t, u, gy = _dp5_case()
    sol = hode.solve_fwd(dev(x0), dev(t), *(dev(u[k]) for k in KEYS), ode, nn, H, L, rtol=1e-10, atol=1e-12, want_tape=True,
                         max_steps=4000)
    assert int(sol.status.max()) == 0
    _, _, _, gin = hode.solve_bwd_inputs(sol, dev(gy), want_gnn=False)
    rng = np.random.default_rng(1)
    # (tVNS moves J ~1e-5 as much as meal does: a step of 1e-5 would leave the difference to rounding in J)
    for k, rel_eps in (("meal", 1e-5), ("tVNS", 1e-3), ("GD", 1e-5)):
        v = rng.standard_normal(u[k].shape)
        eps = rel_eps * float(np.abs(u[k]).max())

        def J(s):
            w = dict(u)
            w[k] = u[k] + s * eps * v
            r = O.solve(x0, t, w["meal"], w["tVNS"], w["GD"], G[f"{tag}_ode"], G[f"{tag}_nn_flat"].astype(np.float64), H, 4,
                        rtol=1e-10, atol=1e-12, dtype=np.float64)
            return float((r.y * gy).sum())
        fd = (J(1) - J(-1)) / (2 * eps)
        ad = float((gin[k].cpu().numpy() * v).sum())
        # (absolute floor: J ~ 1e2 solved at rtol 1e-10 differs by ~1e-13 from run to run, i.e. ~1e-10 in fd at tVNS's step)
        assert abs(ad - fd) <= 1e-5 * abs(fd) + 1e-9, (k, ad, fd)


@pytest.mark.parametrize("tag", ["h64l4", "h128l5"])
def test_fp32_input_grads_match_fp64(G, tag):
    import hode
    x0, t, u, gy = _dp5_case(seed=3)
    res = {}
    for dt in (torch.float64, torch.float32):
        nn, ode, H, L = net(G, tag, dt)
        sol = hode.solve_fwd(dev(x0, dt), dev(t, dt), *(dev(u[k], dt) for k in KEYS), ode, nn, H, L, want_tape=True)
        assert int(sol.status.max()) == 0
        res[dt] = hode.solve_bwd_inputs(sol, dev(gy, dt), want_gnn=False)[3]
    for k in KEYS:
        assert relnorm(res[torch.float32][k].cpu().numpy(), res[torch.float64][k].cpu().numpy()) < 1e-3, k


# ------------------------------------------------------------------ 5. modes, absent inputs, zero rows
@pytest.mark.parametrize("tag", ["h64l4", "h128l5"])
def test_constant_input_gradient_is_the_row_sum_of_the_series_gradient(G, tag):
    import hode
    nn, ode, H, L = net(G, tag)
    x0, t, u, gy = _dp5_case(seed=5)
    c = {k: u[k][:, 0] for k in KEYS}
    out = {}
    for name, ins in (("const", c), ("series", {k: np.repeat(c[k][:, None], len(t), 1) for k in KEYS})):
        sol = hode.solve_fwd(dev(x0), dev(t), *(dev(ins[k]) for k in KEYS), ode, nn, H, L, want_tape=True)
        out[name] = hode.solve_bwd_inputs(sol, dev(gy), want_gnn=False)[3]
    for k in KEYS:
        a, s = out["const"][k].cpu().numpy(), out["series"][k].sum(1).cpu().numpy()
        assert np.allclose(a, s, rtol=1e-12, atol=1e-12 * np.abs(s).max()), k


def test_absent_and_unwanted_inputs_have_no_gradient(G):
    import hode
    nn, ode, H, L = net(G, "h64l4")
    x0, t, u, gy = _dp5_case()
    sol = hode.solve_fwd(dev(x0), dev(t), dev(u["meal"]), None, None, ode, nn, H, L, want_tape=True)
    gx0, _, _, gin = hode.solve_bwd_inputs(sol, dev(gy))
    assert gin["tVNS"] is None and gin["GD"] is None and gin["meal"].shape == (4, 13)
    sol = hode.solve_fwd(dev(x0), dev(t), *(dev(u[k]) for k in KEYS), ode, nn, H, L, want_tape=True)
    gin = hode.solve_bwd_inputs(sol, dev(gy), want_inputs=("GD",))[3]
    assert gin["meal"] is None and gin["tVNS"] is None and gin["GD"] is not None
    with pytest.raises(hode.HodeError):                  # C ABI: a gradient for an input of mode 0
        fn = getattr(hode.load(), "hode_rhs_bwd_inputs_f64")
        x = dev(x0)
        g = torch.empty(4, dtype=torch.float64, device="cuda")
        P = hode.capi
        P._check(fn(P._stream(), P.C.c_int(4), P._ptr(x), P._ptr(None), P._ptr(None), P._ptr(None), P._ptr(None), P._ptr(ode),
                    P._ptr(nn), P.C.c_int(H), P.C.c_int(L), P._ptr(dev(gy[:, 0])), P._ptr(torch.empty_like(x)), P._ptr(None),
                    P._ptr(None), P._ptr(None), P._ptr(g), P._ptr(None), P._ptr(None)), "hode_rhs_bwd_inputs")


@pytest.mark.parametrize("tag", ["h64l4", "h128l5"])
def test_rows_without_taped_steps_are_zero(G, tag):
    import hode
    nn, ode, H, L = net(G, tag)
    x0, _, u, gy = _dp5_case(seed=7, T=9)
    t = np.array([0., .5, 1., 1., 1., 1.5, 2., 2.5, 3.])          # rows 2..4 repeat one time: row 3 bounds no step
    sol = hode.solve_fwd(dev(x0), dev(t), *(dev(u[k]) for k in KEYS), ode, nn, H, L, want_tape=True)
    assert int(sol.status.max()) == 0
    gin = hode.solve_bwd_inputs(sol, dev(gy), want_gnn=False)[3]
    for k in KEYS:
        g = gin[k].cpu().numpy()
        assert np.isfinite(g).all() and (g[:, 3] == 0).all() and (np.abs(g[:, 2]) > 0).all() and (np.abs(g[:, 4]) > 0).all(), k
    # a failed trajectory (step budget exhausted, status 1): every row from two past its failing interval on is 0
    t = np.linspace(0, 3, 9)
    sol = hode.solve_fwd(dev(x0), dev(t), *(dev(u[k]) for k in KEYS), ode, nn, H, L, rtol=1e-10, atol=1e-12, want_tape=True,
                         max_steps=6)
    st = sol.status.cpu().numpy()
    assert (st == 1).all()
    gin = hode.solve_bwd_inputs(sol, dev(gy), want_gnn=False)[3]
    y = sol.y.cpu().numpy()
    for b in range(4):
        first_zero = int(np.argmax(np.all(y[b] == 0, axis=1)))
        assert first_zero > 0
        for k in KEYS:
            g = gin[k].cpu().numpy()[b]
            assert np.isfinite(g).all() and (g[first_zero + 1:] == 0).all(), (b, k)


@pytest.mark.parametrize("tag", ["h64l4", "h128l5"])
def test_rows_of_underflowed_and_non_finite_trajectories(G, tag):
    """Statuses 2 and 3 (as tests/test_baseline_size_gpu.py makes them): a state ON the pole G = -K_m (step size underflow before any
    step), a NaN in x0 (non-finite at row 0) and a NaN in a meal row (non-finite half way, after rows 0..5).  Every row that bounds no
    taped step is 0, nothing non-finite reaches a gradient, and the healthy neighbours are those of a launch without the failures."""
    import hode
    nn, ode, H, L = net(G, tag)
    x0, t, u, gy = _dp5_case(seed=17, B=6)
    x0[1, 0] = -float(G[f"{tag}_ode"][9])                # G = -K_m
    x0[2, 2] = np.nan
    u = {k: v.copy() for k, v in u.items()}
    u["meal"][3, 6] = np.nan                              # interval 5 cannot be integrated: rows 0..5 are written
    sol = hode.solve_fwd(dev(x0), dev(t), *(dev(u[k]) for k in KEYS), ode, nn, H, L, want_tape=True)
    st = sol.status.cpu().numpy()
    assert st[1] == 2 and st[2] == 3 and st[3] == 3 and (st[[0, 4, 5]] == 0).all(), st
    gin = hode.solve_bwd_inputs(sol, dev(gy), want_gnn=False)[3]
    y = sol.y.cpu().numpy()
    for k in KEYS:
        g = gin[k].cpu().numpy()
        assert np.isfinite(g).all(), k
        assert (g[1] == 0).all() and (g[2] == 0).all(), k        # no taped step at all
        assert (np.abs(y[3, :6]) > 0).any() and (y[3, 6:] == 0).all()
        assert (g[3, 7:] == 0).all() and np.abs(g[3, :6]).max() > 0, k
    ok = [0, 4, 5]
    sol2 = hode.solve_fwd(dev(x0[ok]), dev(t), *(dev(u[k][ok]) for k in KEYS), ode, nn, H, L, want_tape=True)
    gin2 = hode.solve_bwd_inputs(sol2, dev(gy[ok]), want_gnn=False)[3]
    for k in KEYS:
        assert torch.equal(gin[k][ok], gin2[k]), k


# ------------------------------------------------------------------ 6. the other gradients stay intact
@pytest.mark.parametrize("tag", ["h64l4", "h128l5"])
def test_other_gradients_unchanged_and_deterministic(G, tag):
    import hode
    x0, t, u, gy = _dp5_case(seed=9, B=64)
    for dt in (torch.float64, torch.float32):
        nn, ode, H, L = net(G, tag, dt)
        sol = hode.solve_fwd(dev(x0, dt), dev(t, dt), *(dev(u[k], dt) for k in KEYS), ode, nn, H, L, want_tape=True)
        ref = hode.solve_bwd(sol, dev(gy, dt), want_gode=True)
        r1 = hode.solve_bwd_inputs(sol, dev(gy, dt), want_gode=True)
        r2 = hode.solve_bwd_inputs(sol, dev(gy, dt), want_gode=True)
        # gx0 and the input gradients are written per trajectory: the same bits run to run.  gnn / gode: the tuned kernels sum in a
        # fixed order (bitwise); the fp64 generic kernels add them with atomics (include/hode.h), equal to rounding only
        exact = tag == "h64l4"
        assert torch.equal(r1[0], r2[0])
        for k in KEYS:
            assert torch.equal(r1[3][k], r2[3][k])
        for i, (a, b) in enumerate(zip(r1[:3], ref)):
            if dt == torch.float64 and (i == 0 or exact):
                assert torch.equal(a, b) and torch.equal(r2[i], b), i
            else:
                assert relnorm(a.cpu().numpy(), b.cpu().numpy()) < (1e-12 if dt == torch.float64 else 1e-5), i


# ------------------------------------------------------------------ 7. class surface
def _model(M, G, tag="h64l4"):
    H, L, _ = NETS[tag]
    torch.manual_seed(0)
    m = M.HybridODENN(nn_hidden=H, nn_layers=L, device="cuda")
    with torch.no_grad():
        flat = torch.as_tensor(G[f"{tag}_nn_flat"])
        off = 0
        for p in m.nn_residual.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        for n, v in zip(["a_GI", "k_I", "rho", "G_b", "I_b", "E_max", "EC_50", "Glu_b", "V_max", "K_m", "k_L", "k_GE0", "IGD_50",
                         "g", "p_7", "p_8", "p_9"], G[f"{tag}_ode"]):
            getattr(m.ode_core, n).fill_(float(v))
    return m


@pytest.fixture(scope="module")
def M():
    import models
    return models


def test_forward_fills_input_grads_like_the_c_abi(M, G):
    import hode
    m = _model(M, G)
    x0, t, u, gy = _dp5_case(seed=11)
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")   # noqa: E731
    ins = {"meal": f32(u["meal"]).requires_grad_(True), "tVNS": f32(u["tVNS"][:, 0]).requires_grad_(True),
           "GD": f32(u["GD"]).requires_grad_(True)}
    y = m(f32(x0), f32(t), ins)
    (y * f32(gy)).sum().backward()
    nn, ode = m._params_on(torch.device("cuda"))
    sol = hode.solve_fwd(f32(x0), f32(t), ins["meal"].detach(), ins["tVNS"].detach(), ins["GD"].detach(), ode.detach(),
                         nn.detach(), 64, 4, want_tape=True)
    gin = hode.solve_bwd_inputs(sol, f32(gy), want_gnn=False)[3]
    for k in KEYS:
        assert ins[k].grad is not None and ins[k].grad.shape == ins[k].shape
        assert relnorm(ins[k].grad.cpu().numpy(), gin[k].cpu().numpy()) < 1e-5, k
    # only one input wanted; a 0-dim input broadcast by the class
    g0 = torch.tensor(400.0, device="cuda", requires_grad=True)
    y = m(f32(x0), f32(t), {"meal": f32(u["meal"]), "GD": g0})
    (y * f32(gy)).sum().backward()
    assert g0.grad is not None and torch.isfinite(g0.grad) and float(g0.grad) != 0


def test_ode_residual_input_grads_match_fixture(M, G):
    m = _model(M, G)
    tag = "h64l4"
    f32 = lambda k: torch.as_tensor(G[f"a_{tag}_{k}"], dtype=torch.float32, device="cuda")   # noqa: E731
    u = {k: f32(k).requires_grad_(True) for k in KEYS}
    (m.ode_residual(f32("t"), f32("x"), u) * f32("w")).sum().backward()
    for k in KEYS:
        assert relnorm(u[k].grad.cpu().numpy(), G[f"a_{tag}_g_{k}"]) < 1e-4, k


def test_chunked_backward_input_grads_equal_one_launch(M, G, monkeypatch):
    import hode
    import models.hybrid_ode_nn as HN
    m = _model(M, G)
    x0, t, u, gy = _dp5_case(seed=13, B=8)
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")   # noqa: E731
    per = hode.capi.tape_nbytes(1, 12 + 32, 4, 4)

    def grads(budget):
        monkeypatch.setattr(HN, "TAPE_BUDGET_BYTES", budget)
        ins = {"meal": f32(u["meal"]).requires_grad_(True), "tVNS": f32(u["tVNS"][:, 0]).requires_grad_(True),
               "GD": f32(u["GD"]).requires_grad_(True)}
        y = m(f32(x0), f32(t), ins)
        (y * f32(gy)).sum().backward()
        return [ins[k].grad.clone() for k in KEYS]

    launches = []
    bwd = hode.solve_bwd_inputs
    monkeypatch.setattr(hode, "solve_bwd_inputs", lambda sol, *a, **k: launches.append(sol.y.shape[0]) or bwd(sol, *a, **k))
    one = grads(64 << 30)
    assert launches == [8]                                 # one adjoint over the batch
    launches.clear()
    # a budget of three 44-step tapes: the class tapes these 8 patients with more steps per trajectory, so the re-integration runs in
    # chunks smaller than three patients -- the chunked backward, as the launch count shows
    chunked = grads(3 * per)
    assert len(launches) > 1 and sum(launches) == 8 and max(launches) < 8, launches
    for a, b in zip(one, chunked):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 8. end to end: meal amplitudes from glucose
def test_recover_meal_amplitudes_from_glucose(M, G):
    m = _model(M, G)
    B, T = 256, 37
    g = torch.Generator().manual_seed(0)
    t = torch.linspace(0, 3, T, device="cuda")
    shape = torch.zeros(T)
    shape[6:10] = torch.tensor([0.5, 1.0, 1.0, 0.5])         # a meal pulse on the grid, amplitude per patient
    shape = shape.cuda()
    x0 = (torch.tensor([5., 60., 80., 10., 0.5, 1.]) * (1 + 0.05 * torch.randn(B, 6, generator=g))).cuda()
    true = (2 + 4 * torch.rand(B, generator=g)).cuda()
    with torch.no_grad():
        obs = m(x0, t, {"meal": true[:, None] * shape})[..., 0]
    amp = torch.full((B,), 4.0, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([amp], lr=0.1)
    first = None
    for it in range(300):
        opt.zero_grad()
        y = m(x0, t, {"meal": amp[:, None] * shape})
        loss = ((y[..., 0] - obs) ** 2).mean()
        loss.backward()
        opt.step()
        if first is None:
            first = float(loss.detach())
    final = float(((m(x0, t, {"meal": amp.detach()[:, None] * shape})[..., 0] - obs) ** 2).mean())
    assert final < first / 100, (first, final)
    err = float(((amp.detach() - true).abs() / true).max())
    assert err < 0.05, err
