"""GPU tests: the tangent-linear solve of GENERIC networks (hode.solve_jvp -> hode_solve_jvp_any_*, csrc/hode_generic_jvp.hip) against
the C oracle's hode_oracle_solve_jvp on the cases of tests/_jvp_generic_cases.py (its docstring has the parts, the bounds and the
measured ratios), and through every layer above it: tapes of each forward team kernel, duality with the generic adjoint, the read-only
tape, HybridODENN.sensitivities and inference.fit_patients.  tests/test_jvp_generic_host.py admits the cases on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _input_grad_cases as IC
import _jvp_cases as JC
import _jvp_generic_cases as GC
from _input_grad_cases import relnorm

pytestmark = pytest.mark.gpu

TORCH_DT = {"f64": torch.float64, "f32": torch.float32}


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.asarray(a)).to("cuda", TORCH_DT[dt]).contiguous()


def host(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O                          # checker only
    return O


@functools.lru_cache(maxsize=None)
def _tapes(part, name, dt):
    """(data, the fp64 oracle's tapes at the solver tolerances of dtype dt, the oracle's tapes at dt) -- once per case and dtype."""
    c = GC.find(part, name)
    d = IC.solve_data(c)
    s64 = JC.oracle_tapes(_oracle(), c, "f64", d, tols_of=dt)
    return d, s64, (s64 if dt == "f64" else JC.oracle_tapes(_oracle(), c, "f32", d))


def _forward(c, dt, d):
    import hode
    tol = IC.solver_tols(c, dt)
    return hode.solve_fwd(dev(d["x0"], dt), dev(d["t"], dt), *(dev(v, dt) for v in d["u"]), dev(d["ode"], dt), dev(d["nn"], dt), c["H"],
                          IC.layers(c["L"], c["act"]), method=c["method"], rtol=tol["rtol"], atol=tol["atol"], max_steps=c["max_steps"],
                          n_sets=c["n_sets"], want_tape=True)


def _start(part, c, dt):
    """The kernel's forward with tape, checked against the oracle's at the same dtype."""
    assert not (c["H"] <= 64 and c["L"] <= 4 and c["act"] == IC.RELU)              # a generic shape
    d, s64, sdt = _tapes(part, c["name"], dt)
    sol = _forward(c, dt, d)
    st, ns = JC.status_nsteps(sdt)
    label = f"{part}/{c['name']}-{dt}"
    assert np.array_equal(host(sol.status), st) and (st == c["expect_status"]).all(), (label, host(sol.status), st)
    assert np.array_equal(host(sol.nsteps), ns), (label, host(sol.nsteps), ns)
    return d, s64, sdt, sol, label


def _launch(sol, dt, v_ode, v_x0):
    import hode
    return hode.solve_jvp(sol, dev(v_ode, dt), dev(v_x0, dt))


def _compare(part, label, c, dt, dy, v_ode, v_x0, s64, sdt, bad, unit):
    """One launch against the oracle on the same directions (each parameter set with its own v_ode): the logic of
    tests/test_jvp_enum_gpu.py's _compare with this table's margins.  fp64, unit directions: per (direction, state component);
    otherwise per direction in the scaled norm; fp32 within MARGIN x d_ref, capped."""
    O = _oracle()
    got = host(dy)
    r64 = JC.oracle_jvp(O, c, s64, v_ode, v_x0)
    rdt = r64 if dt == "f64" else JC.oracle_jvp(O, c, sdt, v_ode, v_x0)
    assert got.shape == r64.shape, (label, got.shape, r64.shape)
    if not np.isfinite(got).all():
        bad.append(f"{label}: non-finite tangents")
        return got, r64
    want0 = np.zeros_like(got[:, :, 0]) if v_x0 is None else np.asarray(v_x0, got.dtype)
    if not np.array_equal(got[:, :, 0], want0):
        bad.append(f"{label}: row 0 is not v_x0")
    for k in range(got.shape[1]):
        name = JC.DIR_NAMES[k] if unit else f"dir{k}"
        if np.abs(r64[:, k]).max() == 0:                    # IGD_50 and g without GD
            if np.abs(got[:, k]).max() != 0:
                bad.append(f"{label} {name}: the reference is identically 0, the kernel's largest entry is {np.abs(got[:, k]).max():.3e}")
            continue
        if dt == "f64" and unit:
            for comp in range(6):
                ref = r64[:, k, :, comp]
                if np.abs(ref).max() == 0:
                    if np.abs(got[:, k, :, comp]).max() != 0:
                        bad.append(f"{label} {name}[{comp}]: the reference is identically 0, the kernel is not")
                    continue
                err, tol = relnorm(got[:, k, :, comp], ref), IC.FP64_TOL[c["method"]]
                print(f"FIGURE {label} {name}[{comp}] err {err:.3e} tol {tol:.3e}")
                if not err <= tol:
                    bad.append(f"{label} {name}[{comp}]: err {err:.3e} > tol {tol:.3e}")
            continue
        err = JC.scaled_norm(got[:, k], r64[:, k])
        d_ref = JC.scaled_norm(rdt[:, k], r64[:, k]) if dt == "f32" else 0.0
        tol = GC.tolerance(part, c["method"], dt, d_ref)
        print(f"FIGURE {label} {name} err {err:.3e} d_ref {d_ref:.3e} ratio {err / d_ref if d_ref else float('nan'):.2f} tol {tol:.3e}")
        if not err <= tol:
            bad.append(f"{label} {name}: err {err:.3e} > tol {tol:.3e} (d_ref {d_ref:.3e})")
    return got, r64


# ------------------------------------------------------------------ parts g / c / k / e against the oracle
@pytest.mark.parametrize("c,dt", JC.params(GC.CASES["g"]), ids=JC.ids(GC.CASES["g"]))
def test_g_every_generic_shape_unit_columns(c, dt):
    d, s64, sdt, sol, label = _start("g", c, dt)
    v_ode, v_x0 = JC.unit_directions(c)
    bad = []
    dy = _launch(sol, dt, v_ode, v_x0)
    _compare("g", label, c, dt, dy, v_ode, v_x0, s64, sdt, bad, unit=True)
    # bits: direction 8 = slot 0 of the second fp32 tile, direction 22 = the last live slot of the ragged third tile
    for k in (8, 22):
        one = _launch(sol, dt, v_ode[:, k:k + 1], v_x0[:, k:k + 1])
        if not torch.equal(dy[:, k:k + 1], one):
            bad.append(f"{label} {JC.DIR_NAMES[k]}: the K = 23 launch and the K = 1 launch differ in bits")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c,dt", JC.params(GC.CASES["c"]), ids=JC.ids(GC.CASES["c"]))
def test_c_row_bookkeeping_edges(c, dt):
    d, s64, sdt, sol, label = _start("c", c, dt)
    bad = []
    for tag, (v_ode, v_x0) in (("unit", JC.unit_directions(c)), (f"dense{JC.K_DENSE_C}", JC.dense_directions(c, d, JC.K_DENSE_C))):
        dy = _launch(sol, dt, v_ode, v_x0)
        _compare("c", f"{label}-{tag}", c, dt, dy, v_ode, v_x0, s64, sdt, bad, unit=tag == "unit")
        if c["grid"] is not None:                           # repeated times: bit copies of the row before
            t = d["t"]
            for r in range(1, len(t)):
                if not t[r] > t[r - 1] and not torch.equal(dy[:, :, r], dy[:, :, r - 1]):
                    bad.append(f"{label}-{tag}: row {r} repeats the time of row {r - 1} and is not a copy of it")
            if not bool((dy[:, :, 3] != dy[:, :, 2]).any()):
                bad.append(f"{label}-{tag}: rows 2 and 3 are of different times and equal")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c,dt", JC.params(GC.CASES["k"]), ids=JC.ids(GC.CASES["k"]))
def test_k_direction_tiling_and_pointers(c, dt):
    d, s64, sdt, sol, label = _start("k", c, dt)
    bad = []
    launches = {}
    for K in JC.K_TILING:
        v_ode, v_x0 = JC.dense_directions(c, d, K)
        launches[K] = _launch(sol, dt, v_ode, v_x0)
        _compare("k", f"{label}-K{K}", c, dt, launches[K], v_ode, v_x0, s64, sdt, bad, unit=False)
    # launches with different K share their leading directions: bit for bit
    for K in JC.K_TILING:
        for K2 in JC.K_TILING:
            if K < K2 and not torch.equal(launches[K], launches[K2][:, :K]):
                bad.append(f"{label}: the first {K} directions of the K = {K2} launch differ in bits from the K = {K} launch")
    v_ode, v_x0 = JC.dense_directions(c, d, JC.K_POINTERS)
    for tag, vo, vx in (("ode-only", v_ode, None), ("x0-only", None, v_x0)):
        dy = _launch(sol, dt, vo, vx)
        _compare("k", f"{label}-{tag}", c, dt, dy, vo, vx, s64, sdt, bad, unit=False)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c,dt", JC.params(GC.CASES["e"]), ids=JC.ids(GC.CASES["e"]))
def test_e_failed_trajectory(c, dt):
    d, s64, sdt, sol, label = _start("e", c, dt)
    assert (host(sol.status) == 1).all() and (host(sol.nsteps) == c["max_steps"]).all()
    v_ode, v_x0 = JC.unit_directions(c)
    bad = []
    dy = _launch(sol, dt, v_ode, v_x0)
    got, r64 = _compare("e", label, c, dt, dy, v_ode, v_x0, s64, sdt, bad, unit=True)
    last = JC.last_written_row(sdt[0], dt, d["t"])
    y = host(sol.y)
    for b in range(c["B"]):
        assert 1 <= last[b] < c["T"] - 1, (b, last[b])
        if not ((got[b, :, last[b] + 1:] == 0).all() and (y[b, last[b] + 1:] == 0).all()):
            bad.append(f"{label}: trajectory {b}: rows after row {last[b]} (the last one a taped step closed) are not exactly 0")
        if not (np.abs(got[b, 0, last[b]]).max() > 0 and (y[b, last[b]] != 0).all()):
            bad.append(f"{label}: trajectory {b}: row {last[b]} was closed by a taped step and is 0")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ tapes from every forward team kernel
def test_tangent_does_not_depend_on_which_team_kernel_taped_the_trajectory(golden_dir, g0):
    """B = 600 / 300 / 5: the forward's four-wave streamed, two-trajectory resident and one-trajectory resident team kernels (the recipe
    of test_team_kernels_of_the_forward_agree_with_each_other_and_the_oracle at 100 x 3), fp32, K = 3 dense, under both methods: a
    sub-batch solved and differentiated on its own gives the rows of the big launch bit for bit."""
    import os

    import hode
    from test_generic_gpu import net
    O = _oracle()
    H, L, K = 100, 3, 3
    g = np.load(os.path.join(golden_dir, "g4_t61_pulses.npz"))
    sel = np.arange(0, 61, 5)
    t = g["t"][sel].astype(np.float64)
    nn, ode = net(H, L, seed=3), g0["ode"].astype(np.float64)
    B = 600
    rng = np.random.default_rng(H)
    x0 = g["x0"][rng.integers(0, 8, B)] * (1 + 0.02 * rng.standard_normal((B, 6)))
    meal, tv = g["meal"][rng.integers(0, 8, B)][:, sel], np.zeros((B, sel.size))
    v_ode = rng.standard_normal((1, K, 17)) * np.abs(ode).reshape(1, 1, 17)
    v_x0 = rng.standard_normal((B, K, 6)) * JC.SCALE

    def run(sub, method):
        sol = hode.solve_fwd(dev(x0[sub], "f32"), dev(t, "f32"), dev(meal[sub], "f32"), dev(tv[sub], "f32"), None, dev(ode, "f32"),
                             dev(nn, "f32"), H, L, method=method, want_tape=True)
        assert int(sol.status.max()) == 0
        return sol, hode.solve_jvp(sol, dev(v_ode, "f32"), dev(v_x0[sub], "f32"))
    for method in (IC.DP5, IC.RK4):
        big, dy = run(slice(0, B), method)
        for n_small in (5, 300):
            sub = slice(17, 17 + n_small)
            small, dys = run(sub, method)
            assert torch.equal(small.y, big.y[sub]) and torch.equal(dys, dy[sub]), (method, n_small)
    # Every direction tile of the launch rule (csrc/hode_generic_jvp.hip launch_solve_jvp_generic: fp32 tiles of 8 / 4 / 2 / 1 by B and
    # K) carries a direction to the same bits: 600 x 9 rides in tiles of 8, 600 x 3 (above) of 4, 600 x 2 of 2, 5 x 9 of 1.
    vo9 = np.concatenate([v_ode, rng.standard_normal((1, 6, 17)) * np.abs(ode).reshape(1, 1, 17)], 1)
    vx9 = np.concatenate([v_x0, rng.standard_normal((B, 6, 6)) * JC.SCALE], 1)
    jvp = lambda sol, sub, k: hode.solve_jvp(sol, dev(vo9[:, :k], "f32"), dev(vx9[sub, :k], "f32"))      # noqa: E731
    dy9 = jvp(big, slice(0, B), 9)
    assert torch.equal(dy9[:, :3], dy) and torch.equal(jvp(big, slice(0, B), 2), dy[:, :2])
    assert torch.equal(jvp(small, sub, 9), dy9[sub])
    sub = slice(17, 22)
    small, _ = run(sub, IC.RK4)
    assert torch.equal(jvp(small, sub, 9), dy9[sub])
    # The first 6 trajectories against the fp64 oracle, within the part-g bound -- of the RK4 launch.  Under DP5(4) this recipe (a
    # 0..240 grid, the gain-0.5 network) is not admissible: the oracle's own fp32 tangent is 4e-5 .. 4e-4 from its fp64 one at
    # IC.FP32_DP5_TOL (equal step counts) and the step counts differ at the default tolerances; under RK4 d_ref is 5e-8 .. 1e-7.
    kw = dict(method=IC.RK4, max_steps=int(big.max_steps), want_tape=True)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)                   # noqa: E731  (what the kernel was given)
    args = (f32(x0[:6]), f32(t), f32(meal[:6]), f32(tv[:6]), None, f32(ode), f32(nn), H, L)
    s64, s32 = O.solve(*args, dtype=np.float64, **kw), O.solve(*args, dtype=np.float32, **kw)
    assert np.array_equal(s64.nsteps, s32.nsteps) and np.array_equal(host(big.nsteps[:6]), s32.nsteps)
    r64, r32 = O.solve_jvp(s64, f32(v_ode[0]), f32(v_x0[:6])), O.solve_jvp(s32, f32(v_ode[0]), f32(v_x0[:6]))
    got = host(dy[:6])
    for k in range(K):
        d_ref = JC.scaled_norm(r32[:, k], r64[:, k])
        assert d_ref <= IC.FP32_CAP[IC.RK4] / 8, (k, d_ref)
        err = JC.scaled_norm(got[:, k], r64[:, k])
        print(f"FIGURE teams dir{k} err {err:.3e} d_ref {d_ref:.3e} ratio {err / d_ref:.2f}")
        assert err <= GC.tolerance("g", IC.RK4, "f32", d_ref), (k, err, d_ref)


# ------------------------------------------------------------------ duality with the generic adjoint
@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("j", range(len(IC.GENERIC_SHAPES)), ids=[f"h{H}l{L}{IC.ACT_NAME[a]}" for H, L, a in IC.GENERIC_SHAPES])
def test_jvp_is_the_transpose_of_the_generic_adjoint_fp64(j, n_sets):
    import hode
    c = dict(GC.CASES["g"][2 * j], n_sets=n_sets, B=6 if n_sets == 3 else 5)
    d = IC.solve_data(c)
    sol = _forward(c, "f64", d)
    assert int(sol.status.max()) == 0
    K = 3
    v_ode, v_x0 = (dev(v, "f64") for v in JC.dense_directions(c, d, K))
    dy = hode.solve_jvp(sol, v_ode, v_x0)
    gy = dev(d["gy"], "f64")
    gx0, _, gode = hode.solve_bwd(sol, gy, want_gnn=False, want_gode=True)
    gode = gode.view(n_sets, 17)
    per = c["B"] // n_sets
    for k in range(K):
        lhs = gy * dy[:, k]
        r0 = gx0 * v_x0[:, k]
        r1 = gode * v_ode[:, k] * 1.0
        scale = float(lhs.abs().sum() + r0.abs().sum() + r1.abs().sum())
        err = abs(float(lhs.sum() - r0.sum() - r1.sum()))
        assert err <= 1e-11 * scale, (c["name"], k, err / scale)
    assert per * n_sets == c["B"]


# ------------------------------------------------------------------ read-only and repeatable
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_tape_is_read_only_and_the_call_repeats_its_bits(dt):
    import hode
    c = GC.find("c", "g100x3-sets3x3")
    d = IC.solve_data(c)
    sol = _forward(c, dt, d)
    v_ode, v_x0 = JC.dense_directions(c, d, JC.K_DENSE_C)
    gy = dev(d["gy"], dt)
    before = hode.solve_bwd(sol, gy, want_gnn=True, want_gode=True)
    tape0 = sol.tape.clone()
    a = _launch(sol, dt, v_ode, v_x0)
    assert torch.equal(sol.tape, tape0)
    b = _launch(sol, dt, v_ode, v_x0)
    assert torch.equal(a, b)
    after = hode.solve_bwd(sol, gy, want_gnn=True, want_gode=True)
    if dt == "f32":                                         # (the fp32 team adjoint is deterministic; fp64 adds with atomics)
        for x, y in zip(before, after):
            assert torch.equal(x, y)
    else:
        assert torch.equal(before[0], after[0])


# ------------------------------------------------------------------ the class surface
def _elu_model():
    import models as M
    m = M.HybridODENN(nn_hidden=40, nn_layers=2, device="cuda")
    m.nn_residual = M.NNResidual(9, 40, 6, 2, activation="elu").cuda()
    return m


@pytest.mark.parametrize("which", ["h128l5relu", "h40l2elu"])
def test_sensitivities_of_a_generic_network_equal_the_c_abi(which):
    import hode
    from models.hybrid_ode_nn import HybridODENN
    from test_jvp_gpu import case
    torch.manual_seed(0)
    m = HybridODENN(nn_hidden=128, nn_layers=5) if which == "h128l5relu" else _elu_model()
    c = case(B=6, T=13, modes=(2, 2, 1))
    x0 = torch.tensor(c["x0"], dtype=torch.float32)
    t = torch.tensor(c["t"], dtype=torch.float32)
    ext = {"meal": torch.tensor(c["u"][0]).float(), "tVNS": torch.tensor(c["u"][1]).float(), "GD": torch.tensor(c["u"][2]).float()}
    wrt = ("a_GI", "V_max", "x0:GLP1", "ode_k_L", "x0:G")
    nn_flat, ode_vec = m._params_on(torch.device("cuda"))
    H, L = m.nn_residual.hidden_dim, m.nn_residual.hip_layers
    assert not (H <= 64 and (L & 0xff) <= 4 and (L >> 8) == 0)
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
            assert int(sol.status.max()) == 0
            v_ode = torch.zeros(n, 5, 17, dtype=dt, device="cuda")
            v_x0 = torch.zeros(6, 5, 6, dtype=dt, device="cuda")
            v_ode[:, 0, 0] = v_ode[:, 1, 8] = v_ode[:, 3, 10] = 1.0
            v_x0[:, 2, 3] = v_x0[:, 4, 0] = 1.0
            want = hode.solve_jvp(sol, v_ode, v_x0)
            assert torch.equal(y.to("cuda"), sol.y) and torch.equal(S.to("cuda"), want), (dt, sets is None)
            assert bool((S[:, 2, 0, 3] == 1).all()) and bool((S[:, 0, 0] == 0).all())
            assert bool(torch.isfinite(S).all()) and float(S[:, 0, -1].abs().max()) > 0


def _tanh_model(H, L, nn, ode):
    """A HybridODENN whose residual is the tanh H x L network `nn` (flat, fp32-representable) and whose constants are `ode`."""
    import models as M
    m = M.HybridODENN(ode_params={n: float(v) for n, v in zip(JC.ODE_NAMES, ode)}, nn_hidden=H, nn_layers=L, device="cuda")
    m.nn_residual = M.NNResidual(9, H, 6, L, activation="tanh").cuda()
    flat, off = torch.tensor(nn, dtype=torch.float32), 0
    with torch.no_grad():
        for p in m.nn_residual.parameters():
            p.copy_(flat[off:off + p.numel()].reshape(p.shape))
            off += p.numel()
    assert off == flat.numel()
    nn_flat, ode_vec = m._params_on(torch.device("cuda"))
    assert np.array_equal(host(nn_flat.detach().double()), nn) and np.array_equal(host(ode_vec.double()), ode)
    return m


def test_sensitivities_match_central_differences_of_forward_rk4_fp64():
    c = GC.fd_case()
    F = GC.FD
    m = _tanh_model(F["H"], F["L"], c["nn"], c["ode"])
    x0, t, ext = torch.tensor(c["x0"]), torch.tensor(c["t"]), {"meal": torch.tensor(c["meal"])}
    wrt = JC.ODE_NAMES + tuple(f"x0:{s}" for s in ("G", "I", "Glu", "GLP1", "GE", "FFA"))
    kw = dict(solver="rk4", dtype=torch.float64)

    def fwd(ode=None, xs=None):
        sets = None if ode is None else {n: torch.full((F["B"],), float(v), dtype=torch.float64) for n, v in zip(JC.ODE_NAMES, ode)}
        y, _ = m.sensitivities(x0 if xs is None else torch.tensor(xs), t, ext, wrt=("a_GI",), ode_sets=sets, **kw)
        return host(y.double())
    y, S = m.sensitivities(x0, t, ext, wrt=wrt, **kw)
    S = host(S.double())
    assert np.isfinite(S).all()
    bad = []
    for j in range(JC.K_UNIT):
        if j < 17:
            h = F["rel_step"] * abs(c["ode"][j])
            e = np.zeros(17)
            e[j] = h
            fd = (fwd(ode=c["ode"] + e) - fwd(ode=c["ode"] - e)) / (2 * h)
        else:
            h = F["rel_step"] * max(np.abs(c["x0"][:, j - 17]).max(), 1.0)
            e = np.zeros(6)
            e[j - 17] = h
            # (x0 passes through fp32 on its way in: the step is taken on the fp32 grid, each patient divided by its own)
            xp, xm = np.float32(c["x0"] + e).astype(np.float64), np.float32(c["x0"] - e).astype(np.float64)
            assert ((xp - xm)[:, j - 17] > h).all()
            fd = (fwd(xs=xp) - fwd(xs=xm)) / (xp - xm)[:, j - 17].reshape(-1, 1, 1)
        if np.abs(fd).max() == 0:
            assert j in JC.GD_ONLY and np.abs(S[:, j]).max() == 0, j
            continue
        err = JC.scaled_norm(S[:, j], fd)
        print(f"FIGURE fd {JC.DIR_NAMES[j]} err {err:.3e}")
        if not err <= F["bound_gpu"]:
            bad.append(f"{JC.DIR_NAMES[j]}: {err:.3e}")
    assert not bad, bad


# ------------------------------------------------------------------ calibration
def test_fit_patients_recovers_the_constants_of_a_generic_network():
    from inference import fit_patients
    C, c = GC.CAL, GC.calibration_case()
    obs = GC.calibration_observations(_oracle())
    m = _tanh_model(C["H"], C["L"], c["nn"], c["ode"])
    batch = {"initial_state": torch.tensor(c["x0"]), "time_points": torch.tensor(c["t"]), "observations": torch.tensor(obs),
             "external_inputs": {"meal": torch.tensor(c["meal"])}}
    res = fit_patients(m, batch, params=GC.CAL_NAMES, priors=None, noise_sigma=C["sigma"], max_iter=100, rtol=C["rtol"], atol=C["atol"],
                       max_steps=C["max_steps"])
    assert (host(res.status) == 0).all(), host(res.status)
    for n in GC.CAL_NAMES:
        rel = np.abs(host(res.params[n]) - c["truth"][n]) / np.abs(c["truth"][n])
        print(f"FIGURE calibration {n} rel {rel.max():.3e}")
        assert rel.max() <= C["bound_gpu"], (n, rel)
    std = host(res.std)
    assert np.isfinite(std).all() and (std > 0).all()
