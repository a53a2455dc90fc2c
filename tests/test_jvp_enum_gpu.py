"""GPU tests: the tangent-linear solve (hode.solve_jvp, csrc/hode_solve_jvp.hip) against the C oracle's hode_oracle_solve_jvp on the
cases of tests/_jvp_cases.py, column by column -- one parametrised test per part of the table (its docstring has the parts, the
directions, the figures, the bounds and the measured error ratios).  Each test: solve_fwd(want_tape) + solve_jvp, the oracle on the
same arrays, status / nsteps equal to the oracle's at the same dtype, every direction against the fp64 oracle, structural zeros and
row 0 with ==.  tests/test_jvp_oracle.py pins the oracle's tangent and admits the cases on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _input_grad_cases as IC
import _jvp_cases as JC
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
    c = JC.find(part, name)
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
    """One launch against the oracle on the same directions (each parameter set with its own v_ode).  fp64, unit directions: per
    (direction, state component); otherwise per direction in the scaled norm; fp32 within MARGIN x d_ref, capped."""
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
        tol = JC.tolerance(part, c["method"], dt, d_ref)
        print(f"FIGURE {label} {name} err {err:.3e} d_ref {d_ref:.3e} ratio {err / d_ref if d_ref else float('nan'):.2f} tol {tol:.3e}")
        if not err <= tol:
            bad.append(f"{label} {name}: err {err:.3e} > tol {tol:.3e} (d_ref {d_ref:.3e})")
    return got, r64


@pytest.mark.parametrize("c,dt", JC.params(JC.CASES["a"]), ids=JC.ids(JC.CASES["a"]))
def test_a_every_instantiation_unit_columns(c, dt):
    assert c["H"] <= 64 and c["L"] <= 4 and c["act"] == IC.RELU
    d, s64, sdt, sol, label = _start("a", c, dt)
    v_ode, v_x0 = JC.unit_directions(c)
    bad = []
    dy = _launch(sol, dt, v_ode, v_x0)
    _compare("a", label, c, dt, dy, v_ode, v_x0, s64, sdt, bad, unit=True)
    # bits: direction 8 = slot 0 of the second fp32 tile, direction 22 = the last live slot of the ragged third tile
    for k in (8, 22):
        one = _launch(sol, dt, v_ode[:, k:k + 1], v_x0[:, k:k + 1])
        if not torch.equal(dy[:, k:k + 1], one):
            bad.append(f"{label} {JC.DIR_NAMES[k]}: the K = 23 launch and the K = 1 launch differ in bits")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c,dt", JC.params(JC.CASES["c"]), ids=JC.ids(JC.CASES["c"]))
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
    if c["n_sets"] > 1:
        # (the dense v_ode differs per set: _compare ran every set's trajectories against the oracle with THAT set's v_ode)
        vo = JC.dense_directions(c, d, JC.K_DENSE_C)[0]
        assert not np.array_equal(vo[0], vo[1]) and not np.array_equal(vo[1], vo[2])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c,dt", JC.params(JC.CASES["k"]), ids=JC.ids(JC.CASES["k"]))
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


@pytest.mark.parametrize("c,dt", JC.params(JC.CASES["e"]), ids=JC.ids(JC.CASES["e"]))
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
