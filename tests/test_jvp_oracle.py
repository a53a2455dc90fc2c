"""CPU tests of the oracle's tangent-linear solve (oracle/hode_oracle_impl.h: hode_oracle_solve_jvp_*) and the admission of every
case of tests/_jvp_cases.py, from the oracle alone.

1. duality with the oracle's adjoint on the same tape, <gy, dy> = <gx0, v_x0> + <gode, v_ode>, fp64, every case and direction set,
   1e-12 of the sum of the absolute terms;
2. finite differences: RK4 unit columns against central differences of the oracle's own forward (exact for the discrete map),
   DP5(4) against Richardson differences of converged solutions -- steps and bounds of tests/test_jvp_gpu.py;
3. rows: the grid with repeated times against the grid without them, the rows after a failure;
4. admission: what a case must satisfy before the kernel is compared on it, and the coverage of the table;
5. the sanitizer self-check program of oracle/Makefile."""
import os
import subprocess

import numpy as np
import pytest

import _input_grad_cases as IC
import _jvp_cases as JC
from _input_grad_cases import relnorm
from test_jvp_gpu import case as gpu_case               # the recipe of the existing finite-difference tests (numpy only)

PARTS = ("a", "c", "k", "e")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


def direction_sets(part, c, d):
    """(label, v_ode, v_x0) of every launch the GPU tests make on case c of `part`."""
    if part in ("a", "e"):
        return [("unit",) + JC.unit_directions(c)]
    if part == "c":
        return [("unit",) + JC.unit_directions(c), (f"dense{JC.K_DENSE_C}",) + JC.dense_directions(c, d, JC.K_DENSE_C)]
    out = [(f"dense{K}",) + JC.dense_directions(c, d, K) for K in JC.K_TILING]
    vo, vx = JC.dense_directions(c, d, JC.K_POINTERS)
    return out + [("ode-only", vo, None), ("x0-only", None, vx)]


# ------------------------------------------------------------------ 1. duality
@pytest.mark.parametrize("part", PARTS)
def test_oracle_jvp_is_the_transpose_of_the_oracle_adjoint(O, part):
    worst = 0.0
    for c in JC.CASES[part]:
        d = IC.solve_data(c)
        sols = JC.oracle_tapes(O, c, "f64", d)
        per = c["B"] // c["n_sets"]
        back = [O.solve_bwd(sol, d["gy"][s * per:(s + 1) * per], want_gnn=False, want_gode=True) for s, sol in enumerate(sols)]
        for label, v_ode, v_x0 in direction_sets(part, c, d):
            dy = JC.oracle_jvp(O, c, sols, v_ode, v_x0)
            assert np.isfinite(dy).all()
            for s in range(c["n_sets"]):
                sl = slice(s * per, (s + 1) * per)
                gx0, _, gode = back[s]
                for k in range(dy.shape[1]):
                    terms = [d["gy"][sl] * dy[sl, k]]
                    rhs = []
                    if v_x0 is not None:
                        rhs.append(gx0 * v_x0[sl, k])
                    if v_ode is not None:
                        rhs.append(gode * v_ode[s, k])
                    scale = sum(float(np.abs(x).sum()) for x in terms + rhs)
                    err = abs(float(terms[0].sum()) - sum(float(x.sum()) for x in rhs))
                    if scale == 0:                          # both sides identically 0: IGD_50 and g without GD
                        assert label == "unit" and k in JC.GD_ONLY and not JC.has_gd(c), (c["name"], label, k)
                        continue
                    worst = max(worst, err / scale)
                    assert err <= 1e-12 * scale, (c["name"], label, s, k, err / scale)
    print(f"FIGURE duality part {part}: worst {worst:.3e}")


# ------------------------------------------------------------------ 2. finite differences
# On the cases of tests/test_jvp_gpu.py (its `case` recipe: the trained 64x4 weights, B = 4, T = 25 on 0..120), with and without GD.
# Not on the table's own cases: on their short horizon (t in [0, 3]) a constant like rho moves y by 1e-9 of |y| per relative step
# of 1e-5, so the rounding of the difference quotient (2e-16 |y| / step) alone is 3e-7 of the column -- above the 1e-7 bound whatever
# the tangent is.  Over 0..120 every constant has moved the trajectory by then.
def _fd_solve(O, c, ode=None, x0=None, tape=False, method=0, **kw):
    return O.solve(c["x0"] if x0 is None else x0, c["t"], *c["u"], c["ode"] if ode is None else ode, c["nn"], c["H"], c["L"],
                   method=method, dtype=np.float64, want_tape=tape, **kw)


@pytest.mark.parametrize("modes", [(2, 2, 2), (2, 2, 0)], ids=["gd1", "gd0"])
def test_oracle_rk4_jvp_matches_central_differences(O, g0, modes):
    """RK4 takes one step per interval whatever the parameters: the oracle's forward is a fixed smooth map and its central
    differences are the derivative to O(step^2).  Step and bound of test_rk4_jvp_matches_central_differences."""
    c = gpu_case(g0=g0, B=4, modes=modes)
    sol = _fd_solve(O, c, tape=True, method=JC.RK4)
    v_ode = np.zeros((JC.K_UNIT, 17))
    v_x0 = np.zeros((4, JC.K_UNIT, 6))
    v_ode[np.arange(17), np.arange(17)] = 1.0
    v_x0[:, 17 + np.arange(6), np.arange(6)] = 1.0
    dy = O.solve_jvp(sol, v_ode, v_x0)
    for j in range(JC.K_UNIT):
        if j < 17:
            h = 1e-5 * abs(c["ode"][j])
            e = np.zeros(17)
            e[j] = h
            yp, ym = _fd_solve(O, c, ode=c["ode"] + e, method=JC.RK4).y, _fd_solve(O, c, ode=c["ode"] - e, method=JC.RK4).y
        else:
            h = 1e-5 * max(abs(c["x0"][:, j - 17]).max(), 1.0)
            e = np.zeros(6)
            e[j - 17] = h
            yp, ym = _fd_solve(O, c, x0=c["x0"] + e, method=JC.RK4).y, _fd_solve(O, c, x0=c["x0"] - e, method=JC.RK4).y
        fd = (yp - ym) / (2 * h)
        if np.abs(fd).max() == 0:
            assert j in JC.GD_ONLY and modes[2] == 0 and np.abs(dy[:, j]).max() == 0, j
            continue
        rel = np.linalg.norm(dy[:, j] - fd) / np.linalg.norm(fd)
        assert rel < 1e-7, (JC.DIR_NAMES[j], rel)


def test_oracle_dp5_jvp_matches_differences_of_converged_solutions(O, g0):
    """As test_dp5_jvp_matches_differences_of_converged_solutions -- its case, columns, Richardson step and 1e-5 bound -- but with
    the solutions converged to rtol 1e-12 / atol 1e-14, not 1e-10 / 1e-12.  At 1e-10 the difference quotient of the oracle's forward
    is too noisy for the bound on ONE column: p_9 (the least sensitive constant) misses with 1.8e-5, every other column is <= 4.3e-6.
    That is the reference's error, not the tangent's: the miss grows to 6.0e-5 when the step shrinks from 2e-2 to 5e-3 (noise / step),
    and at 1e-12 the same column is 6.0e-7 (all columns <= 6.0e-7) -- while RK4 central differences (above) and duality with the
    adjoint (4e-16) pin the same tangent code.  The bound is unchanged and every column is kept."""
    c = gpu_case(g0=g0, B=4, modes=(2, 2, 2))
    kw = dict(rtol=1e-12, atol=1e-14, max_steps=20000)
    sol = _fd_solve(O, c, tape=True, **kw)
    assert int(sol.status.max()) == 0
    idx = [0, 1, 2, 5, 8, 9, 10, 11, 12, 13, 16]
    v_ode = np.zeros((len(idx), 17))
    for k, j in enumerate(idx):
        v_ode[k, j] = 1.0
    dy = O.solve_jvp(sol, v_ode, None)

    def central(j, h):
        e = np.zeros(17)
        e[j] = h
        return (_fd_solve(O, c, ode=c["ode"] + e, **kw).y - _fd_solve(O, c, ode=c["ode"] - e, **kw).y) / (2 * h)
    for k, j in enumerate(idx):
        # Richardson: (4 D(h/2) - D(h)) / 3 cancels the h^2 term, so a step large against the adaptive solver's noise fits
        h = 2e-2 * abs(c["ode"][j])
        fd = (4 * central(j, h / 2) - central(j, h)) / 3
        rel = np.linalg.norm(dy[:, k] - fd) / np.linalg.norm(fd)
        assert rel < 1e-5, (JC.DIR_NAMES[j], rel)


# ------------------------------------------------------------------ 3. rows
@pytest.mark.parametrize("name", ["t33x3-repeats", "t33x3-repeats-m212"])
def test_oracle_jvp_on_repeated_times_equals_the_grid_without_them(O, name):
    c = JC.find("c", name)
    d = IC.solve_data(c)
    t = d["t"]
    keep = [r for r in range(len(t)) if r == 0 or t[r] > t[r - 1]]
    group = np.searchsorted(t[keep], t)                     # row -> index of its time
    v_ode, v_x0 = JC.unit_directions(c)
    run = lambda tt, u: O.solve_jvp(O.solve(d["x0"], tt, *u, d["ode"], d["nn"], c["H"], c["L"], dtype=np.float64, want_tape=True,   # noqa: E731
                                            max_steps=c["max_steps"]), v_ode[0], v_x0)
    full = run(t, d["u"])
    short = run(t[keep], [v if v is None or v.ndim == 1 else v[:, keep] for v in d["u"]])
    assert relnorm(full, short[:, :, group]) <= 1e-15
    for r in range(1, len(t)):
        if not t[r] > t[r - 1]:
            assert np.array_equal(full[:, :, r], full[:, :, r - 1]), r
    assert np.array_equal(full[:, :, 0], v_x0) and np.array_equal(full[:, :, 1], v_x0)


def test_oracle_jvp_rows_after_a_failure_are_zero(O):
    c = JC.CASES["e"][0]
    d = IC.solve_data(c)
    sols = JC.oracle_tapes(O, c, "f64", d)
    st, ns = JC.status_nsteps(sols)
    assert (st == 1).all() and (ns == c["max_steps"]).all()
    v_ode, v_x0 = JC.unit_directions(c)
    dy = JC.oracle_jvp(O, c, sols, v_ode, v_x0)
    last = JC.last_written_row(sols[0], "f64", d["t"])
    assert (last >= 1).all() and (last <= c["T"] - 3).all()            # the budget ends well inside the grid
    for b in range(c["B"]):
        assert (dy[b, :, last[b] + 1:] == 0).all(), b
        assert (sols[0].y[b, last[b] + 1:] == 0).all() and (sols[0].y[b, last[b]] != 0).all(), b
        live = [k for k in range(JC.K_UNIT) if not (k in JC.GD_ONLY and not JC.has_gd(c))]
        assert (np.abs(dy[b, live, last[b]]).max(axis=-1) > 0).all(), b


# ------------------------------------------------------------------ 4. admission and coverage
def _admit(O, part, c):
    d = IC.solve_data(c)
    sets = direction_sets(part, c, d)
    ref = {}
    for dt in c["dtypes"]:
        sols = JC.oracle_tapes(O, c, dt, d)
        st, ns = JC.status_nsteps(sols)
        assert (st == c["expect_status"]).all(), (dt, st)
        for label, v_ode, v_x0 in sets:
            dy = JC.oracle_jvp(O, c, sols, v_ode, v_x0)
            assert np.isfinite(dy).all(), (dt, label)
            ref[dt, label] = dy
            if v_x0 is not None:
                assert np.array_equal(dy[:, :, 0], v_x0.astype(dy.dtype)), (dt, label)
            if label == "unit":
                for k in JC.GD_ONLY:
                    assert (np.abs(dy[:, k]).max() == 0) == (not JC.has_gd(c)), (dt, k)
                for k in range(JC.K_UNIT):
                    assert k in JC.GD_ONLY or np.abs(dy[:, k, 1:]).max() > 0, (dt, k)
        if dt == "f32":
            # the fp64 oracle at the fp32 cases' solver tolerances (they differ for DP5(4)): equal step counts, and the distance
            # of the fp32 oracle from it, per direction, leaves a margin of 8 room under the cap
            sols64 = JC.oracle_tapes(O, c, "f64", d, tols_of="f32")
            st64, ns64 = JC.status_nsteps(sols64)
            assert np.array_equal(st, st64) and np.array_equal(ns, ns64), (ns, ns64)
            for label, v_ode, v_x0 in sets:
                r64 = JC.oracle_jvp(O, c, sols64, v_ode, v_x0)
                for k in range(r64.shape[1]):
                    if np.abs(r64[:, k]).max() == 0:
                        assert np.abs(ref["f32", label][:, k]).max() == 0, (label, k)
                        continue
                    d_ref = JC.scaled_norm(ref["f32", label][:, k], r64[:, k])
                    assert d_ref <= IC.FP32_CAP[c["method"]] / 8, (label, k, d_ref)
    return max(int(JC.steps_per_interval(s, "f32").max()) for s in JC.oracle_tapes(O, c, "f32", d)) if "f32" in c["dtypes"] else 0


@pytest.mark.parametrize("part", PARTS)
def test_every_case_is_admissible(O, part):
    most = 0
    for c in JC.CASES[part]:
        try:
            most = max(most, _admit(O, part, c))
        except AssertionError as e:
            raise AssertionError(f"case {part}/{c['name']} (seed {c['seed']}): {e}") from e
    if part == "c":
        assert most >= 3, most                              # an fp32 case with an interval of three or more taped steps


def test_the_table_covers_every_instantiation_and_tile_residue():
    a = {(dt, c["L"], JC.has_gd(c), c["method"]) for c, dt in JC.params(JC.CASES["a"])}
    assert len(a) == 32 and all(c["H"] <= 64 and c["L"] <= 4 and c["act"] == IC.RELU for p in PARTS for c in JC.CASES[p])
    for L in (1, 2, 3, 4):
        for gd in (False, True):
            assert len({c["H"] for c in JC.CASES["a"] if c["L"] == L and JC.has_gd(c) == gd}) == 2, (L, gd)
    assert {c["H"] for c in JC.CASES["a"]} == {64, 33, 16, 7}
    tile = 8                                                # kJvpTile<float> of csrc/hode_solve_jvp.hip
    res = {("below" if K < tile else "one" if K == tile else "one+1" if K == tile + 1 else "two" if K == 2 * tile else
            "two+1" if K == 2 * tile + 1 else "other") for K in JC.K_TILING}
    assert res == {"below", "one", "one+1", "two", "two+1"}
    assert all("f32" in c["dtypes"] for c in JC.CASES["k"]) and max(JC.K_TILING) <= JC.DENSE_KMAX
    assert [c["name"] for c in JC.CASES["c"]] == [f"t33x3-{n}" for n in JC._C_NAMES] and len(JC.CASES["c"]) == 10
    assert {c["n_sets"] for c in JC.CASES["k"]} == {1, 3} and any(c["t_batched"] for c in JC.CASES["k"])
    assert JC.CASES["e"][0]["expect_status"] == 1 and JC.CASES["e"][0]["dtypes"] == ("f64",)
    assert all(m == 8.0 for m in JC.MARGIN.values()) and all(r < JC.MARGIN[p] for p, r in JC.MEASURED.items())


# ------------------------------------------------------------------ 5. the sanitizer self-check
def test_oracle_jvp_selfcheck_runs_clean_under_sanitizers():
    r = subprocess.run(["make", "-C", os.path.join(IC.ROOT, "oracle"), "-s", "selfcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "inputs_selfcheck: ok" in r.stdout and "jvp_selfcheck: ok" in r.stdout
