"""CPU tests of the oracle's input gradients (oracle/hode_oracle_impl.h: hode_oracle_solve_bwd_inputs_*, hode_oracle_rhs_vjp_inputs_*)
and the admission of every case of tests/_input_grad_cases.py, from the oracle alone.

1. against fixture G10 (torch fp64 autograd through the reference's modules): the RHS gradients of all three nets and the RK4 solve
   with inputs on the grid and constant, at 64x4 and 128x5 -- relative norm <= 1e-12;
2. DP5(4) against the oracle's own central differences at rtol 1e-10;
3. admission: what a case must satisfy before a kernel is compared on it (status, non-zero gradients, fp32 oracle within 1e-6 of the
   fp64 one with equal step counts, off every ReLU kink, several steps per interval where the case is about that);
4. the sanitizer self-check program of oracle/Makefile."""
import os
import subprocess

import numpy as np
import pytest

import _input_grad_cases as IC
from _input_grad_cases import KEYS, relnorm

ROOT = IC.ROOT
NETS = {"h64l4": (64, 4, 0), "h128l5": (128, 5, 0), "h96l6tanh": (96, 6, 1)}


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_input_grads.npz"))


# ------------------------------------------------------------------ 1. G10
@pytest.mark.parametrize("tag", list(NETS))
def test_oracle_rhs_input_grads_match_reference_autograd(O, G, tag):
    H, L, act = NETS[tag]
    a = lambda k: G[f"a_{tag}_{k}"]                        # noqa: E731
    nn = G[f"{tag}_nn_flat"].astype(np.float64)
    gx, gnn, gode, gin = O.rhs_vjp_inputs(a("x"), a("t"), a("meal"), a("tVNS"), a("GD"), G[f"{tag}_ode"], nn, H, O.layers(L, act),
                                          a("w"), dtype=np.float64)
    for k in KEYS:
        assert relnorm(gin[k], a(f"g_{k}")) <= 1e-12, k
    # the old entry point = the new one with no input outputs
    gx2, gnn2, gode2 = O.rhs_vjp(a("x"), a("t"), a("meal"), a("tVNS"), a("GD"), G[f"{tag}_ode"], nn, H, O.layers(L, act), a("w"),
                                 dtype=np.float64)
    assert np.array_equal(gx, gx2) and np.array_equal(gnn, gnn2) and np.array_equal(gode, gode2)


@pytest.mark.parametrize("tag", ["h64l4", "h128l5"])
@pytest.mark.parametrize("mode", ["series", "const"])
def test_oracle_rk4_solve_input_grads_match_reference(O, G, tag, mode):
    H, L, act = NETS[tag]
    b = lambda k: G[f"b_{tag}_{k}"]                        # noqa: E731
    u = [b(f"{mode}_{k}") for k in KEYS]
    sol = O.solve(b("x0"), b("t"), *u, G[f"{tag}_ode"], G[f"{tag}_nn_flat"].astype(np.float64), H, O.layers(L, act),
                  method=O.METHOD_RK4, dtype=np.float64, want_tape=True)
    assert int(sol.status.max()) == 0
    assert relnorm(sol.y, b(f"{mode}_y")) <= 1e-12
    gx0, gnn, gode, gin = O.solve_bwd_inputs(sol, b("gy"))
    for k, v in zip(KEYS, u):
        assert gin[k].shape == v.shape
        assert relnorm(gin[k], b(f"{mode}_g_{k}")) <= 1e-12, k
    ref = O.solve_bwd(sol, b("gy"))
    assert all(np.array_equal(x, y) for x, y in zip((gx0, gnn, gode), ref))


# ------------------------------------------------------------------ 2. DP5(4): the oracle against its own central differences
def test_oracle_dp5_input_grads_match_central_differences(O, G):
    tag = "h64l4"
    H, L, act = NETS[tag]
    g = np.random.default_rng(0)                           # (_dp5_case of tests/test_input_grads_gpu.py)
    B, T = 4, 13
    x0 = np.array([5., 60., 80., 10., 0.5, 1.]) * (1 + 0.1 * g.standard_normal((B, 6)))
    t = np.linspace(0, 3, T)
    u = {"meal": 3 * g.random((B, T)), "tVNS": g.random((B, T)), "GD": 200 + 600 * g.random((B, T))}
    gy = g.standard_normal((B, T, 6))
    nn, ode = G[f"{tag}_nn_flat"].astype(np.float64), G[f"{tag}_ode"]

    def run(w, tape=False):
        return O.solve(x0, t, w["meal"], w["tVNS"], w["GD"], ode, nn, H, L, rtol=1e-10, atol=1e-12, dtype=np.float64, want_tape=tape,
                       max_steps=4000)
    sol = run(u, True)
    assert int(sol.status.max()) == 0
    gin = O.solve_bwd_inputs(sol, gy, want_gnn=False, want_gode=False)[3]
    rng = np.random.default_rng(1)
    for k, rel_eps in (("meal", 1e-5), ("tVNS", 1e-3), ("GD", 1e-5)):
        v = rng.standard_normal(u[k].shape)
        eps = rel_eps * float(np.abs(u[k]).max())

        def J(s):
            w = dict(u)
            w[k] = u[k] + s * eps * v
            return float((run(w).y * gy).sum())
        fd = (J(1) - J(-1)) / (2 * eps)
        ad = float((gin[k] * v).sum())
        assert abs(ad - fd) <= 1e-5 * abs(fd) + 1e-9, (k, ad, fd)


def test_oracle_on_repeated_times_equals_the_grid_without_them(O):
    """Rows of one repeated time carry one input value (tests/_input_grad_cases.py): the solve over the grid with repeats is then the
    solve over the distinct times -- gy and the series gradients of a run of equal times add up, the middle rows stay exactly 0."""
    c = next(c for c in IC.SOLVE["c"] if c["name"] == "t33x3-repeats")
    d = IC.solve_data(c)
    t = d["t"]
    keep = [r for r in range(len(t)) if r == 0 or t[r] > t[r - 1]]
    group = np.searchsorted(t[keep], t)                     # row -> index of its time
    fold = lambda a: np.stack([a[:, group == j].sum(1) for j in range(len(keep))], 1)   # noqa: E731
    run = lambda tt, u, gy: O.solve_bwd_inputs(O.solve(d["x0"], tt, *u, d["ode"], d["nn"], c["H"], c["L"], dtype=np.float64, want_tape=True,   # noqa: E731
                                                       max_steps=c["max_steps"]), gy)
    gx0, gnn, gode, gin = run(t, d["u"], d["gy"])
    hx0, hnn, hode, hin = run(t[keep], [v[:, keep] for v in d["u"]], fold(d["gy"]))
    for a, b in ((gx0, hx0), (gnn, hnn), (gode, hode)) + tuple((fold(gin[k]), hin[k]) for k in KEYS):
        assert relnorm(a, b) <= 1e-13
    for k in KEYS:
        assert (gin[k][:, list(c["zero_rows"])] == 0).all()


# ------------------------------------------------------------------ 3. admission
def _admit_solve(O, c, part):
    d = IC.solve_data(c)
    r64 = IC.oracle_solve(O, c, "f64", d)
    assert (r64["status"] == c["expect_status"]).all(), r64["status"]
    wanted = [k for k in IC.ALL_KEYS if r64["g"][k] is not None]
    assert set(wanted) == {k for k, m in zip(KEYS, c["modes"]) if m} | {"gx0"} | ({"gnn"} if c["want_gnn"] else set()) | \
        ({"gode"} if c["want_gode"] else set())
    for k in wanted:
        assert np.isfinite(r64["g"][k]).all() and np.linalg.norm(r64["g"][k]) > 0, k
    # rows that bound no taped step are exactly 0 (a touched row may be 0 too: tVNS under a dead first layer)
    for k, m in zip(KEYS, c["modes"]):
        if m == 2:
            assert (r64["g"][k][~r64["touched"]] == 0).all(), k
            # (a failed trajectory whose last step did not close its interval carries no cotangent over that interval)
            assert k == "tVNS" or c["gd_zero_rows"] or c["expect_status"] or (r64["g"][k][r64["touched"]] != 0).all(), k
    if c["zero_rows"] is not None:
        untouched = sorted(set(np.flatnonzero(~r64["touched"].all(0)).tolist()))
        assert untouched == list(c["zero_rows"]) and (~r64["touched"][:, untouched]).all()
    if c["gd_zero_rows"] == (0, 1):
        # interval 0 lies between two GD rows of 0: it adds exactly 0 to rows 0 and 1; interval 1 adds to row 1
        assert (r64["g"]["GD"][:, 0] == 0).all() and (r64["g"]["GD"][:, 1] != 0).all() and (r64["g"]["meal"][:, 0] != 0).all()
    if part == "e":
        assert (~r64["touched"][:, -2:]).all() and r64["touched"][:, :2].all()       # the budget ends well inside the grid
    if c["name"].endswith("T4-steps"):
        assert (r64["nsteps"] >= c["T"] + 2).all(), r64["nsteps"]
    # smoothness: no ReLU kink within 1e-6 of the inputs
    r64p = IC.oracle_solve(O, c, "f64", d, scale_inputs=1 + 1e-6)
    assert np.array_equal(r64p["nsteps"], r64["nsteps"])
    for k in wanted:
        assert relnorm(r64p["g"][k], r64["g"][k]) < 1e-5, k
    if "f32" in c["dtypes"]:
        # the fp64 oracle with the fp32 cases' solver tolerances (they differ for DP5(4))
        c64 = dict(c, **IC.solver_tols(c, "f32"))
        r64 = IC.oracle_solve(O, c64, "f64", d)
        r32 = IC.oracle_solve(O, c, "f32", d)
        assert np.array_equal(r32["status"], r64["status"]) and np.array_equal(r32["nsteps"], r64["nsteps"]), (r32["nsteps"], r64["nsteps"])
        for k in wanted:
            assert relnorm(r32["g"][k], r64["g"][k]) <= 1e-6, (k, relnorm(r32["g"][k], r64["g"][k]))


@pytest.mark.parametrize("part", ["a", "b", "c", "d", "e"])
def test_every_solve_case_is_admissible(O, part):
    for c in IC.SOLVE[part]:
        try:
            _admit_solve(O, c, part)
        except AssertionError as e:
            raise AssertionError(f"case {part}/{c['name']} (seed {c['seed']}): {e}") from e


def _admit_rhs(O, c):
    if True:
        for B in IC.RHS_B:
            for present in IC.RHS_SUBSETS:
                d = IC.rhs_data(c, B, present)
                r64, r32 = IC.oracle_rhs(O, c, B, present, "f64", d), IC.oracle_rhs(O, c, B, present, "f32", d)
                where = (c["name"], B, present)
                for k in IC.ALL_KEYS:
                    if k in KEYS and k not in present:
                        assert r64[k] is None, where
                    elif r64[k] is not None:
                        assert np.linalg.norm(r64[k]) > 0, (where, k)
                        assert relnorm(r32[k], r64[k]) <= 1e-6, (where, k, relnorm(r32[k], r64[k]))
                if "GD" in present:
                    zero, neg = IC.rhs_gd_special(B)
                    special = np.concatenate([zero, neg])
                    assert B < 5 or len(special) == 4
                    for r in (r64, r32):
                        assert (r["GD"][special] == 0).all() and (np.delete(r["GD"], special) != 0).all(), where


def test_every_rhs_case_is_admissible(O):
    for c in IC.RHS:
        _admit_rhs(O, c)


def test_the_table_covers_every_instantiation():
    a = {(c["L"], c["want_gode"], c["modes"][2] != 0, dt) for c, dt in IC.params(IC.SOLVE["a"])}
    assert len(a) == 32 and all(c["H"] <= 64 and c["act"] == 0 for c in IC.SOLVE["a"])
    assert {c["H"] for c in IC.SOLVE["a"]} == {64, 33, 16, 7}
    fam = {}
    for c, dt in IC.params(IC.SOLVE["b"]):
        acc = dt == "f32" and c["want_gnn"] and c["L"] - 1 <= 4
        key = (dt, (8, 16 if c["H"] > 64 else 8) if acc else (16 if c["H"] > 64 else 8, 0))
        fam.setdefault(key, set()).add((c["want_gode"], c["modes"][2] != 0))
    assert len(fam) == 6                                   # fp32: four families, fp64: two
    for key, seen in fam.items():
        assert {g for g, _ in seen} == {True, False} and {g for _, g in seen} == {True, False}, key
    rhs = {(c["L"], c["want_gode"]) for c in IC.RHS if c["H"] <= 64 and c["L"] <= 4 and c["act"] == 0}
    assert len(rhs) == 8                                   # x 2 dtypes = the 16 tuned RHS instantiations
    assert IC.waves_with_two_tapes(256) == 8 and IC.waves_with_two_tapes(64) == 8 and IC.waves_with_two_tapes(304) == 8


# ------------------------------------------------------------------ 4. the sanitizer self-check
def test_oracle_inputs_selfcheck_runs_clean_under_sanitizers():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "selfcheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "inputs_selfcheck: ok" in r.stdout
