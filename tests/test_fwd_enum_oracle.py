"""CPU admission of every case of tests/_fwd_enum_cases.py (FE), from the oracle alone: what a case must satisfy before a forward
kernel is compared on it in tests/test_fwd_enum_gpu.py, and that the table reaches every instantiation by the restated launch rule.

Per case and dtype: status as the case expects; the fp32 and the fp64 oracle (at the same solver tolerances) equal in status, nsteps
and nfev -- the condition under which a kernel can be held to EQUALITY with the oracle at its own dtype; d_ref below D_REF_MAX; the
network, and with GD on the Hill term, move every trajectory by at least 100 of its bounds; the rejected-step cases reject, the budget
cases end where they claim, the NaN cases fail only the trajectory they name.

One exemption, by construction and not by tolerance: the nfev of a trajectory with a NaN in x0 under DP5(4).  Every step of it is
rejected and h shrinks by 0.2 until it is below 10 eps |t| (t = 0: 10 eps 1e-30), so the number of attempts is a function of the
format's eps: 51 in fp32, 64 in fp64 (308 = 2 + 6 x 51, 386 = 2 + 6 x 64 evaluations).  Its status and nsteps still agree, and the
kernel is held to the oracle AT ITS OWN dtype on it like on every other trajectory."""
import numpy as np
import pytest

import _fwd_enum_cases as FE
import _input_grad_cases as IC
from _fwd_enum_cases import DP5, RK4

PARTS = ("a", "b", "c", "d", "e")


def _admit(part, c, dt):
    d, rows, r64, rdt, rall = FE.refs(part, c["name"], dt)
    exp = FE.expected_status(c)
    assert np.array_equal(rall["status"], exp), ("status", np.flatnonzero(rall["status"] != exp)[:8], rall["status"][:8])
    assert np.array_equal(r64["status"], exp[rows])
    nan = np.zeros(c["B"], bool)
    nan[list(c["nan_rows"])] = True
    assert set(np.flatnonzero(exp == 3)) == set(c["nan_rows"])          # a NaN case fails only the trajectory it names
    if dt == "f32":
        assert np.array_equal(rdt["status"], r64["status"]) and np.array_equal(rdt["nsteps"], r64["nsteps"]), \
            ("fp32 / fp64 nsteps", rows[np.flatnonzero(rdt["nsteps"] != r64["nsteps"])][:8])
        same = (rdt["nfev"] == r64["nfev"]) | (nan[rows] if c["method"] == DP5 else False)
        assert same.all(), ("fp32 / fp64 nfev", rows[~same][:8], rdt["nfev"][~same][:8], r64["nfev"][~same][:8])
        if c["method"] == DP5 and c["nan_rows"]:
            assert (rdt["nfev"][nan[rows]] == 2 + 6 * 51).all() and (r64["nfev"][nan[rows]] == 2 + 6 * 64).all()
    assert (rall["nsteps"][nan] == 0).all()
    d_ref = FE.figures(rdt["y"], r64["y"]) if dt == "f32" else np.zeros((len(rows), 6))
    assert d_ref.max() <= FE.D_REF_MAX[part][c["method"]], ("d_ref", d_ref.max())
    tol = FE.tolerances(part, c["method"], dt, d_ref)
    tols = IC.solver_tols(c, dt)
    if c["moves"]:
        live = ~nan[rows]
        alts = [("network", dict(nn_scale=0.0))] + ([("Hill term", dict(no_gd=True))] if c["modes"][2] else [])
        for what, kw in alts:
            alt = FE.oracle_fwd(c, d, "f64", tols, rows, **kw)
            move = (FE.figures(alt["y"], r64["y"]) / tol).max(1)
            assert (move[live] >= 100).all(), (what, "moves y by only", move[live].min(), "bounds at", rows[live][np.argmin(move[live])])
    else:
        assert (rall["nsteps"] == 0).all() and (rall["nfev"] == 0).all()        # nothing is integrated: every row is x0
    if c["rejects"]:
        for r in (rall, r64):
            assert (r["status"] == 0).all() and (r["nfev"] > 6 * r["nsteps"] + 2).all(), ("no rejected step", r["nfev"], r["nsteps"])
    if c["ends"] is not None:
        tp = FE.oracle_fwd(c, d, dt, tols, want_tape=True)
        assert np.array_equal(tp["nsteps"], rall["nsteps"])
        assert (rall["status"] == 1).all() and (rall["nsteps"] == c["max_steps"]).all(), rall["nsteps"]
        assert (tp["closed"] == (c["ends"] == "closed")).all(), ("the budget does not end", c["ends"], tp["closed"])
        zero = (rall["y"] == 0).all(2)
        first = zero.argmax(1)
        assert zero.any(1).all() and all(zero[b, f:].all() and not zero[b, :f].any() for b, f in enumerate(first))
        if c["T"] == 33:
            assert (first == 20).all() and 64 < 6 * 20 and 6 * 20 + 5 < 128 and (6 * 20) % 64 != 0   # inside the second 64-real store
        if c["method"] == RK4:
            assert c["max_steps"] < c["T"] - 1
    if isinstance(c["expect"], str):                                     # part d, budget of 2: a live trajectory behind every failing one
        assert (exp[0::2] == 1).all() and (exp[1::2] == 0).all() and c["takes"] == ("multi", 2) and c["max_steps"] == 2
        assert (rall["y"][0::2, 2:] == 0).all() and (rall["y"][0::2, 1] != 0).all() and (rall["y"][1::2] != 0).all()
    if c["some_runs"] is not None:
        t = d["t"]
        runs = (t[:, 1:] == t[:, :-1]).any(1)
        assert runs[1::2].all() and not runs[0::2].any()
    for k, m in enumerate(c["modes"]):
        assert (d["u"][k] is None) == (m == 0) and (m == 0 or d["u"][k].ndim == m)


@pytest.mark.parametrize("part", PARTS)
def test_every_case_is_admissible(part):
    n = 0
    for c, dt in FE.params(part):
        try:
            _admit(part, c, dt)
        except AssertionError as e:
            raise AssertionError(f"case {part}/{c['name']}-{dt} (seed {c['seed']}): {e}") from e
        n += 1
    print(f"part {part}: {n} (case, dtype) admitted")


def test_the_table_reaches_all_68_instantiations_by_the_restated_rule():
    seen = {}
    for part in ("a", "b", "c", "d"):
        for c, dt in FE.params(part):
            assert FE.tuned(c)
            for tape in c["tapes"]:
                p = FE.case_path(c, dt, tape)
                assert (("multi", p[5]) if p[4] else ("single", 1)) == c["takes"], (part, c["name"], p)
                seen.setdefault(FE.instantiation(p, dt), []).append(f"{part}/{c['name']}")
    every = {(dt, nl, m, tape, gd, False) for dt in ("f32", "f64") for nl in (1, 2, 3, 4) for m in (DP5, RK4) for tape in (False, True)
             for gd in (False, True)} | {("f32", nl, DP5, False, False, True) for nl in (1, 2, 3, 4)}
    assert len(every) == 68 and set(seen) == every, (every - set(seen), set(seen) - every)
    # part a alone reaches the 64 one-trajectory kernels, part d the four MULTI ones; every H of the cycle occurs
    a = {FE.instantiation(FE.case_path(c, dt, tape), dt) for c, dt in FE.params("a") for tape in c["tapes"]}
    assert len(a) == 64 and {c["H"] for c in FE.CASES["a"]} == {64, 33, 16, 7}
    assert all(any(c["modes"][k] == v for c in FE.CASES["a"]) for k in range(3) for v in (0, 1, 2))      # every input in every mode
    print(f"forward enumeration: {len(seen)} of {len(every)} instantiations reached")
    # what FwdRot and launch_one make of them: every rotation form and every occupancy occurs, the benchmark kernel is the lean K = 8
    forms = {(p[6], p[7]) for c, dt in FE.params("a") for tape in c["tapes"] for p in [FE.case_path(c, dt, tape)]}
    assert forms == {(0, False), (8, True), (12, False)}
    assert FE.fwd_path("f32", 4, DP5, False, False, 4096, 2, 1)[4:8] == (False, 1, 8, True)
    assert FE.fwd_path("f32", 4, DP5, False, False, 81920, 2, 1)[4:8] == (True, 10, 0, False)
    assert FE.fwd_path("f32", 4, DP5, True, False, 5, 7, 1)[6] == 0 and FE.fwd_path("f32", 4, RK4, True, False, 5, 7, 1)[6] == 8
    assert FE.fwd_path("f32", 4, RK4, True, True, 5, 7, 1)[6] == 0 and FE.fwd_path("f32", 2, DP5, False, False, 5, 7, 1)[6] == 0
    assert {FE.case_path(c, dt, False)[9] for c, dt in FE.params("a")} == {1, 2, 3, 4}
    # both stage forms of fp32 DP5(4) meet rejected steps
    rej = {(dt, FE.case_path(c, dt, False)[8]) for c, dt in FE.params("b") if c["rejects"]}
    assert rej == {("f32", True), ("f32", False), ("f64", False)}
    # the neighbours of part d take one trajectory per wave, everything else of it MULTI with the chunk it names
    single = [c["name"] for c in FE.CASES["d"] if not FE.case_path(c, "f32", False)[4]]
    assert single == ["nl4-h64-B8192-T3-single", "nl4-h64-B8200-T5-single", "nl4-h64-B8200-T3-sets2-single"]
    chunks = {(FE.case_path(c, "f32", False)[0], c["B"], c["T"], FE.case_path(c, "f32", False)[5]) for c in FE.CASES["d"] if c["name"] not in single}
    assert {(nl, 8200, 3, 2) for nl in (1, 2, 3, 4)} | {(nl, 16390, T, 3) for nl in (1, 2, 3, 4) for T in (2, 4)} <= chunks
    assert (16390 + 2) // 3 == 5464 and 16390 - 5463 * 3 == 1           # the last wave of chunk 3 has one trajectory
    assert {(c["H"], c["L"]) for c in FE.CASES["d"] if c["name"] not in single} >= {(64, 1), (33, 2), (16, 3), (7, 4)}
    # part c: the second set of a 64x4 network starts 8 bytes off a 16-byte boundary in fp32
    assert IC.n_params(64, 4) == 13510 and (13510 * 4) % 16 == 8 and any(c["H"] == 64 and c["L"] == 4 and c["n_sets"] == 3 for c in FE.CASES["c"])


def test_part_e_takes_the_team_kernels_it_names():
    want = {("f32", 5): ("resident", 8, 1), ("f32", 258): ("multi", 8, 2), ("f32", 516): ("multi", 8, 4), ("f32", 1032): ("multi", 8, 8),
            ("f64", 5): ("stream", 8, 1), ("f64", 260): ("stream", 4, 1)}
    seen = set()
    for c, dt in FE.params("e"):
        assert not FE.tuned(c) and c["modes"][2] != 0 and c["T"] == 4 and c["tapes"] == (False, True)
        kind, nw, tb, cc, nb = FE.generic_path(dt, c["H"], c["L"], c["B"], c["n_sets"])
        assert (kind, nw, tb) == want[(dt, c["B"])] and cc == (8 if c["H"] <= 64 else 16)
        assert c["takes"] == (kind, tb if kind != "stream" else nw)
        seen.add((dt, c["B"], c["H"], c["method"]))
    assert len(seen) == 2 * 2 * 6
    # the neighbours of the rule's thresholds, as launch_fwd_generic_m has them
    assert FE.generic_path("f32", 100, 3, 512, 1)[:3] == ("multi", 8, 2) and FE.generic_path("f32", 100, 3, 257, 1)[:3] == ("resident", 8, 1)
    assert FE.generic_path("f32", 40, 3, 257, 1)[:3] == ("stream", 4, 1) and FE.generic_path("f32", 100, 6, 258, 1)[:3] == ("stream", 4, 1)
    assert FE.generic_path("f32", 100, 3, 1028, 1)[:3] == ("multi", 8, 4) and FE.generic_path("f32", 100, 3, 1026, 1)[:3] == ("multi", 8, 2)


def test_the_samples_hold_what_they_must():
    for c in FE.CASES["d"]:
        rows = set(FE.sample_rows(c).tolist())
        B = c["B"]
        assert 512 <= len(rows) < B // 8
        chunk = FE.case_path(c, "f32", False)[5]
        n_wg = (B + chunk - 1) // chunk
        assert set(range(chunk)) <= rows and set(range((n_wg - 1) * chunk, B)) <= rows
        failing = np.flatnonzero(FE.expected_status(c))
        if 0 < len(failing) <= 64:
            for b in failing:
                assert {x for x in (b - 1, b, b + 1) if 0 <= x < B} <= rows
        elif len(failing):
            assert sum({b - 1, b, b + 1} <= rows for b in failing) >= 32
    for c in FE.CASES["e"]:                                               # part e: every row
        assert len(FE.sample_rows(c)) == c["B"]


def test_margins_follow_the_rule():
    for p, r in FE.MEASURED.items():
        assert FE.MARGIN[p] == (8.0 if (r is None or r <= 4) else 2.0 * r)
        for m in (DP5, RK4):
            assert FE.MARGIN[p] * FE.D_REF_MAX[p][m] <= FE.FP32_CAP[m] * (1 + 1e-12)
    assert FE.FP32_CAP == {RK4: 1e-5, DP5: 1e-4, "rhs": 1e-5} and FE.FP64_TOL == {RK4: 1e-12, DP5: 1e-9} and FE.FLOOR == 2.0 ** -24
