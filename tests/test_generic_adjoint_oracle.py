"""CPU tests of the case table tests/_generic_adjoint_cases.py (the generic-network training adjoint against the fp64 oracle, team by
team), from the oracle alone:

1. admission: what a case must satisfy before a kernel is compared on it -- the statuses it names, the same steps in fp32 and fp64,
   every figure with a non-zero reference (a row block of dead ReLU rows: exactly 0 in both oracles) and an fp32 oracle within
   D_REF_MAX of the fp64 one, off every kink, and the row bookkeeping the case claims (rows closed by one step, the last taped step of a
   failed trajectory, mixed tape lengths inside a team, the NaN trajectories' places) read from the oracle's tape;
2. every case takes the path it names by the restated launch rule, and the table reaches all 24 instantiations of
   solve_bwd_generic_multi_kernel<GODE, GD, TB, RPW> and every (R, GODE, GD, NW, ACCREG) of the GIN = false one-trajectory kernel
   that the rule can reach;
3. the comparison rejects planted errors, the one in a single wave's rows among them, that the whole-vector criterion lets through."""
import functools

import numpy as np
import pytest

import _generic_adjoint_cases as GC
from _generic_adjoint_cases import relnorm


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def _refs(part, name):
    return GC.references(_oracle(), GC.find(part, name))


# ------------------------------------------------------------------ 1. admission
def _teams(c):
    """[(first, end)] trajectory ranges that share a team (multi path), set by set."""
    TB, per = c["takes"][1], c["B"] // c["n_sets"]
    return [(s * per + g, min(s * per + g + TB, (s + 1) * per)) for s in range(c["n_sets"]) for g in range(0, per, TB)]


def _admit(c, ref):
    O = _oracle()
    d, r64, r32, s_e = ref["d"], ref["r64"], ref["r32"], ref["s_e"]
    B, T = c["B"], c["T"]
    assert np.array_equal(r64["status"], GC.expected_status(c)), r64["status"]
    assert np.array_equal(r32["status"], r64["status"]) and np.array_equal(r32["nsteps"], r64["nsteps"]), (r32["nsteps"], r64["nsteps"])
    assert np.array_equal(r32["seg"], r64["seg"])
    assert (r64["gnn"] is not None) == c["want_gnn"] and (r64["gode"] is not None) == c["want_gode"]
    ok = r64["status"] != 3
    assert (r64["nsteps"][ok] > 0).all() and (r64["nsteps"][~ok] == 0).all() and (r64["nsteps"] <= c["max_steps"]).all()
    # every figure: a non-zero reference (or a listed structural zero, or a block of dead rows), the fp32 oracle within D_REF_MAX
    f32 = GC.figures(c, r32, r64, s_e)
    for key, (err, size) in f32.items():
        if key in GC.WC.structural_zeros(c):
            assert (size == 0).all(), key
            continue
        live = size > 0
        if GC.is_row_block(key) and c["act"] == GC.RELU:
            assert live.any(), key                              # (a block whose rows are all dead: the exact-zero check holds it)
        else:
            assert live.all(), (key, np.flatnonzero(~live)[:4])
        assert np.isfinite(size[live]).all() and err[live].max() <= GC.D_REF_MAX, (key, int(np.argmax(np.where(live, err, 0))), float(err[live].max()))
    # smoothness: no kink within 1e-6 of the inputs
    p64 = GC.oracle_run(O, c, "f64", d, scale_inputs=1 + 1e-6)
    assert np.array_equal(p64["nsteps"], r64["nsteps"])
    for key, (err, size) in GC.figures(c, p64, r64, s_e).items():
        assert err[size > 0].max(initial=0.0) < 1e-5, (key, float(err[size > 0].max()))
    # the row bookkeeping the case is about, from the tape's interval words
    tb = d["t"] if c["t_batched"] else np.tile(d["t"], (B, 1))
    assert c["grid"] == GC.REPEATS_GRID or (np.diff(tb, axis=1) <= 0.5 + 1e-12).all()
    if c["run_closes"] is not None:
        runs = set(range(0, B, 3))
        for b in range(B):
            cl = GC.closes(r64["seg"][b], r64["nsteps"][b], T)
            assert max(cl) == (c["run_closes"] if b in runs else 1), (b, cl)
        mixed = [any(b in runs for b in range(*t)) and any(b not in runs for b in range(*t)) for t in _teams(c)]
        assert sum(mixed) >= len(mixed) // 2                      # team-mates whose tapes differ
    if c["grid"] == GC.REPEATS_GRID:
        for b in range(B):                                      # a step closes the three rows at 1.2, the last one both rows at 3.0
            cl = GC.closes(r64["seg"][b], r64["nsteps"][b], T)
            assert max(cl) == 3 and cl[-1] == 2, (b, cl)
        assert ((r64["seg"][:, 0] & (GC.SEG_CLOSED - 1)) == 1).all()
    if c["kf"] is not None:
        assert ((r64["seg"][:, 0] & (GC.SEG_CLOSED - 1)) == c["kf"]).all() and not (tb[:, c["kf"]] > tb[:, 0]).any()
    if c["last_open"] is not None:
        assert (r64["nsteps"] == c["max_steps"]).all()
        last = r64["seg"][np.arange(B), r64["nsteps"] - 1]
        k = last & (GC.SEG_CLOSED - 1)
        assert (((last & GC.SEG_CLOSED) == 0) == c["last_open"]).all(), last
        assert (k >= 1).all()                                   # an earlier step closed a row: the gradient is not just gy[:, 0]
        if not c["last_open"]:
            assert (~(tb[np.arange(B), k + 2] > tb[np.arange(B), k + 1])).all() and (k + 3 < T).all()
    if c["mixed"]:
        # tapes of different lengths inside one team: some waves serve while others still walk
        differ = sum(len(set(r64["nsteps"][a:b].tolist())) > 1 for a, b in _teams(c))
        assert differ >= len(_teams(c)) // 4 and len(set(r64["nsteps"].tolist())) >= 3, (differ, set(r64["nsteps"].tolist()))
    if c["nan_rows"]:
        TB = c["takes"][1]
        first, last = c["nan_rows"]
        assert first % TB == 0 and last % TB == TB - 1 and first // TB != last // TB and last < B - TB
        assert (r64["status"] == 3).sum() == 2
    if c["gd_zero_rows"]:
        assert (d["u"][2][:, list(c["gd_zero_rows"])] == 0).all()


@pytest.mark.parametrize("part", list(GC.CASES))
def test_every_case_is_admissible(part):
    for c in GC.CASES[part]:
        try:
            _admit(c, _refs(part, c["name"]))
        except AssertionError as e:
            raise AssertionError(f"case {part}/{c['name']} (seed {c['seed']}): {e}") from e


def test_every_rhs_case_is_admissible():
    O = _oracle()
    for c in GC.RHS:
        for B in GC.RHS_B:
            for present in GC.RHS_SUBSETS:
                d, r64, r32 = GC.rhs_refs(O, c, B, present)
                for k in GC.RHS_KEYS:
                    assert (r64[k] is not None) == (k != "gode" or c["want_gode"])
                    if r64[k] is not None:
                        assert np.linalg.norm(r64[k]) > 0 and relnorm(r32[k], r64[k]) <= GC.RHS_D_REF_MAX, (c["name"], c["seed"], B, present, k,
                                                                                                           relnorm(r32[k], r64[k]))
                # smoothness: no kink within 1e-6 of the states and inputs
                p = dict(d, x=d["x"] * (1 + 1e-6), u=tuple(None if v is None else v * (1 + 1e-6) for v in d["u"]))
                p64 = GC.IC.oracle_rhs(O, c, B, present, "f64", p)
                for k in GC.RHS_KEYS:
                    assert r64[k] is None or relnorm(p64[k], r64[k]) < 1e-5, (c["name"], c["seed"], B, present, k, relnorm(p64[k], r64[k]))
        # gt: the central difference is a derivative (two step sizes agree far inside the bound the GPU test uses)
        d = GC.rhs_case_data(c, 5, GC.RHS_SUBSETS[0])
        fd = GC.rhs_gt_reference(O, c, d)
        e, L = 10 * GC.RHS_GT_EPS, GC.layers(c["L"], c["act"])
        wide = ((O.rhs(d["x"], d["t"] + e, *d["u"], d["ode"], d["nn"], c["H"], L, np.float64) -
                 O.rhs(d["x"], d["t"] - e, *d["u"], d["ode"], d["nn"], c["H"], L, np.float64)) * d["w"]).sum(1) / (2 * e)
        assert np.abs(fd).max() > 0 and np.max(np.abs(fd - wide)) < 1e-6 * max(1.0, np.abs(fd).max()), c["name"]


# ------------------------------------------------------------------ 2. the paths and the coverage
def test_the_launch_rule():
    P = GC.generic_adjoint_path
    assert P("f32", 128, 5, GC.RELU, 4096, 1, True) == ("multi", 8, 16, 512) and P("f32", 128, 5, GC.RELU, 1025, 1, True) == ("multi", 8, 16, 129)
    assert P("f32", 128, 5, GC.RELU, 1024, 1, True) == ("multi", 4, 16, 256) and P("f32", 40, 3, GC.TANH, 513, 1, True) == ("multi", 4, 8, 129)
    assert P("f32", 40, 3, GC.TANH, 512, 1, True) == ("multi", 2, 8, 256) and P("f32", 40, 3, GC.TANH, 257, 1, True) == ("multi", 2, 8, 129)
    assert P("f32", 40, 3, GC.TANH, 256, 1, True) == ("team", 8, 8, True, 256) and P("f32", 65, 2, GC.RELU, 5, 1, True) == ("team", 8, 16, True, 5)
    assert P("f32", 40, 3, GC.TANH, 261, 3, True) == ("multi", 2, 8, 44) and P("f32", 40, 3, GC.TANH, 1040, 130, True) == ("multi", 8, 8, 1)
    assert P("f32", 24, 3, GC.LEAKY, 4104, 1, True) == ("multi", 8, 8, 512) and -(-4104 // 8) == 513
    assert P("f32", 24, 3, GC.LEAKY, 1030, 1030, True) == ("team", 8, 8, False, 1024) and P("f32", 24, 3, GC.LEAKY, 2048, 1024, True)[0] == "multi"
    assert P("f32", 100, 1, GC.RELU, 259, 1, True) == ("team", 8, 16, True, 259) and P("f32", 40, 6, GC.TANH, 259, 1, True) == ("team", 8, 0, False, 259)
    assert P("f32", 128, 8, GC.RELU, 5000, 1, True) == ("team", 16, 0, False, 4096) and P("f32", 100, 3, GC.RELU, 259, 1, False) == ("team", 16, 0, False, 259)
    assert P("f64", 64, 5, GC.RELU, 259, 1, True) == ("team", 8, 0, False, 259) and P("f64", 128, 2, GC.ELU, 5, 1, True) == ("team", 16, 0, False, 5)
    assert P("f32", 64, 5, GC.RELU, 300, 3, True) == ("multi", 2, 8, 50) and P("f32", 64, 5, GC.RELU, 120, 3, True) == ("team", 8, 8, True, 120)


def test_every_case_takes_the_path_it_names_and_the_table_covers_every_instantiation():
    multi, team = {}, {}
    for part, cases in GC.CASES.items():
        for c in cases:
            assert not GC.tuned_shape(c["H"], c["L"], c["act"]), c["name"]
            path = GC.generic_adjoint_path(c["dt"], c["H"], c["L"], c["act"], c["B"], c["n_sets"], c["want_gnn"])
            assert path == c["takes"], (c["name"], path)
            assert (path[0] == "multi") == (part in "abc"), (c["name"], path)
            gd = c["modes"][2] != 0
            if path[0] == "multi":
                multi.setdefault((c["want_gode"], gd, path[1], path[2]), []).append(c)
            else:
                team.setdefault((c["dt"], c["want_gode"], gd, path[1], path[2]), []).append(c)
    flags = [(a, b) for a in (False, True) for b in (False, True)]
    assert set(multi) == {(gode, gd, TB, RPW) for gode, gd in flags for TB in (2, 4, 8) for RPW in (8, 16)} and len(multi) == 24
    # what the rule can reach of solve_bwd_generic_kernel<R, GODE, GD, NW, ACCREG, false>: fp32 <8, 8>, <8, 16>, <8, 0>, <16, 0>; fp64 the two last
    want = {(dt, gode, gd, nw, acc) for gode, gd in flags
            for dt, nw, acc in (("f32", 8, 8), ("f32", 8, 16), ("f32", 8, 0), ("f32", 16, 0), ("f64", 8, 0), ("f64", 16, 0))}
    assert set(team) == want and len(want) == 24
    # part a: every (TB, RPW) sees one, two, three and four hidden matrices; the ragged last teams; the row blocks the shapes are about
    a = GC.CASES["a"]
    assert len(a) == 24
    for TB, left in ((2, 1), (4, 3), (8, 5)):
        for RPW in (8, 16):
            mine = [c for c in a if c["takes"][1:3] == (TB, RPW)]
            assert sorted(c["L"] - 1 for c in mine) == [1, 2, 3, 4] and {(c["want_gode"], c["modes"][2] != 0) for c in mine} == set(flags)
            assert all(c["B"] % TB == left and c["takes"][3] == -(-c["B"] // TB) for c in mine)
            assert {c["method"] for c in mine} == {GC.RK4, GC.DP5}
    assert {(c["H"], c["L"], c["act"]) for c in a if c["takes"][2] == 8} == set(GC.MULTI_SHAPES[8])
    assert {(c["H"], c["L"], c["act"]) for c in a if c["takes"][2] == 16} == set(GC.MULTI_SHAPES[16])
    assert {c["act"] for c in a} == {GC.RELU, GC.TANH, GC.ELU, GC.LEAKY}
    assert GC.row_blocks(dict(takes=("multi", 2, 8, 1), H=24)) == [(0, 8), (8, 16), (16, 24)]
    assert GC.row_blocks(dict(takes=("multi", 2, 16, 1), H=100))[-1] == (96, 100) and GC.row_blocks(dict(takes=("multi", 2, 16, 1), H=65))[-1] == (64, 65)
    assert GC.row_blocks(dict(takes=("team", 8, 16, True, 1), H=100)) == [(0, 16), (16, 32), (32, 48), (48, 64), (64, 80), (80, 96), (96, 100)]
    assert GC.row_blocks(dict(takes=("team", 16, 0, False, 1), H=128))[1] == (8, 16)
    # part b: both team sizes on both networks; part c: ragged sets, one group per set, a workgroup's second group
    b = GC.CASES["b"]
    assert {(c["H"], c["takes"][1]) for c in b} == {(100, 2), (100, 4), (40, 2), (40, 4)} and all(c["want_gode"] for c in b)
    cs = {c["name"]: c for c in GC.CASES["c"]}
    assert {c["takes"][1:] for c in cs.values() if c["n_sets"] == 3} == {(2, 8, 44), (2, 16, 44)} and 87 % 2 == 1
    assert {c["takes"][1:] for c in cs.values() if c["n_sets"] == 130} == {(8, 8, 1), (8, 16, 1)} and 1024 // 130 == 7
    big = cs["single-B4104-24x3leaky-rk4"]
    assert big["takes"] == ("multi", 8, 8, 512) and -(-big["B"] // 8) == 513 and big["T"] == 3 and big["method"] == GC.RK4
    # part d: the neighbours the issue names
    d = GC.CASES["d"]
    assert {(c["B"], c["takes"][2]) for c in d if c["name"].startswith("rows")} == {(256, 8), (5, 8), (256, 16), (5, 16)}
    assert {c["takes"] for c in d if c["name"].startswith("gnn0") and c["B"] == 259} == {("team", 8, 0, False, 259), ("team", 16, 0, False, 259)}
    assert all(c["want_gode"] and not c["want_gnn"] for c in d if c["name"].startswith("gnn0") and c["B"] == 259)
    assert {(c["H"], c["L"], c["B"]) for c in d if c["name"].startswith("deep") and c["want_gode"]} == {(40, 6, 259), (128, 8, 5)}
    assert [c["takes"] for c in d if c["name"].startswith("nohidden")] == [("team", 8, 16, True, 259)]
    assert [c["takes"] for c in d if c["name"].startswith("sets1030x1")] == [("team", 8, 8, False, 1024)]
    assert {(c["H"], c["L"], c["B"]) for c in d if c["dt"] == "f64"} == {(64, 5, 5), (64, 5, 259), (128, 2, 5), (128, 2, 259)}
    assert all(c["dt"] == "f32" for p in "abc" for c in GC.CASES[p])
    # part e
    assert {(c["H"], c["L"], c["act"]) for c in GC.RHS} == set(GC.GENERIC_SHAPES) and len(GC.RHS) == 12
    assert -(-GC.RHS_B[-1] // 4) == 1025
    # the margins: 8, or twice the largest measured ratio where that exceeds 4
    for part, m in GC.MARGIN.items():
        r = GC.MEASURED[part]
        assert m == (8.0 if (r is None or r[1] <= 4) else round(2 * r[1], 1)), part


# ------------------------------------------------------------------ 3. planted errors
def _as_result(r):
    return {k: (None if r[k] is None else r[k].copy()) for k in ("status", "nsteps", "gx0", "gnn", "gode")}


def test_the_comparison_rejects_planted_errors():
    """The comparison of the GPU file, run on the fp32 ORACLE's result with one error planted at a time.  The first four pass the
    criterion of test_generic_adjoint_is_bit_reproducible_and_matches_the_oracle (whole-vector relnorm < 5e-3)."""
    c = next(c for c in GC.CASES["a"] if c["takes"][2] == 16 and c["want_gode"] and c["L"] >= 3 and c["act"] == GC.TANH)
    ref = _refs("a", c["name"])
    r64, r32, s_e = ref["r64"], ref["r32"], ref["s_e"]
    H, L, P = c["H"], c["L"], GC.n_params(c["H"], c["L"])
    bad, worst = GC.compare(c, _as_result(r32), ref, quiet=True)
    assert not bad and worst[0] == 1.0 and worst[4] > 0          # the fp32 oracle against itself: every ratio is 1
    blk = dict(GC.blocks(H, L))

    def planted(edit):
        g = _as_result(r32)
        edit(g)
        bad, _ = GC.compare(c, g, ref, quiet=True)
        old = relnorm(g["gnn"], r64["gnn"]) < 5e-3 and relnorm(g["gode"], r64["gode"]) < 5e-3 and relnorm(g["gx0"], r64["gx0"]) < 5e-3
        return bad, old

    def scale_block(name, f=1e-3):
        def e(g):
            g["gnn"][blk[name]] *= np.float32(1 + f)
        return e

    def one_wave(g):                                             # wave 3's rows of the first hidden matrix
        j0, j1 = GC.row_blocks(c)[3]
        g["gnn"][blk["Wh0"][0] + j0 * H:blk["Wh0"][0] + j1 * H] *= np.float32(1 + 3e-4)

    def move_gode(g):
        e = int(np.argmin(np.where(s_e[0] > 0, np.abs(r64["gode"]) / np.maximum(s_e[0], 1e-300), np.inf)))
        g["gode"][e] += np.float32(1e-4 * s_e[0, e])

    def swap_gx0(g):
        g["gx0"][[7, 8]] = g["gx0"][[8, 7]]

    for label, edit, passes_old in (("tVNS column of W1", scale_block("W1c8"), True), ("bh0", scale_block("bh0"), True), ("one wave's rows", one_wave, True),
                                    ("one gode element", move_gode, True), ("gx0 swapped", swap_gx0, None)):
        bad, old = planted(edit)
        assert bad, f"{label}: not rejected"
        assert passes_old is None or old, f"{label}: the whole-vector criterion sees it too"
    bad, _ = planted(one_wave)
    assert {m.split()[1].split("[")[0] for m in bad} == {"Wh0", "Wh0r3"}, bad
    bad, _ = planted(move_gode)
    assert len(bad) == 1 and " gode[0]" in bad[0], bad
    # a dead row woken: the exact-zero check
    z = next(x for x in GC.CASES["a"] if x["act"] == GC.RELU)
    zref = _refs("a", z["name"])
    g = _as_result(zref["r32"])
    dead = np.flatnonzero((zref["r64"]["gnn"] == 0) & (zref["r32"]["gnn"] == 0))
    assert len(dead) > 0.2 * len(g["gnn"])
    g["gnn"][dead[len(dead) // 2]] = 1e-30
    bad, _ = GC.compare(z, g, zref, quiet=True)
    assert len(bad) == 1 and "exactly 0" in bad[0], bad
