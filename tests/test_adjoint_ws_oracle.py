"""CPU tests of the case table tests/_adjoint_ws_cases.py (the fp32 training adjoint against the fp64 oracle, block by block), from
the oracle alone:

1. admission: what a case must satisfy before the kernel is compared on it -- the status it expects, the same in fp32 and fp64, equal
   step counts, every figure with a non-zero reference (or listed as a structural zero) and an fp32 oracle within 2e-6 of the fp64
   one, off every ReLU kink, and the row bookkeeping the case claims (rows closed by one step, the last taped step of a failed
   trajectory, the NaN trajectory's place in its slot) read from the oracle's tape;
2. the table reaches every instantiation of solve_bwd_ws_kernel<NL, U, GODE, GD> and both atomics launches (ws_launch at 256 CUs);
3. the comparison rejects planted errors the whole-vector criterion lets through."""
import functools

import numpy as np
import pytest

import _adjoint_ws_cases as WC
from _adjoint_ws_cases import relnorm

CUS = 256


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def _refs(part, name):
    return WC.references(_oracle(), WC.find(part, name))


def _path(c, cus):
    return WC.ws_launch(c["B"], c["n_sets"], c["L"], c["want_gode"], cus)


# ------------------------------------------------------------------ 1. admission
def _admit(c, ref=None):
    O = _oracle()
    ref = WC.references(O, c) if ref is None else ref
    d, r64, r32, s_e = ref["d"], ref["r64"], ref["r32"], ref["s_e"]
    B, T, per = c["B"], c["T"], c["B"] // c["n_sets"]
    assert np.array_equal(r64["status"], WC.expected_status(c)), r64["status"]
    assert np.array_equal(r32["status"], r64["status"]) and np.array_equal(r32["nsteps"], r64["nsteps"]), (r32["nsteps"], r64["nsteps"])
    assert np.array_equal(r32["seg"], r64["seg"])
    assert (r64["gnn"] is not None) == c["want_gnn"] and (r64["gode"] is not None) == c["want_gode"]
    # every figure: a non-zero reference (or a listed structural zero), the fp32 oracle within 2e-6
    f32 = WC.figures(c, r32, r64, s_e)
    for key, (err, size) in f32.items():
        if key in WC.structural_zeros(c):
            assert (size == 0).all(), key
            continue
        assert (size > 0).all() and np.isfinite(size).all(), (key, np.flatnonzero(~(size > 0))[:4])
        assert err.max() <= WC.D_REF_MAX, (key, int(err.argmax()), float(err.max()))
    # smoothness: no ReLU kink within 1e-6 of the inputs
    p64 = WC.oracle_run(O, c, "f64", d, scale_inputs=1 + 1e-6)
    assert np.array_equal(p64["nsteps"], r64["nsteps"])
    for key, (err, _) in WC.figures(c, p64, r64, s_e).items():
        assert err.max() < 1e-5, (key, float(err.max()))
    # the row bookkeeping the case is about, from the tape's interval words
    tb = d["t"] if c["t_batched"] else np.tile(d["t"], (B, 1))
    if c["closes"] is not None:
        runs = list(c["some_runs"]["trajs"]) if c["some_runs"] else range(B)
        for b in range(B):
            cl = WC.closes(r64["seg"][b], r64["nsteps"][b], T)
            assert max(cl) == (c["closes"] if b in runs else 1), (b, cl)
    if c["kf"] is not None:
        assert ((r64["seg"][:, 0] & (WC.SEG_CLOSED - 1)) == c["kf"]).all() and not (tb[:, c["kf"]] > tb[:, 0]).any()
    if c["last_open"] is not None:
        assert (r64["nsteps"] == c["max_steps"]).all()
        last = r64["seg"][np.arange(B), r64["nsteps"] - 1]
        k = last & (WC.SEG_CLOSED - 1)
        assert (((last & WC.SEG_CLOSED) == 0) == c["last_open"]).all(), last
        assert (k >= 1).all()                                   # an earlier step closed a row: the gradient is not just gy[:, 0]
        if not c["last_open"]:
            # zero-length copies behind the closed interval (the kSegClosed branch walks them), and a longer grid behind those
            assert (~(tb[np.arange(B), k + 2] > tb[np.arange(B), k + 1])).all() and (k + 3 < T).all()
    if c["gd_zero_rows"]:
        assert (d["u"][2][:, list(c["gd_zero_rows"])] == 0).all()
    if c["part"] == "c":
        nan = WC.nan_trajectories(c)
        blocks, U = c["path"][1], c["path"][2]
        for s in range(c["n_sets"]):
            st = r64["status"][s * per:(s + 1) * per]
            assert (st == 3).sum() == 1 and st[nan[s] - s * per] == 3 and r64["nsteps"][nan[s]] == 0
            wg, slot, rnd = WC.slot_of(int(nan[s]) - s * per, blocks, U)
            assert rnd == 0 and WC.slot_counts(per, blocks, U)[wg, slot] == 2
            behind = nan[s] + blocks * WC.kWsP * U              # the slot's next trajectory: live
            assert behind < (s + 1) * per and r64["nsteps"][behind] > 0
        assert (r64["status"] == 1).sum() >= 5
        assert len({int(n) for n in r64["nsteps"]}) >= 3        # mixed lengths
        short = r64["nsteps"][::c["ends_every"]]
        assert (r64["status"][::c["ends_every"]][short > 0] == 0).all()


@pytest.mark.parametrize("part", list(WC.CASES))
def test_every_case_is_admissible(part):
    for c in WC.CASES[part]:
        try:
            _admit(c, _refs(part, c["name"]))
        except AssertionError as e:
            raise AssertionError(f"case {part}/{c['name']} (seed {c['seed']}): {e}") from e


# ------------------------------------------------------------------ 2. coverage
def test_launch_arithmetic():
    assert WC.ws_launch(4096, 1, 4, False, 256) == ("ws", 256, 2) and WC.ws_launch(4096, 1, 4, True, 256) == ("ws", 256, 1)
    assert WC.ws_launch(2048, 1, 4, False, 256) == ("ws", 256, 1) and WC.ws_launch(7, 1, 2, False, 256) == ("ws", 7, 1)
    assert WC.ws_launch(258, 3, 3, False, 256) == ("ws", 85, 1)
    assert WC.ws_launch(4096, 1, 1, False, 256) == ("fused", 256, False) and WC.ws_launch(4096, 1, 4, False, 256, "f64") == ("fused", 256, False)
    assert WC.ws_launch(1024, 1024, 2, False, 256) == ("ws", 1, 1) and WC.ws_launch(1025, 1025, 2, False, 256) == ("fused", 1, True)
    assert WC.ws_launch(2050, 1025, 2, False, 256) == ("fused", 1, True) and WC.ws_launch(4096, 2, 1, True, 304) == ("fused", 152, False)
    n = WC.slot_counts(70, 4, 2)
    assert n.shape == (4, 16) and n.sum() == 70 and n.max() == 2 and (n == 2).sum() == 6 and (n[:, 0] == 2).all() and (n[:2, 1] == 2).all()
    seen = sorted(WC.slot_of(bi, 4, 2) for bi in range(70))
    assert len(set(seen)) == 70 and all(r <= 1 for _, _, r in seen)


def test_the_table_covers_every_instantiation():
    inst = {}
    for c in WC.CASES["a"] + WC.CASES["b"] + WC.CASES["c"]:
        path = _path(c, CUS)
        assert path == c["path"], (c["name"], path)
        assert path[0] == "ws" and c["H"] <= 64 and 2 <= c["L"] <= 4
        inst.setdefault((c["L"], path[2], c["want_gode"], c["modes"][2] != 0), []).append(c)
    want = {(nl, 1, gode, gd) for nl in (2, 3, 4) for gode in (False, True) for gd in (False, True)} | \
           {(nl, 2, False, gd) for nl in (2, 3, 4) for gd in (False, True)}
    assert set(inst) == want and len(want) == 18
    a = [c for c in WC.CASES["a"] if c["n_sets"] == WC.N_SETS_A]
    assert len(a) == 18 and {c["H"] for c in a} == {64, 33, 16, 7} and sum(c["H"] == 64 and c["L"] == 4 for c in a) <= 2
    for nl in (2, 3, 4):
        for U in (1, 2):
            assert {c["method"] for c in a if c["L"] == nl and c["path"][2] == U} == {WC.RK4, WC.DP5}, (nl, U)
    # the slots in use: all 8 once / 8 slots a second trajectory / 16 slots, some a second, the last round ragged
    for c in a:
        n = WC.slot_counts(c["B"] // c["n_sets"], c["path"][1], c["path"][2])
        if c["path"][2] == 2:
            assert n.shape == (4, 16) and n.min() == 1 and n.max() == 2 and 0 < (n == 2).sum() < n.size and len(set(n.sum(1))) > 1
        elif c["want_gode"]:
            assert n.shape == (4, 8) and n.min() == 1 and (n == 2).sum() == 8
        else:
            assert n.shape == (4, 8) and (n == 1).all()
    single = WC.find("a", "nl3-u2-single-B2100-h33-dp5")
    n = WC.slot_counts(single["B"], 256, 2)
    assert _path(single, CUS) == ("ws", 256, 2) and n.sum() == 2100 and n.max() == 1 and n.min() == 0 and (n[:, :8] == 1).all()
    for c in WC.CASES["d"]:
        assert _path(c, CUS) == c["path"], (c["name"], _path(c, CUS))
    d = {c["name"]: c for c in WC.CASES["d"]}
    assert sum(c["path"] == ("fused", 1, True) for c in d.values()) == 2
    assert {(c["H"], c["L"]) for c in d.values() if c["path"][0] == "fused" and c["path"][2]} == {(16, 2), (64, 4)}
    assert sum(c["path"] == ("ws", 1, 1) and c["n_sets"] > CUS for c in d.values()) >= 1
    assert {(c["H"], c["want_gode"]) for c in d.values() if c["L"] == 1} == {(16, False), (16, True), (64, False), (64, True)}
    # the measured margins: 8, or twice the largest ratio where that exceeds 4
    for part, m in WC.MARGIN.items():
        r = WC.MEASURED[part][1] if part in WC.MEASURED else 0.0
        assert m == (8.0 if r <= 4 else round(2 * r, 1)), part


# ------------------------------------------------------------------ 3. planted errors
def _as_result(r):
    return {k: (None if r[k] is None else r[k].copy()) for k in ("status", "nsteps", "gx0", "gnn", "gode")}


def test_the_comparison_rejects_planted_errors():
    """The comparison of the GPU file, run on the fp32 ORACLE's result with one error planted at a time.  The first three pass the old
    criterion (whole-vector relnorm < 1e-4): that is the gap these tests close."""
    c = WC.find("a", "nl4-u1-gode1-gd0-h16-m120-rk4")
    assert c["modes"][1] != 0 and c["want_gode"] and c["method"] == WC.RK4
    ref = _refs("a", c["name"])
    r64, r32, s_e = ref["r64"], ref["r32"], ref["s_e"]
    H, L, ns, P = c["H"], c["L"], c["n_sets"], WC.n_params(c["H"], c["L"])
    clean = _as_result(r32)
    bad, worst = WC.compare(c, clean, ref, quiet=True)
    assert not bad and worst[0] == 1.0                          # the fp32 oracle against itself: every ratio is 1
    blk = dict(WC.blocks(H, L))

    def planted(edit):
        g = _as_result(r32)
        edit(g)
        bad, _ = WC.compare(c, g, ref, quiet=True)
        old = relnorm(g["gnn"], r64["gnn"]) < 1e-4 and relnorm(g["gode"], r64["gode"]) < 1e-4 and relnorm(g["gx0"], r64["gx0"]) < 1e-4
        return bad, old

    def scale_block(name):
        def f(g):
            g["gnn"].reshape(ns, P)[:, blk[name]] *= np.float32(1 + 1e-4)
        return f

    def move_gode(g):
        e = int(np.argmin(np.where(s_e[5] > 0, np.abs(r64["gode"].reshape(ns, 17)[5]) / np.maximum(s_e[5], 1e-300), np.inf)))
        g["gode"].reshape(ns, 17)[5, e] += np.float32(1e-4 * s_e[5, e])

    def swap_gx0(g):
        g["gx0"][[7, 8]] = g["gx0"][[8, 7]]

    def shift_sets(g):
        v = g["gnn"].reshape(ns, P)
        v[3] = r32["gnn"].reshape(ns, P)[4]

    def wake_dead_row(g):
        dead = np.flatnonzero((r64["gnn"] == 0) & (r32["gnn"] == 0))
        assert len(dead) > 0.4 * len(r64["gnn"])
        g["gnn"][dead[len(dead) // 2]] = 1e-30

    for label, edit, passes_old in (("tVNS column of W1", scale_block("W1c8"), True), ("bh1", scale_block("bh1"), True),
                                    ("one gode element", move_gode, True), ("gx0 swapped", swap_gx0, None),
                                    ("set slice from the neighbour", shift_sets, None), ("dead row", wake_dead_row, None)):
        bad, old = planted(edit)
        assert bad, f"{label}: not rejected"
        assert passes_old is None or old, f"{label}: the whole-vector criterion sees it too"
    # each planted error is the only thing reported
    bad, _ = planted(scale_block("W1c8"))
    assert all(" W1c8[" in m for m in bad), bad[:3]
    bad, _ = planted(move_gode)
    assert len(bad) == 1 and " gode[5]" in bad[0], bad
