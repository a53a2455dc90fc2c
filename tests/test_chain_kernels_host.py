"""The call-level restatement of the sampler kernels (tests/_chain_reference.py) is right, and the cases the GPU file runs
(tests/_chain_cases.py) are decidable: composed call by call it reproduces the transition-level NUTS restatement the project
already trusts and a textbook HMC step, its dual averaging matches Hoffman & Gelman's closed form, its Welford pass matches
numpy.var, and every decision of every case sits more than 100 rounding bounds from its threshold, in fp32 and in fp64.
CPU only."""
import math

import numpy as np
import pytest

import _chain_cases as K
import _chain_reference as R
import _nuts_reference as nref


# ------------------------------------------------------------------ 1. begin, (pre, likelihood, post, compact)*, finish
def _exit_of(ist, max_depth):
    j, leaf, n_leaf, div = int(ist[R.J]), int(ist[R.LEAF_I]), int(ist[R.N_LEAF]), int(ist[R.DIVERGENT])
    if div:
        return "divergence"
    if n_leaf != 2 ** j - 1:
        return "u-turn inside a subtree"
    return "depth limit" if j >= max_depth else "u-turn of the whole tree"


def test_composed_calls_reproduce_the_transition_level_restatement():
    seen = set()
    for seed in range(6):
        for max_depth, eps in ((1, (0.3, 0.6, 1.0, 1.5, 40.0)), (3, (0.02, 0.3, 0.7, 1.1, 40.0)), (4, (0.02, 0.45, 0.8, 1.1, 3.0)),
                               (6, (0.005, 0.1, 0.2, 0.6, 2.5))):
            cs = K.TreeCase((7, 7, 0), np.float64, max_depth=max_depth, seed=seed)
            cs.log_eps = np.log(np.array(eps))
            out, T, _ = K.drive_tree(cs, K.RefOps(cs))
            st = cs.start()
            for c in range(cs.C):
                r = nref.transition(st["z"][c], st["p"][c], st["g"][c], float(st["U"][c]), float(st["eps"][c]), cs.minv, cs.u_grad,
                                    nref.philox_uniform(cs.seed, c, cs.it), max_depth)
                s6 = out["stats"][c, 1]
                assert (int(s6[4]), int(s6[5]), bool(s6[2])) == (r["tree_depth"], r["n_leapfrog"], r["divergent"]), (seed, max_depth, c)
                np.testing.assert_allclose(out["z"][c], r["z"], rtol=0, atol=1e-12)
                np.testing.assert_allclose(out["g"][c], r["g"], rtol=0, atol=1e-11)
                assert abs(s6[0] - r["accept_stat"]) < 1e-12 and abs(out["U"][c] - r["U"]) < 1e-11
                np.testing.assert_allclose(out["draws"][c, 1, cs.n_ode:], r["z"][cs.n_ode:], rtol=0, atol=1e-12)
                seen.add(_exit_of(T["ist"][c], max_depth))
    assert seen == {"divergence", "u-turn inside a subtree", "u-turn of the whole tree", "depth limit"}, seen


# ------------------------------------------------------------------ 2. refresh, leapfrog*, accept = textbook HMC
@pytest.mark.parametrize("cmap", [(0, 1, 9), (K.SPARSE_MASK, 1, 4), (K.THREE_MASK, 1, 6)])
def test_composed_calls_reproduce_textbook_hmc(cmap):
    D, C, L, seed, it = 9, 4, 7, 5, 2
    n_ode, P = K.n_ode_of(cmap), cmap[2]
    idx = R.ode_indices(cmap[0])
    g = np.random.default_rng(3)
    mu, sd = g.uniform(0.5, 2, n_ode), g.uniform(0.1, 0.5, n_ode)
    a, b = g.uniform(0.2, 2, D), g.standard_normal(D)
    minv = g.uniform(0.5, 2, D)
    z = g.standard_normal((C, D))
    log_eps = np.log(np.array([0.05, 0.2, 0.6, 3.0]))

    def theta(zr):
        return np.concatenate([mu + sd * zr[:n_ode], zr[n_ode:]])

    def u_grad(zr):                                        # U = 0.7 sum a (theta - b)^2 + |z|^2 / 2
        d = theta(zr) - b
        return 0.7 * float(np.sum(a * d * d)) + 0.5 * float(zr @ zr), 0.7 * 2 * a * d * np.concatenate([sd, np.ones(P)]) + zr

    def lik(nn_p, ode_p):                                  # what the driver's solve + adjoint return for these parameters
        th = np.concatenate([ode_p[:, idx], nn_p[:, :P]], axis=1)
        gt = 0.7 * 2 * a * (th - b)
        gode = np.full((C, 17), 1e30)
        gode[:, idx] = gt[:, :n_ode]
        return gt[:, n_ode:], gode, np.sum(a * (th - b) ** 2, axis=1)

    U, gr = map(np.array, zip(*[u_grad(z[c]) for c in range(C)]))
    s = R.refresh(seed, it, 0.1, minv, log_eps, z, gr, U)
    cur = dict(z=z, p=s["p"], g=gr, U=U, ke=np.zeros(C), failed=s["failed"], nn_p=np.zeros((C, max(P, 1))), ode_p=np.zeros((C, 17)))
    kw = dict(cmap=cmap, mu=mu, sd=sd, lik_scale=0.7)
    step = lambda flags, kick, **more: R.leapfrog(flags, kick, s["eps"], minv, cur["z"], cur["p"], cur["g"], cur["U"], cur["ke"],  # noqa: E731
                                                  cur["failed"], nn_p=cur["nn_p"], ode_p=cur["ode_p"], **kw, **more)
    cur = step(R.KICK | R.DRIFT, 0.5)
    for i in range(L):
        gnn, gode, loss = lik(cur["nn_p"], cur["ode_p"])
        last = i == L - 1
        cur = step(R.ASSEMBLE | R.KICK | (R.KE if last else R.DRIFT), 0.5 if last else 1.0, gnn=gnn, gode=gode, loss_sum=loss)
    o = R.accept(R.SAMPLE, seed, it, 0.8, cur["z"], s["z0"], cur["g"], s["g0"], cur["U"], s["U0"], s["ke0"], cur["ke"], cur["failed"],
                 log_eps, np.zeros((C, 4)), np.zeros((C, 2), np.int32), n_ode, mu, sd, np.zeros((C, 1, D)), np.zeros((C, 1, 4)), 0)
    kept = 0
    for c in range(C):                                     # the textbook step, inline
        e = math.exp(log_eps[c]) * (1 + 0.1 * (2 * R.uniform(seed, c, it, R.JITTER, 0) - 1))
        q, p = z[c].copy(), nref.momentum(seed, c, it, minv)
        H_start = U[c] + 0.5 * float(p @ (minv * p))
        gq = gr[c]
        for _ in range(L):
            p = p - 0.5 * e * gq
            q = q + e * minv * p
            Uq, gq = u_grad(q)
            p = p - 0.5 * e * gq
        dH = Uq + 0.5 * float(p @ (minv * p)) - H_start
        div = not math.isfinite(dH) or dH > 1000
        prob = 0.0 if div else min(1.0, math.exp(-dH))
        keep = R.uniform(seed, c, it, R.ACCEPT, 0) < prob
        kept += keep
        want = q if keep else z[c]
        np.testing.assert_allclose(o["z"][c], want, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(o["draws"][c, 0], theta(want), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(o["stats"][c, 0], [prob, -(Uq if keep else U[c]), float(div), 0.0], rtol=1e-10, atol=1e-12)
    assert 0 < kept < C                                    # the largest step is rejected


# ------------------------------------------------------------------ 3. dual averaging: the closed form
def test_dual_average_matches_the_closed_form():
    g = np.random.default_rng(0)
    acc, delta, mu = g.uniform(0, 1, 50), 0.8, math.log(10 * 0.1)
    st = np.array([mu, 0.0, 0.0, 0.0])
    for t in range(1, 51):
        st, le = R.dual_average(st, delta, acc[t - 1])
        hbar = np.sum(delta - acc[:t]) / (t + 10.0)                                   # H bar_t = sum (delta - a_i) / (t + t0)
        le_all = [mu - math.sqrt(i) / 0.05 * np.sum(delta - acc[:i]) / (i + 10.0) for i in range(1, t + 1)]
        ebar = sum(le_all[i - 1] * i ** -0.75 * np.prod([1 - k ** -0.75 for k in range(i + 1, t + 1)]) for i in range(1, t + 1))
        assert abs(st[2] - hbar) < 1e-13 and abs(le - le_all[-1]) < 1e-11 and abs(st[1] - ebar) < 1e-11 and st[3] == t


# ------------------------------------------------------------------ 4. welford: numpy.var of the pooled rows
def test_welford_matches_numpy_var():
    g = np.random.default_rng(1)
    D = 9
    rows = [1e4 + 1e-2 * g.standard_normal((3, D)) for _ in range(3)]
    wf, minv = np.zeros((3, D)), np.full(D, 7.0)
    for z in rows:
        wf, minv = R.welford(R.W_ACCUM, z, wf, minv)
    pooled = np.concatenate(rows)
    np.testing.assert_allclose(wf[1], pooled.mean(0), rtol=1e-15)
    np.testing.assert_allclose(wf[2] / 8, pooled.var(0, ddof=1), rtol=1e-9)
    wf2, minv2 = R.welford(R.W_FINISH, None, wf, minv)
    np.testing.assert_allclose(minv2, 9 / 14 * pooled.var(0, ddof=1) + 1e-3 * 5 / 14, rtol=1e-9)
    assert not wf2.any()
    # one row: n = 1, minv untouched, still reset; and accumulate + finish in one call
    wf1, m1 = R.welford(R.W_ACCUM | R.W_FINISH, rows[0][:1], np.zeros((3, D)), minv)
    assert np.array_equal(m1, minv) and not wf1.any()
    wf3, m3 = R.welford(R.W_ACCUM | R.W_FINISH, pooled, np.zeros((3, D)), minv)
    np.testing.assert_allclose(m3, minv2, rtol=1e-9)


# ------------------------------------------------------------------ 5. the margin condition, no case left out
def _assert_margins(decisions, dtype, what):
    assert decisions, what
    for d in decisions:
        bound = d.bound32 if dtype == np.float32 else d.bound64
        assert d.margin > 100 * bound, (what, d)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=["f32", "f64"])
def test_margin_condition_accept(dtype):
    for D in sorted({lay[0] for lay in K.LAYOUTS}):
        for mode, slot, _, seed, it, n_ode, s in K.accept_edge_cases(D, dtype):
            _assert_margins(K.accept_ref(mode, seed, it, s, n_ode, None, np.zeros((len(K.ACCEPT_EDGES), 3, 4)), slot)["decisions"], dtype,
                            ("accept edges", D, it, mode))
    for D in sorted({lay[0] for lay in K.SEQ_LAYOUTS}):
        s = K.search_grid(D, dtype, 50)
        s["da"] = np.zeros((s["z"].shape[0], 4))
        _assert_margins(K.accept_ref(R.SEARCH, 50, 0, s)["decisions"], dtype, ("search grid", D))
        dec = []
        K.drive_search(D, dtype, 60, lambda it, s: (lambda o: (dec.extend(o["decisions"]), o)[1])(K.accept_ref(R.SEARCH, 60, it, s)))
        _assert_margins(dec, dtype, ("search sequence", D))
        dec = []
        K.drive_adapt(D, dtype, 61, lambda it, s: (lambda o: (dec.extend(o["decisions"]), o)[1])(K.accept_ref(R.ADAPT, 61, it, s)))
        _assert_margins(dec, dtype, ("adapt sequence", D))


@pytest.mark.parametrize("dtype", K.DTYPES, ids=["f32", "f64"])
def test_margin_condition_status_slots(dtype):
    cs = K.status_case(dtype)
    ops = K.RefOps(cs)
    for n_traj, slot, rank, T2 in K.walk_status_slots(cs, ops):
        assert rank.tolist() == [0, -1, 1, -1, 2]
        assert np.flatnonzero(T2["ist"][:, R.FAILED]).tolist() == ([4] if slot == 2 else [])
    _assert_margins(ops.decisions, dtype, "status slots")


@pytest.mark.parametrize("dtype", K.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("layout", K.TREE_LAYOUTS, ids=str)
@pytest.mark.parametrize("max_depth", [4, 1])
def test_margin_condition_trees(layout, dtype, max_depth):
    """Walked with every stored real rounded to the kernel's type.  On the GPU the inputs of the later calls are the kernel's
    own outputs, a few rounding bounds from these: of the factor 100 that leaves more than 90."""
    cs = K.TreeCase(layout, dtype, max_depth=max_depth)
    ops = K.RefOps(cs)
    _, T, alive = K.drive_tree(cs, ops)
    _assert_margins(ops.decisions, dtype, ("tree", layout, max_depth))
    kinds = {d.kind for d in ops.decisions}
    if max_depth == 4:
        assert {_exit_of(T["ist"][c], 4) for c in range(cs.C)} == {"divergence", "u-turn inside a subtree", "u-turn of the whole tree",
                                                                 "depth limit"}
        assert len(set(alive)) >= 3                        # the chains go inactive at different times
        assert kinds == {"direction", "divergence", "leaf", "merge", "uturn_first", "uturn_last", "uturn_tree_v", "uturn_tree_opp"}
