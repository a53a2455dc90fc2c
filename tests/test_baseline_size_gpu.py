"""BASELINE.json configs 2, 3 and 5 at (or next to) their full size, checked against the ORACLE -- not against another run of
the HIP path -- plus the failure statuses of the regime the reference's dataset really feeds (z-scored states,
/root/reference/train/train_hybrid.py:139) and of its tests' stress states.  `-m gpu`; every call goes through the C ABI.

The `test_cfg*` names sort these first in the suite (tests/conftest.py)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import bench  # noqa: E402  (the benchmark's own cohort / weight generators)
from oracle import oracle as O  # noqa: E402  (checker only)

H, L, T = 64, 4, 241
NCPU = max(1, min(os.cpu_count() or 1, 16))


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def relnorm(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def oracle_fwd_bwd(x0, t, meal, tvns, ode, nn, cot, rtol=1e-10, atol=1e-12, dtype=np.float64, chunk=4, max_steps=None):
    """fp64 oracle solve + adjoint over chunks of trajectories on all host cores (ctypes releases the GIL).
    cot(y_chunk, lo, hi) -> dLoss/dy of that chunk.  Returns y, status, gx0, gnn (summed), gode (summed)."""
    B = x0.shape[0]

    def work(lo):
        hi = min(lo + chunk, B)
        s = O.solve(x0[lo:hi], t if t.ndim == 1 else t[lo:hi], meal[lo:hi], tvns[lo:hi], None, ode, nn, H, L, rtol=rtol, atol=atol,
                    dtype=dtype, want_tape=True, max_steps=max_steps)
        gx, gn, go = O.solve_bwd(s, cot(s.y, lo, hi))
        return lo, hi, s.y, s.status, s.nsteps, gx, gn, go
    with ThreadPoolExecutor(NCPU) as ex:
        parts = list(ex.map(work, range(0, B, chunk)))
    y = np.concatenate([p[2] for p in parts])
    st = np.concatenate([p[3] for p in parts])
    ns = np.concatenate([p[4] for p in parts])
    gx = np.concatenate([p[5] for p in parts])
    return y, st, ns, gx, sum(p[6] for p in parts), sum(p[7] for p in parts)


@pytest.fixture(scope="module")
def hode():
    import hode as h
    h.load()
    return h


# ------------------------------------------------------------------------------------------------------------------------
# failure statuses
def _failure_cohort():
    """256 patients of bench.py's z-scored cohort (x0 ~ N(0,1)^6, seed 4242, the benchmark's meals) + the reference's stress states
    (tests/test_ode_jacobians.py:173-206 `extreme_states`; tests/test_gradient_correctness.py:211-256 x0 = 10 randn, meals up to
    50, tVNS = 1) + states that cannot be integrated at all: NaN / Inf in x0, a NaN in the meal row half way, states exactly ON
    the poles GLP1 = -EC_50 and G = -K_m (models/ode_core.py:129-135 divides by zero there; SURVEY 8a: "no clamping")."""
    _, t, meal, tvns = (v.numpy().astype(np.float64) for v in bench.synth_cohort(4096, 1000))
    xz = torch.randn(4096, 6, generator=torch.Generator().manual_seed(4242)).numpy().astype(np.float64)[:256]
    mz, vz = meal[:256].copy(), tvns[:256].copy()
    g = torch.Generator().manual_seed(5)
    ext = np.array([[20.0, 500.0, 200.0, 100.0, 2.0, 5.0], [2.0, 10.0, 10.0, 5.0, 0.0, 0.1], [5.0, 100.0, 50.0, 20.0, 0.0, 1.0]])
    xs = np.concatenate([ext, (torch.randn(29, 6, generator=g) * 10).numpy().astype(np.float64)])
    ms = np.zeros((32, T))
    ms[:, ::4] = (torch.rand(32, 61, generator=g) * 50).numpy()            # large meal inputs on every fourth grid point
    vs = np.ones((32, T))
    base = np.array([5.0, 60.0, 80.0, 10.0, 0.0, 1.0])
    xb = np.tile(base, (8, 1))
    mb, vb = np.zeros((8, T)), np.zeros((8, T))
    xb[0, 2] = np.nan                    # missing value in the initial state
    xb[1, 0] = np.inf
    mb[2, 100] = np.nan                  # missing value in an input row: fails in interval 99, rows 0..99 are good
    xb[3, 3] = -50.0                     # GLP1 = -EC_50: GLP1 / (EC_50 + GLP1) = -50 / 0, non-finite at every step size
    mb[4, 7] = 1.0                       # healthy neighbours in the same launch
    xb[5, 0] = -7.0                      # G = -K_m: V_max G / (K_m + G)
    x0 = np.concatenate([xz, xs, xb])
    return x0, t, np.concatenate([mz, ms, mb]), np.concatenate([vz, vs, vb])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cfg2_failure_statuses_rows_and_adjoint_match_oracle(hode, dtype):
    """Reference behaviour on a failed integration (models/hybrid_ode_nn.py:243-256): warn, keep the rows computed so far, zeros
    beyond.  Here: per-trajectory status 2 (step size underflow: the pole of G/(K_m+G) or GLP1/(EC_50+GLP1) is reached in finite
    time -- what SciPy reports as 'Required step size is less than spacing between numbers') and 3 (non-finite state) must BOTH
    occur and equal the oracle's, trajectory by trajectory; nsteps within 1; rows written before the failure agree; rows after
    it are exactly zero; and the ADJOINT of such a batch equals the oracle's adjoint (failed trajectories contribute the
    cotangents of the rows they wrote, nothing else; healthy neighbours are untouched; nothing non-finite leaks into the
    shared parameter gradient)."""
    npd = np.float32 if dtype == torch.float32 else np.float64
    x0, t, meal, tvns = _failure_cohort()
    B = x0.shape[0]
    nn, ode = bench.synth_weights(0).numpy().astype(np.float64), bench.ODE_DEFAULT.numpy().astype(np.float64)
    max_steps = 8 * (T - 1) + 64
    rng = np.random.default_rng(11)
    c = rng.standard_normal((B, T, 6)) / (B * T * 6)
    c[B - 8, 3, :] = np.nan                 # a cotangent on a row that was never written (failed at row 0) must be ignored ...
    c[B - 6, 150, :] = np.inf               # ... also far behind the failure (NaN meal at grid index 100)
    with np.errstate(all="ignore"):
        yo, sto, nso, gxo, gno, goo = oracle_fwd_bwd(x0.astype(npd), t.astype(npd), meal.astype(npd), tvns.astype(npd), ode, nn,
                                                    lambda y, lo, hi: c[lo:hi].astype(npd), rtol=1e-6, atol=1e-8, dtype=npd,
                                                    max_steps=max_steps)
    assert (sto == 2).sum() >= 3 and (sto == 3).sum() >= 3 and (sto == 0).sum() >= 250, np.bincount(sto, minlength=4)
    s = hode.solve_fwd(dev(x0, dtype), dev(t, dtype), dev(meal, dtype), dev(tvns, dtype), None, dev(ode, dtype), dev(nn, dtype), H, L,
                       rtol=1e-6, atol=1e-8, want_tape=True, max_steps=max_steps)
    st, ns, y = s.status.cpu().numpy(), s.nsteps.cpu().numpy(), s.y.cpu().numpy().astype(np.float64)
    assert np.array_equal(st, sto), (np.nonzero(st != sto)[0], st[st != sto], sto[st != sto])
    ok = sto == 0
    f32 = dtype == torch.float32
    m = {"status_counts": np.bincount(sto, minlength=4).tolist()}
    # a trajectory that dies on a pole takes ever smaller steps: the last accepted ones are a matter of the last bit
    m["dnsteps_ok"], m["dnsteps_failed"] = int(np.abs(ns[ok] - nso[ok]).max()), int(np.abs(ns[~ok] - nso[~ok]).max())
    err_ok, err_pre, kz_diff, tail_nonzero, nonfinite_rows = 0.0, 0.0, 0, 0, 0
    for b in range(B):
        written_o = np.nonzero(np.any(yo[b] != 0, axis=1))[0]
        kz_o = written_o.max() + 1 if written_o.size else 0                 # first row the oracle left at zero
        written = np.nonzero(np.any(y[b] != 0, axis=1))[0]
        kz = written.max() + 1 if written.size else 0
        kz_diff = max(kz_diff, abs(kz - kz_o))
        if ok[b]:
            err_ok = max(err_ok, float(np.max(np.abs(y[b] - yo[b]) / (np.abs(yo[b]) + 1e-3))))
        else:
            tail_nonzero += int(np.count_nonzero(y[b, kz:]))
            nonfinite_rows += int(np.count_nonzero(~np.isfinite(y[b, 1:])))  # (row 0 echoes x0, NaN / Inf included)
            if kz > 3:        # the rows next to a pole are ill-conditioned (dx/dt ~ 1/(K_m+G)): up to three rows before the end
                err_pre = max(err_pre, float(np.max(np.abs(y[b, :kz - 3] - yo[b, :kz - 3]) / (np.abs(yo[b, :kz - 3]) + 1e-3))))
    m.update(err_ok=err_ok, err_before_failure=err_pre, first_zero_row_diff=kz_diff, nonzero_after_failure=tail_nonzero,
             nonfinite_rows=nonfinite_rows)
    # ---- adjoint of the same batch
    gx0, gnn, gode = hode.solve_bwd(s, dev(c, dtype), want_gode=True)
    gx0, gnn, gode = gx0.cpu().numpy(), gnn.cpu().numpy(), gode.cpu().numpy()
    m["grads_finite"] = bool(np.all(np.isfinite(gnn)) and np.all(np.isfinite(gode)) and np.all(np.isfinite(gno)) and np.all(np.isfinite(goo))
                             and np.all(np.isfinite(gx0[ok])) and np.all(np.isfinite(gx0[sto == 2])))
    m["gx0_ok"] = relnorm(gx0[ok], gxo[ok])
    m["gx0_ok_worst"] = max(relnorm(gx0[b], gxo[b]) for b in np.nonzero(ok)[0])
    # trajectories that failed at row 0 wrote nothing but row 0 itself: gx0 = the cotangent of row 0
    dead = np.array([B - 8, B - 7, B - 5, B - 3])
    m["dead_gx0_is_row0_cotangent"] = bool(np.allclose(gx0[dead], c[dead, 0, :], rtol=1e-6, atol=0) and
                                           np.allclose(gxo[dead], c[dead, 0, :], rtol=1e-6, atol=0))
    # status-2 trajectories: the adjoint walks up to the pole; trajectory by trajectory, relative to each one's own size
    m["gx0_status2_worst"] = max(relnorm(gx0[b], gxo[b]) for b in np.nonzero(sto == 2)[0])
    # the shared parameter gradient: dominated by whatever the near-pole steps contribute, still the same vector
    m["gnn_all"], m["gode_all"] = relnorm(gnn, gno), relnorm(gode, goo)
    # ... and with the failed trajectories' cotangents zeroed (they still walk their tapes, with zero cotangents: nothing
    # non-finite may leak out of them)
    c2 = c.copy()
    c2[~ok] = 0.0
    with np.errstate(all="ignore"):
        _, _, _, gxo2, gno2, goo2 = oracle_fwd_bwd(x0.astype(npd), t.astype(npd), meal.astype(npd), tvns.astype(npd), ode, nn,
                                                   lambda y_, lo, hi: c2[lo:hi].astype(npd), rtol=1e-6, atol=1e-8, dtype=npd,
                                                   max_steps=max_steps)
    gx2, gnn2, gode2 = (v.cpu().numpy() for v in hode.solve_bwd(s, dev(c2, dtype), want_gode=True))
    m.update(gnn_ok_only=relnorm(gnn2, gno2), gode_ok_only=relnorm(gode2, goo2), gx0_ok_only=relnorm(gx2[ok], gxo2[ok]),
             failed_gx0_zero=bool(np.all(gx2[~ok] == 0.0)))
    # yardstick for the healthy z-scored trajectories: what the SAME algorithm moves when only the arithmetic changes (oracle fp32
    # vs oracle fp64 at the same tolerances).  They run close to the poles before they escape, which amplifies the last bits
    if f32:
        with np.errstate(all="ignore"):
            y64, st64, *_ = oracle_fwd_bwd(x0, t, meal, tvns, ode, nn, lambda y_, lo, hi: c[lo:hi], rtol=1e-6, atol=1e-8, dtype=np.float64,
                                           max_steps=max_steps)
        both = ok & (st64 == 0)
        m["oracle_fp32_vs_fp64_ok"] = float(np.max(np.abs(yo[both] - y64[both]) / (np.abs(y64[both]) + 1e-3)))
        # ... and the bar itself: the fp32 KERNEL against the fp64 oracle at CONVERGED tolerances (1e-10 / 1e-12).
        # Where does the pointwise figure above come from?  Not from the poles: the healthy trajectories stay 3.5 away from
        # G = -K_m and 11 from GLP1 = -EC_50 (printed below; measured on the kernel's run).  z-scored components CROSS ZERO, and |dy| / (|y| + 1e-3) at a point
        # where |y| = 2e-5 on a component that ranges over +-3.6 turns an error of 4e-6 into "3.7e-3".  So the healthy
        # trajectories are held to north_star's 1e-3 in the two readings that mean something there: (i) every point whose
        # |y| is at least 1 % of its component's range on that trajectory, relative to |y|; (ii) every other point (the zero
        # crossings), relative to that range.
        with np.errstate(all="ignore"):
            yc, stc, *_ = oracle_fwd_bwd(x0, t, meal, tvns, ode, nn, lambda y_, lo, hi: c[lo:hi], rtol=1e-10, atol=1e-12, dtype=np.float64,
                                         max_steps=64 * (T - 1))
        hc = ok & (stc == 0)
        hc[256:] = False                                                    # the z-scored cohort (the stress states behind it: err_ok above)
        rng_c = np.max(np.abs(yc), axis=1, keepdims=True) + 1e-300          # [B, 1, 6]: the range of every component on every trajectory
        big = np.abs(yc) >= 1e-2 * rng_c
        d = np.abs(y - yc)
        m["vs_converged_fp64"] = {
            "healthy": int(hc.sum()),
            "points_away_from_zero": int(big[hc].sum()), "rel_err_away_from_zero": float(np.max(np.where(big, d / (np.abs(yc) + 1e-300), 0.0)[hc])),
            "points_at_zero_crossings": int((~big)[hc].sum()), "err_over_range_at_zero_crossings": float(np.max(np.where(big, 0.0, d / rng_c)[hc])),
            "err_over_range_anywhere": float(np.max((d / rng_c)[hc])),
            "min_distance_to_G_pole": float(np.min(np.abs(ode[9] + yc[hc][:, :, 0]))),
            "min_distance_to_GLP1_pole": float(np.min(np.abs(ode[6] + yc[hc][:, :, 3])))}
    print("failure-regime metrics", "fp32" if f32 else "fp64", m)
    assert np.all(sto[dead] >= 2) and np.all(sto[dead[:3]] == 3)      # (the G pole ends in a zero initial step: status 2)
    assert m["dnsteps_ok"] <= 1 and m["dnsteps_failed"] <= 3
    assert m["first_zero_row_diff"] == 0 and m["nonzero_after_failure"] == 0 and m["nonfinite_rows"] == 0
    # z-scored states run close to the poles before they either escape or die: same algorithm, same dtype, but the kernel's
    # fp32 forms (v_rcp_f32 instead of a division, ...) differ in the last bits and the poles amplify that.  fp64 is held to
    # north_star's fp64 bar; fp32 to twice what fp32 arithmetic itself moves these trajectories in the oracle (measured 1.1e-3
    # against a yardstick of the same size), and to the fp32 bar of 1e-3 on the rows before a failure
    assert m["err_ok"] < (max(2e-5, 2 * m["oracle_fp32_vs_fp64_ok"]) if f32 else 1e-5), m
    if f32:
        v = m["vs_converged_fp64"]
        assert v["healthy"] >= 250 and v["rel_err_away_from_zero"] < 1e-3 and v["err_over_range_at_zero_crossings"] < 1e-4, v
        assert v["err_over_range_anywhere"] < 1e-4, v                       # measured 4e-6
    assert m["err_before_failure"] < (1e-3 if f32 else 1e-5)
    assert m["grads_finite"] and m["dead_gx0_is_row0_cotangent"] and m["failed_gx0_zero"]
    # measured: fp32 1e-6 (healthy) / 6e-4 (status 2, per trajectory) / 2e-4 (shared gradient with the near-pole steps in it);
    # fp64 1e-11 or better throughout
    assert m["gx0_ok"] < (1e-4 if f32 else 1e-8) and m["gx0_ok_worst"] < (1e-3 if f32 else 1e-8)
    assert m["gx0_status2_worst"] < (1e-2 if f32 else 1e-8)
    assert m["gnn_all"] < (5e-3 if f32 else 1e-8) and m["gode_all"] < (1e-3 if f32 else 1e-8)
    assert m["gnn_ok_only"] < (1e-4 if f32 else 1e-8) and m["gode_ok_only"] < (1e-4 if f32 else 1e-8) and m["gx0_ok_only"] < (1e-4 if f32 else 1e-8)


def test_rk4_blow_up_is_status_3_and_never_reaches_the_tape(hode):
    """a fixed-step RK4 step whose result is not finite is not an accepted step -- it is not on the tape, its row is
    not written, and the adjoint of the batch stays finite (the shared gnn / gode must not be poisoned by one patient)."""
    Tn = 21
    t = np.linspace(0.0, 20.0, Tn)                    # one-hour RK4 steps
    base = np.array([5.0, 60.0, 80.0, 10.0, 0.0, 1.0])
    x0 = np.tile(base, (6, 1))
    x0[1, 5] = 1.0e30                                 # FFA: (p9 G - p7 - p8 I) F with h = 1 overflows fp32 after a few steps
    x0[4, 1] = 3.0e38
    meal = np.zeros((6, Tn))
    meal[:, 3] = 1.0
    tv = np.zeros((6, Tn))
    nn, ode = bench.synth_weights(0).numpy(), bench.ODE_DEFAULT.numpy()
    with np.errstate(all="ignore"):
        ref = O.solve(x0, t, meal, tv, None, ode, nn, H, L, method=O.METHOD_RK4, dtype=np.float32, want_tape=True, max_steps=Tn - 1)
    assert (ref.status == 3).sum() >= 1 and (ref.status == 0).sum() >= 4, ref.status
    s = hode.solve_fwd(dev(x0), dev(t), dev(meal), dev(tv), None, dev(ode), dev(nn), H, L, method=hode.METHOD_RK4, want_tape=True,
                       max_steps=Tn - 1)
    assert np.array_equal(s.status.cpu().numpy(), ref.status) and np.array_equal(s.nsteps.cpu().numpy(), ref.nsteps)
    y = s.y.cpu().numpy()
    assert np.all(np.isfinite(y))
    for b in np.nonzero(ref.status == 3)[0]:
        k = int(ref.nsteps[b])                        # rows 0..k were written, the rest is zero
        assert np.all(y[b, k + 1:] == 0) and np.all(ref.y[b, k + 1:] == 0)
    c = np.random.default_rng(2).standard_normal(y.shape).astype(np.float32)
    gx0, gnn, gode = hode.solve_bwd(s, dev(c), want_gode=True)
    with np.errstate(all="ignore"):
        rx, rnn, rode = O.solve_bwd(ref, c)
    assert torch.isfinite(gnn).all() and torch.isfinite(gode).all() and np.all(np.isfinite(rnn))
    okb = ref.status == 0
    assert relnorm(gx0.cpu().numpy()[okb], rx[okb]) < 1e-4


# ------------------------------------------------------------------------------------------------------------------------
# BASELINE config 3 at its size, against the oracle
def test_cfg3_train_step_4096x241_gradients_vs_fp64_oracle_then_adam(hode):
    """One fused training step of BASELINE config 3 -- 4 096 patients x 241 grid points: forward with tape, fused MSE +
    cotangent, adjoint, clip + Adam.  The gradients of THIS launch are compared with the fp64 oracle at converged tolerances:
    gx0 of 32 patients sampled over the whole batch, and the parameter gradient through a 64-patient sub-batch run with the
    same global cotangent scale (the full-batch gradient is its sum with the rest's, checked at 1e-5).  Then the update against
    clip_grad_norm_ + torch.optim.Adam."""
    B = 4096
    x0, t, meal, tvns = bench.synth_cohort(B, 1000)
    nn_t, ode = bench.synth_weights(0), bench.ODE_DEFAULT
    d = torch.device("cuda")
    obs, student = bench.train_problem(d, x0.to(d), t.to(d), meal.to(d), tvns.to(d), ode.to(d), nn_t.to(d), 0)
    n_glob = B * T * 6
    xd, td, md, vd, od = x0.to(d), t.to(d), meal.to(d), tvns.to(d), ode.to(d)

    def step(lo, hi):
        sol = hode.solve_fwd(xd[lo:hi].contiguous(), td, md[lo:hi].contiguous(), vd[lo:hi].contiguous(), None, od, student, H, L, want_tape=True)
        ls, gy = hode.mse_fwd_bwd(sol.y, obs[lo:hi].contiguous(), 1.0 / n_glob)
        gx0, gnn, _ = hode.solve_bwd(sol, gy)
        return sol, float(ls), gx0, gnn, gy
    sol, ls, gx0, gnn, gy = step(0, B)
    assert int(sol.status.max()) == 0
    _, ls_a, gx_a, gnn_a, _ = step(0, 64)
    _, ls_b, gx_b, gnn_b, _ = step(64, B)
    assert relnorm((gnn_a + gnn_b).cpu().numpy(), gnn.cpu().numpy()) < 1e-5 and abs(ls_a + ls_b - ls) < 1e-9 * ls
    assert torch.equal(gx0[:64], gx_a)                                    # a trajectory's gx0 does not depend on its batch
    # oracle: the 64-patient sub-batch + 32 patients sampled from the rest
    idx = np.concatenate([np.arange(64), 64 + np.sort(np.random.default_rng(3).choice(B - 64, 32, replace=False))])
    obs_h = obs.cpu().numpy().astype(np.float64)
    p64, ode64 = student.cpu().numpy().astype(np.float64), ode.numpy().astype(np.float64)
    # the cotangent 2 (y - obs) / n is a difference of nearly equal numbers (|y| ~ 80, y - obs ~ 0.1): the fp32 trajectory's
    # 1e-6 relative error is 1e-3 of it.  That is the conditioning of the LOSS, not an error of the adjoint: the fused MSE
    # kernel's cotangent is checked on its own (exactly 2 (y - obs) / n of the kernel's y) and then handed to kernel and oracle alike
    gy_h = gy.cpu().numpy().astype(np.float64)
    yk_all = sol.y.cpu().numpy().astype(np.float64)
    assert np.max(np.abs(gy_h - 2.0 * (yk_all - obs_h) / n_glob)) < 2e-7 * np.max(np.abs(gy_h))
    assert abs(ls - float(((yk_all - obs_h) ** 2).sum())) < 1e-6 * ls
    yo, sto, _, gxo, _, _ = oracle_fwd_bwd(x0.numpy()[idx].astype(np.float64), t.numpy().astype(np.float64), meal.numpy()[idx].astype(np.float64),
                                           tvns.numpy()[idx].astype(np.float64), ode64, p64, lambda y, lo, hi: gy_h[idx[lo:hi]])
    assert int(sto.max()) == 0
    yk = yk_all[idx]
    assert float(np.max(np.abs(yk - yo) / (np.abs(yo) + 1e-3))) < 1e-4          # forward rows of the same 96 patients
    assert abs(float(((yk - obs_h[idx]) ** 2).sum()) - float(((yo - obs_h[idx]) ** 2).sum())) < 1e-4 * float(((yo - obs_h[idx]) ** 2).sum())
    gxk = gx0.cpu().numpy()[idx]
    worst = max(relnorm(gxk[j], gxo[j]) for j in range(len(idx)))
    print("cfg3: worst per-patient gx0 error", worst)
    assert worst < 1e-4, worst
    _, _, _, _, gno, _ = oracle_fwd_bwd(x0.numpy()[:64].astype(np.float64), t.numpy().astype(np.float64), meal.numpy()[:64].astype(np.float64),
                                        tvns.numpy()[:64].astype(np.float64), ode64, p64, lambda y, lo, hi: gy_h[lo:hi])
    assert relnorm(gnn_a.cpu().numpy(), gno) < 1e-4, relnorm(gnn_a.cpu().numpy(), gno)
    # the update: fused clip + Adam kernel vs torch on the full-batch gradient
    p_t = torch.nn.Parameter(student.clone())
    p_t.grad = gnn.clone()
    opt = torch.optim.Adam([p_t], lr=1e-3)
    torch.nn.utils.clip_grad_norm_([p_t], 5.0)
    opt.step()
    p_k, m, v = student.clone(), torch.zeros_like(student), torch.zeros_like(student)
    hode.adam_step(p_k, gnn, m, v, 1e-3, step=1, max_norm=5.0)
    assert float((p_k - p_t.detach()).abs().max()) < 2e-6 and float((p_k - student).abs().max()) > 1e-5


# ------------------------------------------------------------------------------------------------------------------------
# BASELINE config 5 with the real network against the oracle
def _vi_model(M):
    prior = {f"ode_{n}": {"mean": v, "std": 0.02 * v} for n, v in
             [("a_GI", 0.0104), ("k_I", 0.025), ("rho", 0.003), ("E_max", 0.1), ("EC_50", 50.0), ("V_max", 9.0), ("K_m", 7.0), ("k_L", 0.02)]}
    torch.manual_seed(0)
    m = M.HybridODENN(use_variational=True, prior_params=prior, device="cuda")          # the 4 x 64 network
    teacher = bench.synth_weights(0)
    with torch.no_grad():
        off = 0
        for name, p in m.nn_residual.named_parameters():
            m.variational_params.means["nn_" + name.replace(".", "_")].copy_(teacher[off:off + p.numel()].reshape(p.shape))
            off += p.numel()
        for n, p in m.variational_params.log_stds.items():
            p.fill_(-5.0 if n.startswith("nn_") else float(np.log(0.02 * prior[n]["mean"])))
    return m, prior


def test_cfg5_elbo_4x64_16_draws_value_and_gradient_vs_per_draw_oracle(monkeypatch):
    """BASELINE config 5's arithmetic with the REAL network (4 x 64), S = 16 draws x B = 8 patients, T = 61: `elbo()` (one
    launch for all draws, fp64 KL and likelihood, reparameterised gradient through the adjoint) against per-draw fp64 oracle
    solves at converged tolerances: value to 1e-5, d ELBO / d mu of every MLP weight and ODE constant against the oracle's
    adjoint (theta = mu + eps sigma: d theta / d mu = 1, d theta / d log sigma = eps sigma) to 1e-4.  Then the same ELBO
    through the chunked route (tape budget squeezed to two draws per piece): same value, same gradient."""
    import models as M
    import models.hybrid_ode_nn as MH
    m, prior = _vi_model(M)
    S, B, Tn, sigma = 16, 8, 61, 1.0
    x0, t, meal, tvns = bench.synth_cohort(64, 555)
    x0, meal, tvns, t = x0[:B], meal[:B, :Tn].contiguous(), tvns[:B, :Tn].contiguous(), t[:Tn].contiguous()
    with torch.no_grad():
        y_mean = m.forward_with_params({k: v.detach() for k, v in m.variational_params.means.items()}, x0.cuda(), t.cuda(),
                                       {"meal": meal.cuda(), "tVNS": tvns.cuda()})
    obs = y_mean + sigma * torch.randn(y_mean.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    batch = {"initial_state": x0.cuda(), "observations": obs, "time_points": t.cuda(), "external_inputs": {"meal": meal.cuda(), "tVNS": tvns.cuda()}}
    vp = m.variational_params

    def run():
        m.zero_grad()
        torch.manual_seed(21)
        e, comp = m.elbo(batch, n_samples=S, noise_sigma=sigma, return_components=True)
        e.backward()
        return float(e), float(comp["log_likelihood"]), float(comp["kl"]), {n: p.grad.detach().cpu().double().numpy().copy() for n, p in vp.means.items()}, \
            {n: p.grad.detach().cpu().double().numpy().copy() for n, p in vp.log_stds.items()}
    e, ll, kl, gmu, gls = run()
    assert int((m.last_solve_info["status"] != 0).sum()) == 0 and m.last_solve_info["status"].numel() == S * B
    # the same draws, one oracle solve + adjoint per draw
    torch.manual_seed(21)
    draws = vp.sample(S)
    obs_h = obs.cpu().numpy().astype(np.float64)
    # the kernel's own trajectories for these draws (a solve under autograd returns the bits of the no-grad solve): their
    # residuals are the cotangent both adjoints get -- the conditioning of (y - obs) is not the adjoint's business (see cfg3)
    with torch.no_grad():
        y_k = m.forward_param_sets([{k: v.detach() for k, v in d.items()} for d in draws], batch["initial_state"], batch["time_points"],
                                   batch["external_inputs"]).cpu().numpy().astype(np.float64)
    ll_k = sum(-0.5 * float(((y_k[s_] - obs_h) ** 2).sum()) / (sigma ** 2 * S) for s_ in range(S)) - 0.5 * obs_h.size * np.log(2 * np.pi * sigma ** 2)
    assert abs(ll - ll_k) < 1e-9 * abs(ll_k)                     # elbo()'s fp64 likelihood IS that of these trajectories
    xs, ts, ms, vs = (v.numpy().astype(np.float64) for v in (x0, t, meal, tvns))
    ll_o, gmu_o, gls_o = 0.0, {n: np.zeros(p.shape) for n, p in vp.means.items()}, {n: np.zeros(p.shape) for n, p in vp.means.items()}
    names_nn = ["nn_" + n.replace(".", "_") for n, _ in m.nn_residual.named_parameters()]
    from models.ode_core import ODE_PARAM_NAMES
    for si, d in enumerate(draws):
        nn_flat, ode_vec = m._params_on(torch.device("cuda"), d)
        nn64, ode64 = nn_flat.detach().cpu().double().numpy(), ode_vec.detach().cpu().double().numpy()
        yo, sto, _, _, gn, go = oracle_fwd_bwd(xs, ts, ms, vs, ode64, nn64, lambda y, lo, hi: -(y_k[si, lo:hi] - obs_h[lo:hi]) / (sigma ** 2 * S))
        assert float(np.max(np.abs(y_k[si] - yo) / (np.abs(yo) + 1e-3))) < 1e-4
        assert int(sto.max()) == 0
        ll_o += -0.5 * float(((yo - obs_h) ** 2).sum()) / (sigma ** 2 * S)
        off = 0
        for n in names_nn:
            k = int(np.prod(vp.means[n].shape))
            g = gn[off:off + k].reshape(tuple(vp.means[n].shape))
            off += k
            eps_sig = (d[n] - vp.means[n]).detach().cpu().double().numpy()          # eps * sigma of this draw
            gmu_o[n] += g
            gls_o[n] += g * eps_sig
        for i, n in enumerate(ODE_PARAM_NAMES):
            key = "ode_" + n
            if key in gmu_o:
                eps_sig = (d[key] - vp.means[key]).detach().cpu().double().numpy()
                gmu_o[key] += go[i]
                gls_o[key] += go[i] * eps_sig
    ll_o -= 0.5 * obs_h.size * np.log(2 * np.pi * sigma ** 2)
    kl_o = 0.0
    for n in vp.param_shapes:
        mu, ls = vp.means[n].detach().cpu().double().numpy(), vp.log_stds[n].detach().cpu().double().numpy()
        mu_p, s_p = vp.prior_means.get(n, 0.0), vp.prior_stds.get(n, 1.0)
        kl_o += float((np.log(s_p) - ls + (np.exp(2 * ls) + (mu - mu_p) ** 2) / (2 * s_p ** 2) - 0.5).sum())
        gmu_o[n] -= (mu - mu_p) / s_p ** 2
        gls_o[n] -= (-1.0 + np.exp(2 * ls) / s_p ** 2)
    assert abs(kl - kl_o) < 1e-6 * abs(kl_o)
    assert abs(ll - ll_o) < 1e-5 * abs(ll_o), (ll, ll_o)
    assert abs(e - (ll_o - kl_o)) < 1e-5 * abs(ll_o - kl_o)
    flat = lambda dct, keys: np.concatenate([np.asarray(dct[k]).reshape(-1) for k in keys])           # noqa: E731
    ode_keys = [k for k in vp.param_shapes if k.startswith("ode_")]
    assert relnorm(flat(gmu, names_nn), flat(gmu_o, names_nn)) < 1e-4, relnorm(flat(gmu, names_nn), flat(gmu_o, names_nn))
    assert relnorm(flat(gls, names_nn), flat(gls_o, names_nn)) < 1e-4
    ode_err = {k: abs(float(gmu[k]) - float(gmu_o[k])) / (abs(float(gmu_o[k])) + 1e-12) for k in ode_keys}
    print("cfg5: d ELBO / d mu of the ODE constants, relative error", ode_err)
    # eight scalars of very different size, each a sum over 16 x 8 x 360 stages accumulated in ONE fp32 register per constant
    # (hode_adjoint.h mech_vjp).  As a vector in the posterior's own units (gradient x prior width: what an optimiser step on the
    # standardised parameter sees) 1e-3; each on its own 5e-2: rho's net gradient is what is left after d f / d rho =
    # lI GLP1 a_GI (G - G_b) has changed sign with G - G_b along every trajectory (measured 1.4e-2; a_GI 2.5e-4; the others 1e-5)
    sc = np.array([vp.prior_stds.get(k, 1.0) for k in ode_keys])
    gk, gk_o = np.array([float(gmu[k]) for k in ode_keys]) * sc, np.array([float(gmu_o[k]) for k in ode_keys]) * sc
    assert relnorm(gk, gk_o) < 1e-3, (gk, gk_o)
    for k in ode_keys:
        assert ode_err[k] < 5e-2, (k, float(gmu[k]), float(gmu_o[k]))
    # three individual weights, as the reference's FD spot checks pick them
    for name, ix in [("nn_network_0_weight", (3, 2)), ("nn_network_4_weight", (10, 20)), ("nn_network_8_weight", (1, 7))]:
        a, b = float(gmu[name][ix]), float(gmu_o[name][ix])
        # single entries, each a sum with cancellation over 16 draws x 8 patients x 360 stages: against the size of the tensor's
        # gradient (the vector as a whole is held to 1e-4 above; G7's FD spot checks of the reference took 5e-3 of scale)
        assert abs(a - b) < 1e-4 * abs(b) + 5e-4 * float(np.abs(gmu_o[name]).max()), (name, a, b)
    # ---- the chunked route: the tape budget admits two draws (16 trajectories) per piece
    per_traj = __import__("hode").capi.tape_nbytes(1, MH._tape_steps(Tn, 0, None), 4, L, H)
    monkeypatch.setattr(MH, "_tape_budget", lambda dev_, *a: 2 * B * per_traj + 1)
    assert len(MH._pieces(S, B, 2 * B)) == 8
    e2, ll2, kl2, gmu2, gls2 = run()
    assert abs(e2 - e) < 1e-9 * abs(e) and kl2 == kl
    assert relnorm(flat(gmu2, names_nn), flat(gmu, names_nn)) < 1e-5 and relnorm(flat(gls2, names_nn), flat(gls, names_nn)) < 1e-5
    # ... and slices of one draw (budget below one draw's 8 trajectories)
    monkeypatch.setattr(MH, "_tape_budget", lambda dev_, *a: 3 * per_traj + 1)
    e3, _, _, gmu3, _ = run()
    assert abs(e3 - e) < 1e-9 * abs(e) and relnorm(flat(gmu3, names_nn), flat(gmu, names_nn)) < 1e-5


def test_cfg5_posterior_predictive_module_function_equals_the_vi_method():
    """reference models/bayes.py:177-214 `compute_posterior_predictive(model, x_initial, t_span, external_inputs, n_samples)` and
    inference/vi.py:273-312 `VariationalInference.posterior_predictive` draw `sample(1)` n_samples times and reduce over the
    draws: under the same seed they are the same numbers (one launch each here), and equal the draws integrated one at a time."""
    import models as M
    from inference.vi import VariationalInference
    m, _ = _vi_model(M)
    x0, t, meal, tvns = bench.synth_cohort(8, 31)
    x0, t, ext = x0[:3].cuda(), t[:31].contiguous().cuda(), {"meal": meal[:3, :31].contiguous().cuda(), "tVNS": tvns[:3, :31].contiguous().cuda()}
    torch.manual_seed(5)
    mean_a, std_a = M.compute_posterior_predictive(m, x0, t, ext, n_samples=6)
    vi = VariationalInference(m, device=torch.device("cuda"))
    torch.manual_seed(5)
    mean_b, std_b = vi.posterior_predictive(x0, t, ext, n_samples=6)
    assert tuple(mean_a.shape) == (3, 31, 6) and torch.equal(mean_a, mean_b) and torch.equal(std_a, std_b)
    torch.manual_seed(5)
    with torch.no_grad():
        ys = torch.stack([m.forward_with_params(m.sample_posterior(1)[0], x0, t, ext) for _ in range(6)])
    assert torch.equal(ys.mean(0), mean_a) and torch.equal(ys.std(0), std_a) and float(std_a.max()) > 0
    # single patient: (n_time, n_states), as the reference documents
    torch.manual_seed(5)
    m1, s1 = M.compute_posterior_predictive(m, x0[0], t, {k: v[0] for k, v in ext.items()}, n_samples=4)
    assert tuple(m1.shape) == (31, 6) and tuple(s1.shape) == (31, 6)


# ------------------------------------------------------------------------------------------------------------------------
# the wave-specialised adjoint's own geometry
@pytest.mark.parametrize("B", [1, 7, 9, 2100])
def test_ws_adjoint_slot_geometry_ragged_batches_vs_oracle(hode, B):
    """csrc/hode_solve_bwd_ws.hip deals trajectories to 8 (or, above 8 per workgroup, 16) slots per workgroup, slot-major, and runs
    all of them in lock step for as many iterations as the longest slot needs.  Batches that leave slots empty, fill them
    unevenly (2 100 = 256 workgroups x 8 slots + 52: two trajectories per propagation wave, most second trajectories missing),
    trajectories of different length in one workgroup (a batched grid with repeated times shortens some), one that fails at
    row 0 (NaN state: zero steps on the tape) and one whose step budget ends mid-grid: gx0 trajectory by trajectory and the
    parameter gradient against the fp64 oracle fed the same cotangent."""
    Tn = 13
    rng = np.random.default_rng(B)
    base = np.array([5.0, 60.0, 80.0, 10.0, 0.0, 1.0])
    x0 = base * (1 + 0.05 * rng.standard_normal((B, 6)))
    t = np.tile(np.arange(Tn) * (5.0 / 60.0), (B, 1))
    for b in range(0, B, 5):                               # every fifth trajectory: a shorter grid (repeated times at both ends)
        t[b, :3] = t[b, 2]
        t[b, -2:] = t[b, -3]
    meal = (rng.random((B, Tn)) < 0.2).astype(np.float64)
    tv = np.zeros((B, Tn))
    if B >= 7:
        x0[3, 2] = np.nan                                  # status 3 at row 0
    nn, ode = bench.synth_weights(0).numpy().astype(np.float64), bench.ODE_DEFAULT.numpy().astype(np.float64)
    max_steps = Tn - 3 if B == 9 else 2 * Tn               # B = 9: the budget (10 steps for up to 12 intervals) runs out on the full grids
    s = hode.solve_fwd(dev(x0), dev(t), dev(meal), dev(tv), None, dev(ode), dev(nn), H, L, want_tape=True, max_steps=max_steps)
    st = s.status.cpu().numpy()
    c = rng.standard_normal((B, Tn, 6)) / (B * Tn * 6)
    gx0, gnn, gode = (v.cpu().numpy() for v in hode.solve_bwd(s, dev(c), want_gode=True))
    with np.errstate(all="ignore"):
        yo, sto, _, gxo, gno, goo = oracle_fwd_bwd(x0, t, meal, tv, ode, nn, lambda y, lo, hi: c[lo:hi], rtol=1e-6, atol=1e-8, dtype=np.float64,
                                                   max_steps=max_steps, chunk=64)
    assert np.array_equal(st, sto), (st, sto)
    if B == 9:
        assert (st == 1).sum() >= 5
    if B >= 7:
        assert st[3] == 3 and np.allclose(gx0[3], c[3, 0], rtol=1e-6)
    fin = np.isfinite(gxo).all(axis=1)
    assert np.all(np.isfinite(gnn)) and np.all(np.isfinite(gode))
    worst = max(relnorm(gx0[b], gxo[b]) for b in np.nonzero(fin)[0])
    assert worst < 1e-4, worst
    assert relnorm(gnn, gno) < 1e-4 and relnorm(gode, goo) < 1e-3
    gx0b, gnnb, godeb = (v.cpu().numpy() for v in hode.solve_bwd(s, dev(c), want_gode=True))
    assert np.array_equal(gnn, gnnb) and np.array_equal(gode, godeb) and np.array_equal(gx0[fin], gx0b[fin])      # same bits twice
    # without ODE-constant gradients the big batch takes the two-trajectories-per-wave instantiation
    _, gnn2, _ = hode.solve_bwd(s, dev(c))
    assert relnorm(gnn2.cpu().numpy(), gno) < 1e-4


def test_ws_adjoint_two_trajectories_per_wave_with_parameter_sets(hode):
    """The two-trajectories-per-propagation-wave instantiation (more than 8 x 256 trajectories per parameter set, no ODE-constant
    gradients) with MORE THAN ONE parameter set in the launch: the gradient rows of a workgroup belong to its set, the slot
    dealing restarts per set.  Two sets x 2 100 patients in one launch against the two sets launched on their own: gx0 bitwise,
    the per-set parameter gradients to the order of their fp32 sums; and a 24-patient sample of each set against the fp64 oracle."""
    Tn, per = 13, 2100
    rng = np.random.default_rng(17)
    base = np.array([5.0, 60.0, 80.0, 10.0, 0.0, 1.0])
    x0 = np.tile(base * (1 + 0.05 * rng.standard_normal((per, 6))), (2, 1))
    t = np.arange(Tn) * (5.0 / 60.0)
    meal = np.tile((rng.random((per, Tn)) < 0.2).astype(np.float64), (2, 1))
    tv = np.zeros((2 * per, Tn))
    nn0 = bench.synth_weights(0).numpy().astype(np.float64)
    nn1 = nn0 * (1 + 0.1 * rng.standard_normal(nn0.shape))
    ode0 = bench.ODE_DEFAULT.numpy().astype(np.float64)
    ode1 = ode0 * (1 + 0.02 * rng.standard_normal(17))
    nn2, ode2 = np.concatenate([nn0, nn1]), np.concatenate([ode0, ode1])
    c = rng.standard_normal((2 * per, Tn, 6)) / (per * Tn * 6)
    s = hode.solve_fwd(dev(x0), dev(t), dev(meal), dev(tv), None, dev(ode2), dev(nn2), H, L, want_tape=True, n_sets=2)
    assert int(s.status.max()) == 0
    gx, gnn, _ = hode.solve_bwd(s, dev(c))
    P = nn0.size
    assert gnn.numel() == 2 * P
    for k, (nn_k, ode_k) in enumerate(((nn0, ode0), (nn1, ode1))):
        sl = slice(k * per, (k + 1) * per)
        sk = hode.solve_fwd(dev(x0[sl]), dev(t), dev(meal[sl]), dev(tv[sl]), None, dev(ode_k), dev(nn_k), H, L, want_tape=True)
        assert torch.equal(sk.y, s.y[sl])
        gxk, gnk, _ = hode.solve_bwd(sk, dev(c[sl]))
        assert torch.equal(gxk, gx[sl])
        assert relnorm(gnn[k * P:(k + 1) * P].cpu().numpy(), gnk.cpu().numpy()) < 1e-5
        idx = np.sort(rng.choice(per, 24, replace=False)) + k * per
        _, sto, _, gxo, _, _ = oracle_fwd_bwd(x0[idx], t, meal[idx], tv[idx], ode_k, nn_k, lambda y, lo, hi: c[idx[lo:hi]], rtol=1e-6, atol=1e-8,
                                              dtype=np.float64, chunk=24)
        assert int(sto.max()) == 0
        assert max(relnorm(gx.cpu().numpy()[i], gxo[j]) for j, i in enumerate(idx)) < 1e-4
    # the two sets' gradients differ (the launch did not hand one set's rows to the other)
    assert relnorm(gnn[:P].cpu().numpy(), gnn[P:].cpu().numpy()) > 1e-2


def test_many_short_trajectories_per_wave_equal_one_trajectory_per_wave(hode):
    """The physics term of loss() at 4 096 patients is 81 920 two-point solves (reference models/hybrid_ode_nn.py:318-330): above
    8 192 trajectories of <= 4 grid points and one parameter set a wave integrates several, one after the other, with the weights
    loaded once.  Same bits as the launches of <= 8 192 that take the one-trajectory kernel; a sample against the fp64 oracle."""
    B = 20011                                                       # 3 per wave, the last wave short
    x0, _, meal, tvns = bench.synth_cohort(B, 77)
    g = torch.Generator().manual_seed(9)
    x0 = (x0 * (0.5 + torch.rand(B, 6, generator=g))).cuda()
    m, v = (meal[:, 40] * torch.rand(B, generator=g)).cuda().contiguous(), torch.rand(B, generator=g).cuda()
    t = torch.tensor([0.0, 0.1], device="cuda")
    nn, ode = bench.synth_weights(0).cuda(), bench.ODE_DEFAULT.cuda()
    big = hode.solve_fwd(x0, t, m, v, None, ode, nn, H, L)
    parts = [hode.solve_fwd(x0[lo:lo + 8192].contiguous(), t, m[lo:lo + 8192].contiguous(), v[lo:lo + 8192].contiguous(), None, ode, nn, H, L)
             for lo in range(0, B, 8192)]
    assert torch.equal(big.y, torch.cat([p.y for p in parts])) and int(big.status.max()) == 0
    assert torch.equal(big.nsteps, torch.cat([p.nsteps for p in parts])) and torch.equal(big.nfev, torch.cat([p.nfev for p in parts]))
    idx = [0, 1, 2, 8191, 8192, 12345, B - 2, B - 1]
    ref = O.solve(x0[idx].cpu().numpy().astype(np.float64), np.array([0.0, 0.1]), m[idx].cpu().numpy().astype(np.float64),
                  v[idx].cpu().numpy().astype(np.float64), None, ode.cpu().numpy().astype(np.float64), nn.cpu().numpy().astype(np.float64),
                  H, L, rtol=1e-10, atol=1e-12, dtype=np.float64)
    assert relnorm(big.y[idx].cpu().numpy(), ref.y) < 1e-5
