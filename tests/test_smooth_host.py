"""Host-side tests of backward-simulation smoothing: the C ABI's surface and argument validation (no
launch, no GPU), the properties of the numpy restatement tests/_smooth_reference.py that tests/test_smooth_gpu.py holds the
kernel to, and the correctness of the method against a Rauch-Tung-Striebel smoother."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest

import hode

import _filter_reference as FR
import _smooth_cases as SC
import _smooth_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ surface
def test_header_declares_and_capi_binds_the_smoother():
    hdr = open(os.path.join(ROOT, "include", "hode.h")).read()
    declared = set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    lib = hode.load()
    for name in ("hode_pf_smooth_f32", "hode_pf_smooth_f64"):
        assert name in declared and name in hode.capi.SYMBOLS and hasattr(lib, name), name
    assert "Particle smoother" in hdr and callable(hode.capi.pf_smooth)
    philox = open(os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd", "csrc", "hode_philox.h")).read()
    assert re.search(r"kRngFilterSmooth = 10\b", philox) and SR.SMOOTH == 10
    kernel = open(os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd", "csrc", "hode_smooth.hip")).read()
    assert re.search(rf"kTile = {SC.TILE}\b", kernel)              # the GPU cases straddle the kernel's tile


def test_inference_exports_smooth_result():
    import inference
    assert "SmoothResult" in inference.__all__
    from inference.filter import FilterResult, SmoothResult
    assert inference.SmoothResult is SmoothResult and callable(FilterResult.smooth)


def _call(sfx="f32", B=1, N=8, M=4, S=3, link=1, null=()):
    """hode_pf_smooth_* with dummy non-null pointers (never dereferenced: every case here returns before a launch)."""
    names = ["hist", "lwh", "pred", "q", "dt", "idx", "paths"]
    p = {n: C.c_void_p(16 * (k + 1)) for k, n in enumerate(names)}
    for n in null:
        p[n] = C.c_void_p(0)
    f = getattr(hode.load(), f"hode_pf_smooth_{sfx}")
    return f(C.c_void_p(0), C.c_int(B), C.c_int(N), C.c_int(M), C.c_int(S), C.c_uint64(1), C.c_uint32(0), p["hist"], p["lwh"], p["pred"],
             p["q"], p["dt"], C.c_int(link), p["idx"], p["paths"])


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_argument_validation_without_gpu(sfx):
    """Every HODE_EINVAL / HODE_EUNSUPPORTED case of the header returns before a launch."""
    EINVAL, EUNSUPPORTED = -1, -2
    for name in ("B", "N", "M", "S"):
        assert _call(sfx, **{name: 0}) == EINVAL and _call(sfx, **{name: -2}) == EINVAL, name
    assert _call(sfx, link=2) == EINVAL and _call(sfx, link=-1) == EINVAL
    for name in ("hist", "lwh", "pred", "q", "dt", "idx", "paths"):
        assert _call(sfx, null=(name,)) == EINVAL, name
    assert _call(sfx, N=4097) == EUNSUPPORTED
    assert _call(sfx, N=4097, link=5) == EINVAL                    # a bad argument outranks the unsupported size
    assert _call(sfx, N=4097, null=("idx",)) == EINVAL and _call(sfx, N=4097, M=0) == EINVAL


def test_smooth_raises_before_a_device_is_touched():
    import torch
    from inference.filter import FilterResult
    S, B, N = 3, 2, 4
    eng = types.SimpleNamespace(N=N, B=B, seed=0, link=1, q=torch.full((6,), 0.05, dtype=torch.float64), ode_sets=False)
    base = dict(engine=eng, stats=torch.zeros(S, B, 16, dtype=torch.float64), step_index=torch.arange(S), times=torch.arange(S),
                particles=torch.ones(B, N, 6), log_weights=torch.zeros(B, N, dtype=torch.float64), ode_p=torch.ones(B, N, 17), counter=S)
    stored = dict(history=torch.ones(S, B, N, 6), ancestors=torch.zeros(S, B, N, dtype=torch.int32),
                  kept=(torch.ones(S, B, N, 6), torch.zeros(S, B, N, dtype=torch.float64), torch.ones(S, B, dtype=torch.float64)))
    plain = FilterResult(history=None, ancestors=None, **base)
    assert plain.predicted is None and plain.log_weight_history is None and plain.step_dt is None
    with pytest.raises(ValueError, match="store_particles=True"):
        plain.smooth()
    with pytest.raises(ValueError, match="forecast"):
        FilterResult(forecast=True, **base, **stored).smooth()
    eng_sets = types.SimpleNamespace(**dict(vars(eng), ode_sets=True))
    with pytest.raises(ValueError, match="ode_sets"):
        FilterResult(**dict(base, engine=eng_sets), **stored).smooth()
    with pytest.raises(ValueError, match="n_trajectories"):
        FilterResult(**base, **stored).smooth(n_trajectories=0)


def test_smooth_result_moments_distinct_and_lost():
    import torch
    from inference import SmoothResult
    index = torch.tensor([[[0, 1], [0, 2], [3, 2], [-1, 2]]], dtype=torch.int32)              # [B = 1, M = 4, S = 2]
    paths = torch.arange(48, dtype=torch.float32).reshape(1, 4, 2, 6)
    paths[0, 3, 0] = float("nan")
    r = SmoothResult(paths, index, torch.arange(2), torch.arange(2))
    assert r.lost.tolist() == [1] and r.distinct().tolist() == [[2, 2]]
    want0 = paths[0, :3, 0].double()
    assert torch.equal(r.mean[0, 0], want0.mean(0)) and torch.allclose(r.std[0, 0], want0.std(0, unbiased=False))
    assert torch.equal(r.mean[0, 1], paths[0, :, 1].double().mean(0))
    assert torch.equal(r.quantile(0.5)[0, 0], want0.median(0).values) and r.quantile([0.1, 0.9]).shape == (2, 1, 2, 6)


# ------------------------------------------------------------------ the restatement's properties
def _filter(rng, N=40, S=4, link="log", q=None):
    q = np.array([0.05, 0.03, 0.04, 0.02, 0.1, 0.06]) * (SC.SCALE if link == "additive" else 1.0) if q is None else q
    hist, lwh, pred, dt = SC.stored_filter(rng, 1, N, S, link, q)
    return hist[:, 0], lwh[:, 0], pred[:, 0], q, dt[:, 0]


def test_one_candidate_with_all_the_weight_is_taken_by_every_trajectory():
    rng = np.random.default_rng(1)
    hist, lwh, pred, q, dt = _filter(rng)
    lwh[:] = -np.inf
    heavy = [7, 0, 39, 12]
    for s, k in enumerate(heavy):
        lwh[s, k] = 0.3
    r = SR.smooth(hist, lwh, pred, q, dt, 9, seed=4, key=2)
    assert (r["idx"] == np.array(heavy)[:, None]).all() and np.array_equal(r["paths"][:, 0], hist[np.arange(4), heavy])


def test_a_dead_candidate_or_a_nan_pred_row_is_never_chosen():
    rng = np.random.default_rng(2)
    for link in ("log", "additive"):
        hist, lwh, pred, q, dt = _filter(rng, link=link)
        lwh[0, 5] = lwh[2, 11] = -np.inf
        pred[1, 3] = np.nan                                         # slot 3 of step 0 failed its solve
        pred[3, 20, 4] = np.nan                                     # slot 20 of step 2
        pred[2, 8, 0] = -1.0 if link == "log" else np.nan           # the logarithm of a negative number
        r = SR.smooth(hist, lwh, pred, q, dt, 200, seed=1, key=0, link=SC.LINK[link])
        assert (r["idx"] >= 0).all()
        assert not set(r["idx"][0]) & {5, 3} and not set(r["idx"][2]) & {11, 20} and 8 not in set(r["idx"][1])
        assert len(set(r["idx"][0])) > 5                            # (the draws are spread over the others)


def test_every_candidate_dead_loses_the_trajectory_from_there_back():
    rng = np.random.default_rng(3)
    hist, lwh, pred, q, dt = _filter(rng)
    lwh[1] = -np.inf
    r = SR.smooth(hist, lwh, pred, q, dt, 5)
    assert (r["idx"][2:] >= 0).all() and (r["idx"][:2] == -1).all() and np.isnan(r["paths"][:2]).all() and np.isfinite(r["paths"][2:]).all()


def test_with_a_noiseless_state_the_trajectory_is_the_genealogy():
    """A state with q = 0 is carried exactly, so only the true parent (and its identical copies) has a transition density: a
    filter run with the step restatement (a matrix product as the solve) whose state 2 differs between any two particles that
    are not copies of each other; the backward trajectory from slot k of the last step is the ancestor trace from k."""
    rng = np.random.default_rng(4)
    N, S = 48, 6
    A = np.eye(6) * 0.95 + 0.02 * rng.standard_normal((6, 6))
    A[2, 2] = 1.0                  # state 2 has no noise of its own but is fed by the noised ones: its value names the particle
    q = np.array([0.3, 0.2, 0.0, 0.25, 0.3, 0.1])
    sigma = np.full(6, 0.7)
    x = rng.standard_normal((N, 6))
    x[:, 2] = np.arange(N) + 1.0
    lw = np.zeros(N)
    hist, lwh, pred, ancs, dts = [], [], [], [], []
    for s in range(S):
        x_in = x if s == 0 else x @ A.T
        dt = 1.0 if s == 0 else 0.5 + rng.random()
        r = FR.step(x_in, x_in.mean(0) + 0.3 * rng.standard_normal(6), sigma, q, dt, lw, s, seed=9, key=1, link=0, ess_frac=0.6)
        x, lw = r["x_out"], r["lw"]
        hist.append(x), lwh.append(lw), pred.append(x_in), ancs.append(r["anc"]), dts.append(dt)
    assert sum(int((a != np.arange(N)).any()) for a in ancs) >= 2    # (some steps resampled)
    res = SR.smooth(np.array(hist), np.array(lwh), np.array(pred), q, np.array(dts), 64, seed=2, key=1, link=0)
    for m in range(64):
        k = res["idx"][S - 1, m]
        for s in range(S - 1, 0, -1):
            k = ancs[s][k]
            # (the copies a resampling made of one particle are the same candidate in all but the slot number: compare the states)
            assert np.array_equal(res["paths"][s - 1, m], hist[s - 1][k]), (m, s)


def test_a_single_step_is_a_draw_from_the_final_weights():
    rng = np.random.default_rng(5)
    N, M = 6, 4000
    lwh = rng.standard_normal((1, N))
    lwh[0, 4] = -np.inf
    hist = rng.random((1, N, 6))
    r = SR.smooth(hist, lwh, np.full((1, N, 6), np.nan), np.full(6, 0.1), np.ones(1), M, seed=7)
    w = np.exp(lwh[0]) / np.exp(lwh[0]).sum()
    freq = np.bincount(r["idx"][0], minlength=N) / M
    assert freq[4] == 0 and np.abs(freq - w).max() < 4 * math.sqrt(0.25 / M)
    c = np.cumsum(np.exp(lwh[0] - lwh[0].max()))                    # and draw by draw: the inverse of the running sum at u
    from _nuts_reference import hmc_rng, u01
    for m in range(20):
        assert r["idx"][0, m] == np.searchsorted(c, u01(hmc_rng(7, 0, 0, SR.SMOOTH, m)[0]) * c[-1])


def test_a_constant_added_to_a_steps_log_weights_changes_nothing():
    rng = np.random.default_rng(6)
    hist, lwh, pred, q, dt = _filter(rng, N=33, S=5)
    a = SR.smooth(hist, lwh, pred, q, dt, 40, seed=3, key=5)
    b = SR.smooth(hist, lwh + np.array([8.0, -3.0, 0.5, 100.0, -40.0])[:, None], pred, q, dt, 40, seed=3, key=5)
    assert a["tie"] > 1e-9 and np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["paths"], b["paths"])


def test_a_trajectory_depends_on_its_own_number_only():
    rng = np.random.default_rng(7)
    hist, lwh, pred, q, dt = _filter(rng, N=20, S=3)
    a, b = SR.smooth(hist, lwh, pred, q, dt, 3, seed=3, key=5), SR.smooth(hist, lwh, pred, q, dt, 9, seed=3, key=5)
    assert np.array_equal(a["idx"], b["idx"][:, :3]) and not np.array_equal(b["idx"][:, :3], b["idx"][:, 3:6])


# ------------------------------------------------------------------ the method against a Rauch-Tung-Striebel smoother
def _rts(A, x0, q0, q, dts, ys, sigma):
    """The smoothed means [S, 6] of x_0 ~ N(x0, diag(q0^2)), x_s = A x_{s-1} + N(0, diag(q^2 dt_s)), y_s = x_s + N(0, diag(sigma^2))
    on the finite entries of y_s: a Kalman filter forward, the Rauch-Tung-Striebel recursion backward."""
    S = len(ys)
    mp, Pp, mf, Pf = [], [], [], []
    m, P = x0.copy(), np.diag(q0 ** 2)
    for s, y in enumerate(ys):
        if s > 0:
            m, P = A @ m, A @ P @ A.T + np.diag(q ** 2 * dts[s])
        mp.append(m), Pp.append(P)
        on = np.isfinite(y)
        if on.any():
            H = np.eye(6)[on]
            K = P @ H.T @ np.linalg.inv(H @ P @ H.T + np.diag(sigma[on] ** 2))
            m, P = m + K @ (y[on] - H @ m), (np.eye(6) - K @ H) @ P
        mf.append(m), Pf.append(P)
    ms = [None] * S
    ms[S - 1] = mf[S - 1]
    for s in range(S - 2, -1, -1):
        G = Pf[s] @ A.T @ np.linalg.inv(Pp[s + 1])
        ms[s] = mf[s] + G @ (ms[s + 1] - mp[s + 1])
    return np.array(ms)


def _ffbs_means(transition, R, N, M):
    rng = np.random.default_rng(21)
    A = np.eye(6) * 0.9 + 0.05 * rng.standard_normal((6, 6))
    x0 = rng.standard_normal(6)
    q0, q, sigma = np.full(6, 0.5), np.array([0.3, 0.2, 0.15, 0.25, 0.3, 0.1]), np.full(6, 0.7)
    S = 9
    dts = np.concatenate([[1.0], 0.5 + rng.random(S - 1)])
    xt = x0 + q0 * rng.standard_normal(6)
    ys = []
    for s in range(S):
        if s > 0:
            xt = A @ xt + q * math.sqrt(dts[s]) * rng.standard_normal(6)
        y = xt + sigma * rng.standard_normal(6)
        y[rng.random(6) < 0.3] = np.nan
        ys.append(y)
    want = _rts(A, x0, q0, q, dts, ys, sigma)
    means = []
    for seed in range(R):
        x, lw = np.tile(x0, (N, 1)), np.zeros(N)
        hist, lwh, pred = [], [], []
        for s in range(S):
            x_in = x if s == 0 else x @ A.T
            r = FR.step(x_in, ys[s], sigma, q0 if s == 0 else q, dts[s], lw, s, seed=seed, key=0, link=0, ess_frac=0.5)
            x, lw = r["x_out"], r["lw"]
            hist.append(x), lwh.append(lw), pred.append(x_in)
        res = SR.smooth(np.array(hist), np.array(lwh), np.array(pred), q, dts, M, seed=seed, key=0, link=0, transition=transition)
        assert (res["idx"] >= 0).all()
        means.append(res["paths"].mean(1))
    means = np.array(means)                                          # [R, S, 6]
    return (means.mean(0) - want) / (means.std(0, ddof=1) / math.sqrt(R))


R_SEEDS, N_PART, M_TRAJ = 24, 128, 64


def test_backward_simulation_reproduces_the_rts_smoother():
    """A 6-state linear-Gaussian model, additive link, step 0 + 8 steps, about a third of the observations missing; the filter is
    the step restatement with a matrix product as the solve, N = 128, resampling at ESS < N / 2, M = 64 trajectories, 24 seeds.
    The mean of the backward-simulated means over the seeds lies within 4 standard errors (from the same 24 values) of the
    Rauch-Tung-Striebel mean at every step and state.
    Observed z-scores (54 values): largest |z| = 2.66, root mean square 1.23.
    Control, verified once (test_the_control_without_the_transition_term_fails below keeps it verified): with the transition
    term dropped from l the same comparison gives a largest |z| of 19.5 and fails."""
    z = _ffbs_means(True, R_SEEDS, N_PART, M_TRAJ)
    print(f"FFBS against RTS: max |z| {np.abs(z).max():.2f}, rms {math.sqrt((z * z).mean()):.2f}")
    assert np.abs(z).max() < 4.0


def test_the_control_without_the_transition_term_fails():
    """Without the transition term every step is a fresh draw from the FILTER weights: the early steps then miss the smoothed
    mean by many standard errors, so the comparison above has the power to see a wrong density."""
    z = _ffbs_means(False, R_SEEDS, N_PART, M_TRAJ)
    print(f"control without the transition term: max |z| {np.abs(z).max():.2f}")
    assert np.abs(z[:-1]).max() > 4.0 and np.abs(z[-1]).max() < 4.0  # (the last step never had a transition term)


# ------------------------------------------------------------------ the GPU file's inputs have no near-tie
@pytest.mark.parametrize("idx", range(len(SC.CASES)), ids=[SC.case_id(c) for c in SC.CASES])
def test_gpu_cases_have_no_pointer_near_a_boundary(idx):
    """tests/test_smooth_gpu.py asks for exactly equal indices; that needs every pointer u c_{N-1} further from every boundary
    c_k than the kernel and the restatement can differ (the bound is derived there).  Every case keeps 100 times that bound."""
    c = SC.CASES[idx]
    for b, r in enumerate(SC.reference(idx)):
        bound = SR.tie_bound(c["N"], r["spread"], r["logamp"])
        assert r["tie"] >= 100 * bound, (b, r["tie"], bound)
