"""Host-side tests of the unscented RTS smoother: the C ABI's surface and argument validation (no launch,
no GPU), and the properties of the numpy restatement tests/_ukf_smooth_reference.py that tests/test_ukf_smooth_gpu.py holds the
kernels to -- above all that with the identity link it IS the Kalman RTS smoother on linear-Gaussian models."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hode

import _ukf_cases as UC
import _ukf_reference as UR
import _ukf_smooth_cases as SC
import _ukf_smooth_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda v: np.ascontiguousarray(v).view(np.uint8)                                 # noqa: E731  (NaN and -0 included)


# ------------------------------------------------------------------ surface
def test_extension_header_declares_and_capi_binds_the_smoother():
    """include/hode_ukf_smooth.h against its table (hode/_abi.py EXTENSIONS), prototype by prototype, with the parser that holds
    the main table to include/hode.h; and the declarations load() leaves on the library."""
    from hode import _abi
    from test_capi_abi_host import parse_header
    hdr = open(os.path.join(ROOT, "include", "hode_ukf_smooth.h")).read()
    declared = parse_header(hdr)
    assert list(declared) == ["hode_ukf_smooth_f32", "hode_ukf_smooth_f64"] == hode.capi.EXT_SYMBOLS["hode_ukf_smooth.h"]
    assert set(declared) == set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr)) and '#include "hode.h"' in hdr
    table = {sym: (ret, words) for sym, _, _, ret, words in _abi.expand(_abi.EXTENSIONS["hode_ukf_smooth.h"])}
    assert table == declared
    lib = hode.load()
    for sym, (ret, words) in declared.items():
        fn = getattr(lib, sym)
        assert fn.restype is _abi.RETURNS[ret] and len(fn.argtypes) == len(words), sym
        for at, w in zip(fn.argtypes, words):
            assert (at is _abi.SCALARS[w]) if w in _abi.SCALARS else (isinstance(at, _abi.Pointer) and at.word == w), (sym, w)
        assert sym not in hode.capi.SYMBOLS                                 # (hode.h and its table are as they were)
    assert "Unscented RTS smoother" in hdr and callable(hode.capi.ukf_smooth)


def test_inference_exports_the_smooth_result():
    import inference
    from inference.ukf import UKFResult, UKFSmoothResult
    assert "UKFSmoothResult" in inference.__all__ and inference.UKFSmoothResult is UKFSmoothResult and callable(UKFResult.smooth)
    for name in ("propagated_history", "dt_history"):
        assert name in UKFResult.__doc__, name


INPUTS = ["history", "ode_history", "propagated", "mean_f", "cov_f", "alive", "q", "walk", "dt"]
OUTPUTS = ["mean_s", "cov_s", "gain", "pred_mean", "pred_cov", "moments"]


def _call(sfx="f32", S=3, B=1, link=1, mode=(0,) * 17, w=(2.6, 0.1, 0.1, 0.07), null=(), alias=()):
    """hode_ukf_smooth_* with dummy non-null device pointers (never dereferenced: every case here returns before a launch); mode is
    the one host array, and real."""
    p = {n: C.c_void_p(16 * (k + 1)) for k, n in enumerate(INPUTS + OUTPUTS)}
    for n in null:
        p[n] = C.c_void_p(0)
    for dst, src in alias:
        p[dst] = p[src]
    md = C.c_void_p(0) if mode is None else (C.c_int32 * 17)(*mode)
    f = getattr(hode.load(), f"hode_ukf_smooth_{sfx}")
    return f(C.c_void_p(0), C.c_int(S), C.c_int(B), C.c_int(link), md, *(C.c_double(v) for v in w), *(p[n] for n in INPUTS + OUTPUTS))


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_argument_validation_without_gpu(sfx):
    """Every HODE_EINVAL case of the header returns before a launch."""
    EINVAL = -1
    assert _call(sfx, S=0) == EINVAL and _call(sfx, S=-1) == EINVAL and _call(sfx, B=0) == EINVAL and _call(sfx, B=-2) == EINVAL
    assert _call(sfx, link=2) == EINVAL and _call(sfx, link=-1) == EINVAL
    for bad in (3, -1):
        for at in (0, 16):
            mode = [0] * 17
            mode[at] = bad
            assert _call(sfx, mode=mode) == EINVAL, (bad, at)
    assert _call(sfx, mode=None) == EINVAL
    for gamma in (0.0, -1.0, math.nan, math.inf):
        assert _call(sfx, w=(gamma, 0.1, 0.1, 0.07)) == EINVAL, gamma
    for k in (1, 2, 3):
        w = [2.6, 0.1, 0.1, 0.07]
        w[k] = math.nan
        assert _call(sfx, w=w) == EINVAL, k
    for name in INPUTS + OUTPUTS:
        assert _call(sfx, null=(name,)) == EINVAL, name
    for name in ("mean_s", "cov_s", "moments"):                         # (with one step there are no pairs: only these are written)
        assert _call(sfx, S=1, null=(name,)) == EINVAL, name
    for out in OUTPUTS:
        for src in INPUTS:
            assert _call(sfx, alias=((out, src),)) == EINVAL, (out, src)
    assert _call(sfx, alias=(("gain", "pred_cov"),)) == EINVAL and _call(sfx, alias=(("cov_s", "mean_s"),)) == EINVAL


def test_smooth_needs_a_stored_run():
    """(the checks stand in front of everything that touches a device)"""
    from inference.ukf import UKFResult
    res = UKFResult.__new__(UKFResult)
    res._forecast, res.history = False, None
    with pytest.raises(ValueError, match="store_history"):
        res.smooth()
    res._forecast, res.history = True, object()
    with pytest.raises(ValueError, match="forecast"):
        res.smooth()


# ------------------------------------------------------------------ the restatement on linear-Gaussian models
@pytest.fixture(scope="module", params=[1, 2])
def linear(request):
    M = UC.linear_model(request.param)
    c = SC.filter_linear_model(M)
    return M, c, SC.smooth_patient(c, 0)


def test_on_a_linear_model_it_is_the_kalman_rts_smoother(linear):
    M, c, got = linear
    worst_m = worst_P = 0.0
    for s, (m, P) in enumerate(SC.kalman_rts(M)):
        worst_m, worst_P = max(worst_m, np.abs(got["mean_s"][s] - m).max()), max(worst_P, np.abs(got["cov_s"][s] - P).max())
    print(f"smoothed mean {worst_m:.2e}, covariance {worst_P:.2e} from the exact smoother; largest cond(P-) {np.nanmax(got['cond']):.3g}")
    assert worst_m <= 1e-12 and worst_P <= 1e-12
    assert np.nanmax(got["cond"]) <= UC.COND_CAP


def test_smoothing_never_widens_a_covariance(linear):
    _, c, got = linear
    low = min(np.linalg.eigvalsh(c["cov_f"][s, 0] - got["cov_s"][s]).min() for s in range(c["S"]))
    print(f"smallest eigenvalue of P_s - Ps_s: {low:.2e}")
    assert low >= -1e-12


def test_the_terminal_step_is_a_copy_and_the_predicted_moments_are_the_filters(linear):
    M, c, got = linear
    S = c["S"]
    assert np.array_equal(bits(got["mean_s"][S - 1]), bits(c["mean_f"][S - 1, 0]))
    assert np.array_equal(bits(got["cov_s"][S - 1]), bits(c["cov_f"][S - 1, 0]))
    assert got["terminal"] == S - 1
    # the same inputs in the same order: m-, P- of a pair are what the filter's step s + 1 started its update from
    w = UR.weights(M["n"])
    for s in range(1, S):
        r = UR.step(c["prop"][s, 0], c["ode"][s - 1, 0], M["mode"], M["ys"][s], M["sigma"], M["q"], M["walk"], M["dts"][s], 1, None, None, w,
                    predict=True, link=0)
        assert np.array_equal(bits(r["m_pred"]), bits(got["pred_mean"][s - 1])), s
        assert np.array_equal(bits(r["P_pred"]), bits(got["pred_cov"][s - 1])), s
    # and the natural-space moments of the terminal step are the step's statistics
    assert np.array_equal(bits(got["moments"][S - 1]), bits(r["stats"][4:16]))


@pytest.mark.parametrize("which", [1, 2])
def test_nothing_observed_at_the_end_smoothed_is_filtered(which):
    """Trailing all-NaN rows: from the last observed step on D and delta are exactly zero."""
    M = UC.linear_model(which)
    ys = M["ys"].copy()
    last = M["S"] - 4
    ys[last + 1:] = np.nan
    c = SC.filter_linear_model(M, ys=ys)
    got = SC.smooth_patient(c, 0)
    for s in range(last, M["S"]):
        assert np.array_equal(bits(got["mean_s"][s]), bits(c["mean_f"][s, 0])), s
        assert np.array_equal(bits(got["cov_s"][s]), bits(c["cov_f"][s, 0])), s
    assert not np.array_equal(got["mean_s"][last - 1], c["mean_f"][last - 1, 0])       # (before it the future does speak)
    want = SC.kalman_rts(M, ys=ys)
    assert max(np.abs(got["mean_s"][s] - want[s][0]).max() for s in range(M["S"])) <= 1e-12


def test_a_coordinate_the_filter_holds_exactly_takes_and_gives_nothing():
    """A hand-made additive-link model: state 2 decoupled in A, without process noise or initial spread, at the value 1 (and
    dyadic weights, n + kappa = 8, so that the mean of equal points is that value exactly)."""
    M = UC.linear_model(1)
    A = M["A"].copy()
    A[2, :], A[:, 2] = 0.0, 0.0
    A[2, 2] = 1.0
    q, P0, m0 = M["q"].copy(), M["P0"].copy(), M["m0"].copy()
    q[2], P0[2, 2], m0[2] = 0.0, 0.0, 1.0
    M = dict(M, A=A, q=q, P0=P0, m0=m0)
    n, K, S = 6, 13, M["S"]
    w = UR.weights(n, kappa=2.0)
    x, aux = np.zeros((K, 6)), np.ones((K, 17))
    mean, cov = m0.copy(), P0.copy()
    hist, prop, ode, mean_f, cov_f = np.zeros((S, K, 6)), np.zeros((S, K, 6)), np.ones((S, K, 17)), np.zeros((S, n)), np.zeros((S, n, n))
    for s in range(S):
        if s > 0:
            x = x @ A.T
        prop[s] = x
        r = UR.step(x, aux, M["mode"], M["ys"][s], M["sigma"], q, M["walk"], M["dts"][s], 1, mean, cov, w, predict=s > 0, link=0)
        assert r["alive"] == 1
        x, mean, cov = r["x_out"], r["mean"], r["cov"]
        hist[s], mean_f[s], cov_f[s] = x, mean, cov
    assert (hist[:, :, 2] == 1.0).all() and (mean_f[:, 2] == 1.0).all()
    got = SR.smooth(hist, ode, prop, mean_f, cov_f, np.ones(S), M["mode"], q, M["walk"], M["dts"], w, link=0)
    assert not got["gain"][:, 2, :].any() and not got["gain"][:, :, 2].any()
    assert not got["cov_s"][:, 2, :].any() and not got["cov_s"][:, :, 2].any()
    assert np.array_equal(bits(got["mean_s"][:, 2]), bits(mean_f[:, 2]))
    assert np.isfinite(got["mean_s"]).all() and np.abs(got["mean_s"] - mean_f)[:-1].max() > 1e-3          # (the rest is smoothed)


def test_a_patient_lost_mid_record_ends_at_its_last_alive_step():
    M5 = dict(UC.linear_model(1), S=5)
    dead, ok = SC.filter_linear_model(M5, dead_at=2), SC.filter_linear_model(M5)
    assert dead["alive"][:, 0].tolist() == [1, 1, 0, 0, 0]
    got = SC.smooth_patient(dead, 0)
    assert got["terminal"] == 1
    for name in ("mean_s", "cov_s", "moments"):
        assert np.isnan(got[name][2:]).all() and np.isfinite(got[name][:2]).all(), name
    for name in ("gain", "pred_mean", "pred_cov"):
        assert np.isnan(got[name][1:]).all() and np.isfinite(got[name][:1]).all(), name
    assert np.array_equal(bits(got["mean_s"][1]), bits(dead["mean_f"][1, 0])) and np.array_equal(bits(got["cov_s"][1]), bits(dead["cov_f"][1, 0]))
    # step 0 is smoothed from step 1 alone: the smoother of the record cut after step 1
    cut = SC.smooth_patient({k: (v[:2] if isinstance(v, np.ndarray) and v.shape[:1] == (5,) else v) for k, v in ok.items()}, 0)
    assert np.array_equal(bits(got["mean_s"][0]), bits(cut["mean_s"][0])) and np.array_equal(bits(got["cov_s"][0]), bits(cut["cov_s"][0]))
    # a batch of the two: the neighbour's bits are those of its own pass
    both = {k: (np.concatenate([dead[k], ok[k]], axis=1) if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[0] == 5 else v)
            for k, v in dead.items()}
    alone, beside = SC.smooth_patient(ok, 0), SC.smooth_patient(both, 1)
    for name in ("mean_s", "cov_s", "gain", "pred_mean", "pred_cov", "moments"):
        assert np.array_equal(bits(alone[name]), bits(beside[name])), name
    never = SR.smooth(dead["hist"][:, 0], dead["ode"][:, 0], dead["prop"][:, 0], dead["mean_f"][:, 0], dead["cov_f"][:, 0], np.zeros(5),
                      dead["mode"], dead["q"], dead["walk"], dead["dt"][:, 0], dead["w"], 0)
    assert never["terminal"] == -1 and all(np.isnan(never[k]).all() for k in ("mean_s", "cov_s", "gain", "pred_mean", "pred_cov", "moments"))


# ------------------------------------------------------------------ the cases of the GPU test
@pytest.mark.parametrize("idx", range(len(SC.SPECS)), ids=[SC.case_id(s) for s in SC.SPECS])
def test_the_gpu_cases_are_well_conditioned_and_show_what_they_are_for(idx):
    spec, c, refs = SC.SPECS[idx], SC.case(idx), SC.reference(idx)
    conds = np.array([r["cond"] for r in refs])
    if c["S"] > 1:
        assert np.nanmax(conds) <= UC.COND_CAP, np.nanmax(conds)
    lost = spec.get("edge") == "lost"
    assert (c["alive"][:, [b for b in range(c["B"]) if not (lost and b == 1)]] == 1).all()
    if lost:
        assert c["alive"][:, 1].tolist() == [1, 1, 0, 0] and refs[1]["terminal"] == 1 and np.isnan(refs[1]["gain"][1:]).all()
    for b, r in enumerate(refs):
        t = r["terminal"]
        assert np.array_equal(bits(r["mean_s"][t]), bits(c["mean_f"][t, b])) and np.isfinite(r["moments"][:t + 1]).all()
        if t > 0:
            assert np.abs(r["mean_s"][:t] - c["mean_f"][:t, b]).max() > 1e-6                                # (the pass does something)
            low = min(np.linalg.eigvalsh(c["cov_f"][s, b] - r["cov_s"][s]).min() for s in range(t))
            assert low >= -1e-12 * np.abs(c["cov_f"][:t + 1, b]).max(), low
    if spec.get("edge") == "zero_state":
        for r in refs:
            assert not r["gain"][:, 2, :].any() and not r["gain"][:, :, 2].any() and not r["cov_s"][:, 2, :].any()
