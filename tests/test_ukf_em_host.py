"""Host-side tests of the EM noise fit over the unscented smoother: the C ABI's surface and argument
validation (no launch, no GPU), the argument errors of inference.fit_ukf_noise, and the properties of the numpy restatement
tests/_ukf_em_reference.py that tests/test_ukf_em_gpu.py holds the kernels to -- above all that with the identity link its
statistic IS the exact Kalman-smoother expectation on linear-Gaussian models, and that its iterations raise their exact evidence."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hode

import _ukf_cases as UC
import _ukf_em_cases as EC
import _ukf_em_reference as ER
import _ukf_reference as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda v: np.ascontiguousarray(v).view(np.uint8)                                 # noqa: E731  (NaN and -0 included)
SYMBOLS = ["hode_ukf_em_points_f32", "hode_ukf_em_points_f64", "hode_ukf_em_stats_f32", "hode_ukf_em_stats_f64", "hode_ukf_em_mstep"]


# ------------------------------------------------------------------ surface
def test_extension_header_declares_and_capi_binds_the_em_entries():
    """include/hode_ukf_em.h against its table (hode/_abi.py EXTENSIONS), prototype by prototype, with the parser that holds the
    main table to include/hode.h; and the declarations load() leaves on the library."""
    from hode import _abi
    from test_capi_abi_host import parse_header
    hdr = open(os.path.join(ROOT, "include", "hode_ukf_em.h")).read()
    declared = parse_header(hdr)
    assert list(declared) == SYMBOLS == hode.capi.EXT_SYMBOLS["hode_ukf_em.h"]
    assert set(declared) == set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr)) and '#include "hode.h"' in hdr
    table = {sym: (ret, words) for sym, _, _, ret, words in _abi.expand(_abi.EXTENSIONS["hode_ukf_em.h"])}
    assert table == declared
    lib = hode.load()
    for sym, (ret, words) in declared.items():
        fn = getattr(lib, sym)
        assert fn.restype is _abi.RETURNS[ret] and len(fn.argtypes) == len(words), sym
        for at, w in zip(fn.argtypes, words):
            assert (at is _abi.SCALARS[w]) if w in _abi.SCALARS else (isinstance(at, _abi.Pointer) and at.word == w), (sym, w)
        assert sym not in hode.capi.SYMBOLS                                 # (hode.h and its table are as they were)
    assert len(hode.capi.SYMBOLS) == 79 and list(hode.capi.EXT_SYMBOLS) == ["hode_ukf_smooth.h", "hode_ukf_em.h"]
    assert all(callable(getattr(hode.capi, f)) for f in ("ukf_em_points", "ukf_em_stats", "ukf_em_mstep"))
    for name, value in (("HODE_UKF_EM_SUMS", hode.capi.UKF_EM_SUMS), ("HODE_UKF_EM_FIT", hode.capi.UKF_EM_FIT), ("HODE_UKF_EM_SLOTS", ER.SLOTS)):
        assert re.search(rf"#define {name} (\d+)", hdr).group(1) == str(value), name
    assert (ER.SUMS, ER.FIT) == (hode.capi.UKF_EM_SUMS, hode.capi.UKF_EM_FIT)
    at = hode.capi.UKF_EM_SUM_AT
    assert (at["A"].start, at["N"], at["D"], at["R"].start, at["M"].start) == (ER.AT_A, ER.AT_N, ER.AT_D, ER.AT_R, ER.AT_M)


def test_inference_exports_the_fit():
    import inference
    from inference.ukf import UKFNoiseFit, UKFSmoothResult, fit_ukf_noise
    assert "fit_ukf_noise" in inference.__all__ and inference.fit_ukf_noise is fit_ukf_noise and inference.UKFNoiseFit is UKFNoiseFit
    assert callable(UKFSmoothResult.noise_statistics)


# ------------------------------------------------------------------ every HODE_EINVAL, by return code
ARGS = {"points": (["mean_s", "cov_s", "alive", "ode_history"], ["x_em", "aux_em", "chol"]),
        "stats": (["prop_em", "status", "chol", "mean_s", "cov_s", "gain", "alive", "obs", "mask", "moments"], ["e2", "pair_ok", "r2", "seen"]),
        "mstep": (["e2", "pair_ok", "r2", "seen", "dt"], ["q", "walk", "sigma", "sums"])}
PAIR_ONLY = {"points": ["x_em", "aux_em", "chol"], "stats": ["prop_em", "status", "chol", "gain", "e2", "pair_ok"], "mstep": ["e2", "pair_ok"]}
EINVAL = -1


def _call(entry, sfx="f32", S=3, B=1, link=1, mode=(0,) * 17, w=(2.6, 0.1, 0.1, 0.07), null=(), alias=(), fit=(1,) * 29, floor=(1e-6,) * 29):
    """hode_ukf_em_<entry> with dummy non-null device pointers (never dereferenced: every case here returns before a launch); the
    host arrays are real."""
    ins, outs = ARGS[entry]
    p = {n: C.c_void_p(16 * (k + 1)) for k, n in enumerate(ins + outs)}
    for n in null:
        p[n] = C.c_void_p(0)
    for dst, src in alias:
        p[dst] = p[src]
    md = C.c_void_p(0) if mode is None else (C.c_int32 * 17)(*mode)
    head = [C.c_void_p(0), C.c_int(S), C.c_int(B), C.c_int(link), md]
    lib = hode.load()
    if entry == "points":
        return getattr(lib, f"hode_ukf_em_points_{sfx}")(*head, C.c_double(w[0]), *(p[n] for n in ins + outs))
    if entry == "stats":
        return getattr(lib, f"hode_ukf_em_stats_{sfx}")(*head, *(C.c_double(v) for v in w), *(p[n] for n in ins + outs))
    fm = C.c_void_p(0) if fit is None else (C.c_int32 * 29)(*fit)
    fl = C.c_void_p(0) if floor is None else (C.c_double * 29)(*floor)
    return lib.hode_ukf_em_mstep(*head, fm, fl, *(p[n] for n in ins + outs))


@pytest.mark.parametrize("entry,sfx", [("points", "f32"), ("points", "f64"), ("stats", "f32"), ("stats", "f64"), ("mstep", "")])
def test_argument_validation_without_gpu(entry, sfx):
    """Every HODE_EINVAL case of the header returns before a launch."""
    ins, outs = ARGS[entry]
    assert _call(entry, sfx, S=0) == EINVAL and _call(entry, sfx, S=-1) == EINVAL and _call(entry, sfx, B=0) == EINVAL
    assert _call(entry, sfx, link=2) == EINVAL and _call(entry, sfx, link=-1) == EINVAL
    for bad in (3, -1):
        for at in (0, 16):
            mode = [0] * 17
            mode[at] = bad
            assert _call(entry, sfx, mode=mode) == EINVAL, (bad, at)
    assert _call(entry, sfx, mode=None) == EINVAL
    if entry != "mstep":
        for gamma in (0.0, -1.0, math.nan, math.inf):
            assert _call(entry, sfx, w=(gamma, 0.1, 0.1, 0.07)) == EINVAL, gamma
    if entry == "stats":
        for k in (1, 2, 3):
            w = [2.6, 0.1, 0.1, 0.07]
            w[k] = math.nan
            assert _call(entry, sfx, w=w) == EINVAL, k
    for name in ins + outs:
        if name != "mask":                                              # (mask may always be NULL)
            assert _call(entry, sfx, null=(name,)) == EINVAL, name
    for name in ins + outs:                                             # with one step there are no pairs: the rest is still needed
        if name not in PAIR_ONLY[entry] and name != "mask":
            assert _call(entry, sfx, S=1, null=(name,)) == EINVAL, name
    for out in outs:
        for src in ins:
            assert _call(entry, sfx, alias=((out, src),)) == EINVAL, (out, src)
    assert _call(entry, sfx, alias=((outs[1], outs[0]),)) == EINVAL and _call(entry, sfx, alias=((outs[-1], outs[0]),)) == EINVAL
    if entry == "mstep":
        assert _call(entry, fit=None) == EINVAL and _call(entry, floor=None) == EINVAL
        for bad in (2, -1):
            assert _call(entry, fit=[1] * 28 + [bad]) == EINVAL and _call(entry, fit=[bad] + [1] * 28) == EINVAL
        for bad in (-1e-9, math.nan, math.inf):
            assert _call(entry, floor=[1e-6] * 28 + [bad]) == EINVAL and _call(entry, floor=[bad] + [1e-6] * 28) == EINVAL, bad
    if entry == "points":                                               # one step: nothing to do, and nothing is launched
        assert _call(entry, sfx, S=1, null=("x_em", "aux_em", "chol")) == 0


def test_fit_ukf_noise_refuses_bad_arguments_before_a_device_is_touched():
    """(no model, no data: every check here stands in front of them)"""
    from inference import ParameterLearning, fit_ukf_noise
    from inference.observation import ObservationModel
    for kw, match in ((dict(n_iter=0), "n_iter"), (dict(n_iter=-3), "n_iter"), (dict(fit=()), "selects nothing"),
                      (dict(fit={"process_noise": [False] * 6, "noise_sigma": False}), "selects nothing"),
                      (dict(fit=("process_noise", "initial_spread")), "initial_spread"), (dict(fit=("walk",)), "learn"),
                      (dict(fit={"noise_sigma": [True] * 5}), "one flag or 6"), (dict(tol=-1.0), "tol"), (dict(tol=math.nan), "tol"),
                      (dict(floor=-1.0), "floor"), (dict(floor=[1e-6] * 6), "floor"), (dict(learn="k_I"), "ParameterLearning"),
                      (dict(noise_sigma=ObservationModel(1.0, noise="marginal")), "marginal"), (dict(noise_link="sqrt"), "noise_link"),
                      (dict(process_noise=-0.1), "process_noise")):
        with pytest.raises(ValueError, match=match):
            fit_ukf_noise(None, None, **kw)
    learn = ParameterLearning(["k_I", "a_GI"], walk=[0.1, 0.0], initial_spread=0.2)
    with pytest.raises(ValueError, match="one flag or 2"):
        fit_ukf_noise(None, None, learn=learn, fit={"walk": [True] * 3})
    from inference.ukf import _fit_mask
    m = _fit_mask({"walk": [False, True], "noise_sigma": True}, learn)
    assert m[:6].sum() == 0 and m[23:].sum() == 6 and m[6:23].sum() == 1 and m[6 + learn.columns[1]] == 1
    assert _fit_mask("process_noise", None).tolist() == [1] * 6 + [0] * 23


# ------------------------------------------------------------------ the restatement on linear-Gaussian models
@pytest.fixture(scope="module", params=[1, 2])
def linear(request):
    M = UC.linear_model(request.param)
    return request.param, M, EC.estep_linear(M, [M["ys"]])


def test_on_a_linear_model_the_statistic_is_the_exact_smoother_expectation(linear):
    """e2 against the diagonal of Ps_{s+1} - F G Ps_{s+1} - (.)^T + F Ps_s F^T + d d^T and r2 against (y - H ms)^2 + diag(H Ps H^T) of
    the exact Kalman RTS smoother, within 1e-12 of the largest term (DESIGN.md section 4.23's bound).
    Measured: model 1 e2 1.4e-15, r2 7.5e-16; model 2 e2 1.9e-15, r2 5.2e-16 of the largest term."""
    which, M, e = linear
    want_e2, want_r2, scale = EC.exact_statistics(M, M["ys"])
    assert e["pair_ok"].all() and np.isfinite(e["e2"]).all()
    err_e2 = max(np.abs(e["e2"][s, 0] - want_e2[s]).max() / scale[s] for s in range(M["S"] - 1))
    err_r2 = np.abs(e["r2"][:, 0] - want_r2).max() / np.abs(want_r2).max()
    print(f"model {which}: e2 {err_e2:.2e}, r2 {err_r2:.2e} of the largest term")
    assert err_e2 <= 1e-12 and err_r2 <= 1e-12
    seen = np.array([[(int(e["seen"][s, 0]) >> j) & 1 for j in range(6)] for s in range(M["S"])], dtype=bool)
    assert np.array_equal(seen, np.isfinite(M["ys"])) and not e["r2"][:, 0][~seen].any()
    assert e["seen"][4, 0] == 0                                          # (the step that observes nothing)


def test_an_exact_coordinate_keeps_its_zero_and_passes_nothing():
    """Model 2: state 3 has no process noise -- its q stays exactly 0 whatever the statistic says -- and state 1 is known exactly
    at the first step: its column of the factor is a zero column, and its row of V is exactly zero."""
    M = UC.linear_model(2)
    e = EC.estep_linear(M, [M["ys"]])
    assert M["q"][3] == 0.0 and M["P0"][1, 1] == 0.0
    assert not e["V"][0, 0, 1, :].any() and e["V"][0, 0, 0, :].any() and e["V"][1, 0, 1, :].any()
    sums = ER.reduce(e["e2"], e["pair_ok"], e["r2"], e["seen"], e["dt"])
    q, walk, sigma = ER.mstep(sums, M["q"], M["walk"], M["sigma"], M["mode"], np.ones(ER.FIT, dtype=np.int32), np.full(ER.FIT, 1e-6), link=0)
    assert q[3] == 0.0 and sums[ER.AT_A + 3] != 0.0 and (q[[0, 1, 2, 4, 5]] != M["q"][[0, 1, 2, 4, 5]]).all()
    cols = M["cols"]
    assert walk[cols[0]] == 0.0 and walk[cols[1]] != M["walk"][cols[1]] and walk[cols[1]] > 0       # (a walk of 0 stays, the other is fitted)
    carried = [c for c in range(17) if c not in cols]
    assert np.array_equal(bits(walk[carried]), bits(M["walk"][carried]))


def test_em_iterations_raise_the_exact_evidence():
    """Eight iterations on records simulated from model 1 (B = 6, S = 40), started a factor of 3 and of 1/2 off: the exact Kalman
    evidence at each iteration's values never falls (slack 1e-9 |l| for rounding).  The identity link: the drift-free M-step."""
    M0 = UC.linear_model(1)
    M, ys = EC.simulate(M0, S=40, B=6, seed=77)
    start = dict(M, q=3.0 * M["q"], sigma=0.5 * M["sigma"])
    fit_mask = np.array([1] * 6 + [0] * 17 + [1] * 6, dtype=np.int32)
    models, sums = EC.em_linear(start, ys, 8, fit_mask)
    ev = [EC.evidence(m, ys) for m in models]
    print("evidence:", " ".join(f"{v:.4f}" for v in ev))
    print("q:", models[-1]["q"], "sigma:", models[-1]["sigma"], "(generating", M["q"], M["sigma"], ")")
    assert len(ev) == 9 and all(sums[i][ER.AT_N] == 6 * 39 for i in range(8))
    for a, b in zip(ev, ev[1:]):
        assert b >= a - 1e-9 * abs(a), (a, b)
    assert ev[-1] > ev[0] + 10.0
    assert np.abs(np.log(models[-1]["sigma"] / M["sigma"])).max() < np.abs(np.log(start["sigma"] / M["sigma"])).max()


def test_the_log_link_closed_form_is_a_stationary_maximum():
    for A, N, D in ((0.5, 234.0, 190.0), (3e-3, 36.0, 41.5), (40.0, 8.0, 2.5), (1e-9, 1000.0, 980.0)):
        obj = lambda v: -(N / 2) * math.log(v) - A / (2 * v) - v * D / 8                 # noqa: E731
        v = ER.log_link_variance(A, N, D)
        assert v > 0 and obj(v) > obj(1.01 * v) and obj(v) > obj(0.99 * v), (A, N, D)
        assert abs(-(N / 2) / v + A / (2 * v * v) - D / 8) <= 1e-9 * (N / 2) / v          # (the derivative vanishes)
        # the form with the difference is the same number, up to the digits sqrt(N^2 + A D) - N cancels: 2^-52 N^2 / (A D) of it
        assert math.isclose(v, 2 * (math.sqrt(N * N + A * D) - N) / D, rel_tol=8 * 2.0 ** -52 * (1 + N * N / (A * D)))
        assert v < A / N                                                                  # (the drift takes some of the residual)


def test_what_leaves_every_value_as_it_is():
    """S = 1 (no pairs), a state nobody observes, and a fit_mask of zeros: bit for bit."""
    ones, floor = np.ones(ER.FIT, dtype=np.int32), np.full(ER.FIT, 1e-6)
    c = EC.case(8)
    assert c["S"] == 1 and c["e2"].shape == (0, 3, 8) and c["sums"][ER.AT_N] == 0 and c["sums"][ER.AT_M:].sum() > 0
    q, walk, sigma = ER.mstep(c["sums"], c["q"], c["walk"], c["sigma"], c["mode"], ones, floor, c["link"])
    assert np.array_equal(bits(q), bits(c["q"])) and np.array_equal(bits(walk), bits(c["walk"])) and not np.array_equal(sigma, c["sigma"])
    c = EC.case(2)
    r2, seen = c["r2"].copy(), c["seen"] & ~(1 << 3)                        # state 3 is missing throughout
    r2[:, :, 3] = 0.0
    sums = ER.reduce(c["e2"], c["pair_ok"], r2, seen, c["dt"])
    assert sums[ER.AT_M + 3] == 0 and sums[ER.AT_R + 3] == 0
    q, walk, sigma = ER.mstep(sums, c["q"], c["walk"], c["sigma"], c["mode"], ones, floor, c["link"])
    assert sigma[3] == c["sigma"][3] and (sigma[[0, 1, 2, 4, 5]] != c["sigma"][[0, 1, 2, 4, 5]]).all()
    got = ER.mstep(c["sums"], c["q"], c["walk"], c["sigma"], c["mode"], np.zeros(ER.FIT, dtype=np.int32), floor, c["link"])
    for a, b in zip(got, (c["q"], c["walk"], c["sigma"])):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ the cases of the GPU test
@pytest.mark.parametrize("idx", range(len(EC.SPECS)), ids=[EC.case_id(s) for s in EC.SPECS])
def test_the_gpu_cases_are_well_conditioned_and_show_what_they_are_for(idx):
    spec, c = EC.SPECS[idx], EC.case(idx)
    S, B, n, K = c["S"], c["B"], c["n"], c["K"]
    live = c["alive"][1:] == 1
    if S > 1:
        assert np.nanmax(c["cond"]) <= UC.COND_CAP and np.isfinite(c["cond"][live]).all(), np.nanmax(c["cond"])
    want_ok = live.copy()
    if idx == EC.STATUS_CASE:
        want_ok[EC.STATUS_PAIR, EC.STATUS_PATIENT] = False
        assert c["alive"][EC.STATUS_PAIR + 1, EC.STATUS_PATIENT] == 1
    assert np.array_equal(c["pair_ok"] == 1, want_ok) and np.array_equal(np.isnan(c["e2"]).all(2), ~want_ok)
    assert np.isfinite(c["e2"][want_ok]).all() and c["sums"][ER.AT_N] == want_ok.sum()
    if spec.get("edge") == "lost":
        assert c["pair_ok"][:, 1].tolist() == [1, 0, 0] and (c["x_em"][1:, K:2 * K] == 1.0).all() and np.isnan(c["chol"][1:, 1]).all()
        assert (c["seen"][2:, 1] == 0).all() and not c["r2"][2:, 1].any()
    if spec.get("edge") == "zero_state":                                 # the exact coordinate: a zero column, a zero residual
        assert not c["chol"][:, :, 2, :].any() and not c["chol"][:, :, :, 2].any() and not c["e2"][:, :, 2].any()
        assert c["q"][2] == 0.0 and c["new_q"][2] == 0.0
    if S > 1:
        assert (c["seen"][S - 2, 0] == 0) and not c["r2"][S - 2, 0].any()                                # the step that sees nothing
        assert (c["e2"][want_ok][:, [j for j in range(n) if j != 2]] > 0).all()
    if c["mask"] is not None:
        assert (c["seen"][1, c["alive"][1] == 1] <= 1).all() and (c["seen"][1] == 1).any()               # one state seen
    # the update: a value left out, a value at zero and the carried columns keep their bits; a floor holds
    assert c["new_q"][1] == c["q"][1] and c["new_sigma"][4] == c["sigma"][4] and c["new_q"][2] == 0.0
    cols, _ = UR.columns(c["mode"])
    carried = [k for k in range(17) if k not in cols]
    assert np.array_equal(bits(c["new_walk"][carried]), bits(c["walk"][carried]))
    if S > 1:
        assert c["new_q"][0] == 10.0 and (c["new_q"][[3, 4, 5]] != c["q"][[3, 4, 5]]).all() and (c["new_walk"][cols] != c["walk"][cols]).all()
    assert (c["new_sigma"][[0, 1, 2, 3, 5]] != c["sigma"][[0, 1, 2, 3, 5]]).all()
