"""Host-side tests of the tangent-linear solve for generic networks (no GPU): admission of every case of
tests/_jvp_generic_cases.py from the oracle alone, declaration / export / argument validation of hode_solve_jvp_any_*, the build checks
of csrc/hode_generic_jvp.hip (cross-compiles, no scratch in fp32, no DPP hazard; csrc/hode_solve_jvp.hip keeps its eight fp32 kernels),
the oracle's tangent of a tanh 96 x 5 network against finite differences of the oracle's own solve, and the admission of the calibration
case (Levenberg-Marquardt around the oracle)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _input_grad_cases as IC
import _jvp_cases as JC
import _jvp_generic_cases as GC

import hode

ROOT = IC.ROOT
CSRC = os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd", "csrc")
NEW = ["hode_solve_jvp_any_f32", "hode_solve_jvp_any_f64"]
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.build()
    return oracle


# ------------------------------------------------------------------ 1. admission, from the oracle alone
def _admit(O, part, c):
    d = IC.solve_data(c)
    sets = GC.direction_sets(part, c, d)
    ref = {}
    worst = 0.0
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
            # the fp64 oracle at the fp32 cases' solver tolerances: equal statuses and step counts, and the distance of the fp32 oracle
            # from it, per direction, leaves a margin of 8 room under the cap
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
                    worst = max(worst, d_ref / IC.FP32_CAP[c["method"]])
                    assert d_ref <= IC.FP32_CAP[c["method"]] / 8, (label, k, d_ref)
    return worst


@pytest.mark.parametrize("part", GC.PARTS)
def test_every_case_is_admissible(O, part):
    worst = 0.0
    for c in GC.CASES[part]:
        try:
            worst = max(worst, _admit(O, part, c))
        except AssertionError as e:
            raise AssertionError(f"case {part}/{c['name']} (seed {c['seed']}): {e}") from e
    print(f"FIGURE admission part {part}: largest d_ref / cap {worst:.3f}")


def test_the_table_is_generic_and_reuses_the_existing_cases():
    tuned = lambda c: c["H"] <= 64 and c["L"] <= 4 and c["act"] == IC.RELU         # noqa: E731
    assert not any(tuned(c) for p in GC.PARTS for c in GC.CASES[p])
    assert [c["name"] for c in GC.CASES["g"]] == [c["name"] for c in IC.SOLVE["b"]] and len(GC.CASES["g"]) == 12
    assert {(c["H"], c["L"], c["act"]) for c in GC.CASES["g"]} == set(IC.GENERIC_SHAPES)
    assert {c["act"] for c in GC.CASES["g"]} == {IC.RELU, IC.TANH, IC.ELU, IC.LEAKY}
    assert [c["name"] for c in GC.CASES["c"]] == [f"g100x3-{n}" for n in JC._C_NAMES]
    assert [c["name"] for c in GC.CASES["k"]] == ["g100x3-tbatched", "g100x3-sets3x3"]
    assert GC.CASES["e"][0]["name"] == "g100x3-budget6" and GC.CASES["e"][0]["dtypes"] == ("f64",)
    assert all(m >= 8.0 for m in GC.MARGIN.values()) and all(r < GC.MARGIN[p] for p, r in GC.MEASURED.items())


# ------------------------------------------------------------------ 2. the entry points
def test_jvp_any_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hode.h")).read()
    declared = set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(hode.lib_path())
    for name in NEW:
        assert name in declared and name in hode.capi.SYMBOLS and hasattr(lib, name), name


def _call(sfx, K=2, v_ode=True, v_x0=True, H=64, L=4, meal_mode=0, meal=False, n_sets=1):
    """ONLY with arguments that fail validation: a supported shape with these fake pointers would launch."""
    lib = ctypes.CDLL(hode.lib_path())
    P, i = ctypes.c_void_p, ctypes.c_int
    fake = P(256)                                     # never dereferenced: validation fails first
    fn = getattr(lib, f"hode_solve_jvp_any_{sfx}")
    return fn(P(0), i(4), i(10), fake, i(0), fake if meal else P(0), i(meal_mode), P(0), i(0), P(0), i(0), fake, fake, i(n_sets),
              i(H), i(L), i(0), i(20), fake, fake, fake, i(K), fake if v_ode else P(0), fake if v_x0 else P(0), fake)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_jvp_any_arguments_are_checked_before_any_launch(sfx):
    assert _call(sfx, v_ode=False, v_x0=False) == EINVAL           # no direction
    assert _call(sfx, K=0) == EINVAL
    assert _call(sfx, K=-3) == EINVAL
    assert _call(sfx, meal_mode=1, meal=False) == EINVAL             # a mode without its pointer
    assert _call(sfx, meal_mode=3, meal=True) == EINVAL
    assert _call(sfx, n_sets=3) == EINVAL                           # B % n_sets
    assert _call(sfx, H=129) == EUNSUPPORTED
    assert _call(sfx, L=9) == EUNSUPPORTED
    assert _call(sfx, L=hode.capi.layers(4, 4)) == EUNSUPPORTED      # an activation code the library does not know
    assert _call(sfx, L=4 | hode.capi.NN_SHARED) == EUNSUPPORTED
    assert _call(sfx, H=129, K=0) == EINVAL                         # a bad argument outranks an unsupported shape
    assert _call(sfx, H=128, L=hode.capi.layers(5, hode.capi.ACT_TANH), n_sets=3) == EINVAL


# ------------------------------------------------------------------ 3. build checks
@pytest.fixture(scope="module")
def resource_usage(tmp_path_factory):
    """{source: [(kernel, scratch bytes per lane)]} of the two JVP sources, cross-compiled for gfx950."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = {}
    for src in ("hode_generic_jvp.hip", "hode_solve_jvp.hip"):
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-gpu-rdc", "--cuda-device-only", "-c",
                            os.path.join(CSRC, src), "-o", str(tmp_path_factory.mktemp("jvp") / "o.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, r.stderr[-3000:]
        out[src] = [(k, int(s)) for k, s in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S)]
    return out


def test_generic_jvp_kernels_cross_compile_without_scratch_in_fp32(resource_usage):
    kernels = resource_usage["hode_generic_jvp.hip"]
    gen = [(k, s) for k, s in kernels if k.startswith("_ZN4hode24solve_jvp_generic_kernelI")]
    f32 = [(k, s) for k, s in gen if k.startswith("_ZN4hode24solve_jvp_generic_kernelIf")]
    f64 = [(k, s) for k, s in gen if k.startswith("_ZN4hode24solve_jvp_generic_kernelId")]
    assert len(f32) >= 2 and len(f64) >= 2, kernels                 # with / without the Hill term, each dtype
    assert all(s == 0 for _, s in f32), f32


def test_tuned_jvp_source_still_yields_its_eight_fp32_kernels(resource_usage):
    kernels = resource_usage["hode_solve_jvp.hip"]
    f32 = [(k, s) for k, s in kernels if k.startswith("_ZN4hode16solve_jvp_kernelIf")]
    assert len(f32) == 8 and all(s == 0 for _, s in f32), kernels


def test_no_dpp_or_lds_hazard_in_the_generic_jvp_source():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dpp_hazard_check.py"), os.path.join(CSRC, "hode_generic_jvp.hip")],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "0 hazard(s)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------ 4. the oracle's tangent against finite differences
def test_oracle_jvp_of_a_tanh_network_matches_central_differences(O):
    """fp64, RK4 (one step per interval whatever the parameters: the forward is a fixed smooth map), tanh 96 x 5, B = 3, T = 7: every
    constant and every initial state against central differences of the oracle's own solve with relative step 1e-6, in the scaled
    norm.  The GPU test of sensitivities() uses ten times this bound."""
    c, F = GC.fd_case(), GC.FD
    L = IC.layers(F["L"], F["act"])
    run = lambda ode=None, x0=None, tape=False: O.solve(c["x0"] if x0 is None else x0, c["t"], c["meal"], None, None,   # noqa: E731
                                                        c["ode"] if ode is None else ode, c["nn"], F["H"], L, method=IC.RK4,
                                                        dtype=np.float64, want_tape=tape)
    sol = run(tape=True)
    assert (sol.status == 0).all()
    v_ode = np.zeros((JC.K_UNIT, 17))
    v_x0 = np.zeros((F["B"], JC.K_UNIT, 6))
    v_ode[np.arange(17), np.arange(17)] = 1.0
    v_x0[:, 17 + np.arange(6), np.arange(6)] = 1.0
    dy = O.solve_jvp(sol, v_ode, v_x0)
    bad = []
    for j in range(JC.K_UNIT):
        if j < 17:
            h = F["rel_step"] * abs(c["ode"][j])
            e = np.zeros(17)
            e[j] = h
            fd = (run(ode=c["ode"] + e).y - run(ode=c["ode"] - e).y) / (2 * h)
        else:
            h = F["rel_step"] * max(np.abs(c["x0"][:, j - 17]).max(), 1.0)
            e = np.zeros(6)
            e[j - 17] = h
            fd = (run(x0=c["x0"] + e).y - run(x0=c["x0"] - e).y) / (2 * h)
        if np.abs(fd).max() == 0:
            assert j in JC.GD_ONLY and np.abs(dy[:, j]).max() == 0, j            # no GD input: IGD_50 and g move nothing
            continue
        err = JC.scaled_norm(dy[:, j], fd)
        print(f"FIGURE oracle fd {JC.DIR_NAMES[j]} err {err:.3e}")
        if not err <= F["bound_oracle"]:
            bad.append(f"{JC.DIR_NAMES[j]}: {err:.3e}")
    assert not bad, bad


# ------------------------------------------------------------------ 5. admission of the calibration case
def test_calibration_case_is_recovered_by_lm_around_the_oracle(O):
    """levenberg_marquardt with an oracle-backed callback (oracle solve + oracle JVP, fp64, DP5(4) at rtol 1e-10), least squares in
    the coordinates fit_patients uses without priors (z = theta / theta at the start): every patient ends with status 0 and its
    constants to 1e-7."""
    from inference.calibrate import levenberg_marquardt
    C, c = GC.CAL, GC.calibration_case()
    obs = GC.calibration_observations(O)
    B, K, T = C["B"], len(GC.CAL_NAMES), C["T"]
    L = IC.layers(C["L"], C["act"])
    s = c["ode"][c["idx"]]                                # the starting values = the model's constants
    v_ode = np.zeros((K, 17))
    v_ode[np.arange(K), c["idx"]] = 1.0

    def fn(z, want_jac):
        theta = z.numpy() * s
        r, J, ok = np.zeros((B, T * 6)), np.zeros((B, T * 6, K)), np.zeros(B, bool)
        for b in range(B):
            ode = c["ode"].copy()
            ode[c["idx"]] = theta[b]
            sol = O.solve(c["x0"][b:b + 1], c["t"], c["meal"][b:b + 1], None, None, ode, c["nn"], C["H"], L, method=IC.DP5, rtol=C["rtol"],
                          atol=C["atol"], max_steps=C["max_steps"], dtype=np.float64, want_tape=want_jac)
            ok[b] = sol.status[0] == 0
            r[b] = ((sol.y[0] - obs[b]) / C["sigma"]).reshape(-1)
            if want_jac:
                S = O.solve_jvp(sol, v_ode, None)[0]      # [K, T, 6]
                J[b] = S.reshape(K, T * 6).T / C["sigma"] * s
        return torch.tensor(r), (torch.tensor(J) if want_jac else None), torch.tensor(ok)
    out = levenberg_marquardt(fn, torch.ones(B, K, dtype=torch.float64), torch.zeros(K), max_iter=100)
    assert (out["status"].numpy() == 0).all(), out["status"]
    theta = out["z"].numpy() * s
    for k, n in enumerate(GC.CAL_NAMES):
        rel = np.abs(theta[:, k] - c["truth"][n]) / np.abs(c["truth"][n])
        print(f"FIGURE calibration admission {n} rel {rel.max():.3e}")
        assert rel.max() <= C["bound_oracle"], (n, rel)
