"""The per-stage work of the forward solve AROUND the hidden layers -- stage time, forcing at the stage time, state broadcasts,
mechanistic terms, first layer -- gives the bits it gave before it was trimmed, on the paths that tests/golden/fwd_asm_merge/ and
tests/golden/fwd_lds_rot/ do not pin: tVNS different at every grid point with a constant meal per trajectory, a meal pulse that makes the
controller reject a step and take two steps in one interval, a repeated grid time, a z-scored initial state that ends in a step-size
underflow (status 2); each with L = 4 plain (the benchmark instantiation), L = 4 taped with its adjoint, L = 3 and RK4; and the RHS
and tangent-linear entry points on the same states.

The fixtures under tests/golden/fwd_stage_trim/ were recorded on an MI355X from the library of the commit before that work
(tools/record_fwd_stage_trim.py); tests/_fwd_stage_trim_cases.py holds the cases."""
import os

import numpy as np
import pytest

import _fwd_asm_merge_cases as A
import _fwd_stage_trim_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hode():
    import hode
    assert not os.environ.get("HODE_LIB"), "this test is about the product library"
    return hode


@pytest.fixture(scope="module")
def weights(golden_dir):
    w = np.load(os.path.join(golden_dir, "g0_weights_h64_l4.npz"))
    return w["nn_flat"].astype(np.float32), w["ode"].astype(np.float32)


def load(name):
    d = np.load(C.fixture(name))
    return ({k[3:]: d[k] for k in d.files if k.startswith("in_")}, {k[4:]: d[k] for k in d.files if k.startswith("out_")})


def assert_same_bits(got, want, keys):
    assert sorted(want) == sorted(keys) and sorted(got) == sorted(keys)
    for k in keys:
        assert C.same_bits(got[k], want[k]), k               # bytes, so that NaNs of a failed trajectory compare too


def test_the_fixtures_hold_the_paths_they_are_for():
    """What the recorder refuses to write without, read back from what it wrote (no GPU work)."""
    inp, want = load("tvns_l4")
    assert inp["x0"].shape == (C.B, 6) and inp["t"].shape == (C.T,) and inp["meal"].shape == (C.B,) and inp["tvns"].shape == (C.B, C.T)
    assert (inp["tvns"] != 0).all() and (np.diff(inp["tvns"], axis=1) != 0).all() and int(want["status"].max()) == 0
    assert inp["t"][C.REPEAT] == inp["t"][C.REPEAT - 1]
    inp, want = load("pulse_l4")
    assert inp["meal"].shape == (C.B, C.T) and inp["t"][C.REPEAT] == inp["t"][C.REPEAT - 1]
    assert (want["nfev"] > 6 * want["nsteps"] + 2).any()                                            # a rejected step
    assert ((want["status"] == 0) & (want["nsteps"] > C.positive_intervals(inp["t"]))).any()         # an interval with two steps
    assert int(want["status"][C.B - 1]) == 2                                                         # the z-scored state


@pytest.mark.parametrize("name,L,taped,method", [(n, L, tp, m) for n, _, L, tp, m in C.SOLVE_CASES])
def test_solve_bits(hode, weights, name, L, taped, method):
    inp, want = load(name)
    got, _ = C.run(hode, torch, inp, A.sub_network(weights[0], C.H0, L), weights[1], C.H0, L, taped=taped, method=method)
    assert_same_bits(C.digest(got), want, C.SOLVE_KEYS + (("gx0", "gnn_some", "gnn_sha256") if taped else ()))


def test_rhs_bits(hode, weights):
    inp, want = load("rhs")
    assert inp["x"].shape == (2 * C.B, 6)
    assert_same_bits(C.run_rhs(hode, torch, inp, A.sub_network(weights[0], C.H0, C.L0), weights[1]), want, ("f",))


def test_jvp_bits(hode, weights):
    inp, want = load("jvp")
    got = C.run_jvp(hode, torch, inp, A.sub_network(weights[0], C.H0, C.L0), weights[1])
    assert_same_bits(got, want, C.SOLVE_KEYS + ("dy",))
    assert int(got["status"].max()) == 0 and got["dy"].shape == (C.B, 2, C.T, 6)
