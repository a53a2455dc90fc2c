"""The forward solve kernels on the paths that tests/golden/fwd_asm_merge/ does not reach -- the Hill term (the rolled-stage
instantiation) under DP5(4) and RK4, the MULTI routing (two trajectories per wave), each with three and with two hidden matrices,
several parameter sets per launch, an all-zero hidden input with H = 16 -- give the bits they gave before the forward kernels'
hidden layer was touched: any form of that layer issues the same products in the same order per accumulator.

The fixtures under tests/golden/fwd_lds_rot/ were recorded on an MI355X from the library of the commit before that work
(tools/record_fwd_lds_rot.py); tests/_fwd_lds_rot_cases.py holds the cases."""
import os

import numpy as np
import pytest

import _fwd_asm_merge_cases as A
import _fwd_lds_rot_cases as C

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
    assert sorted(want) == sorted(keys)
    for k in keys:
        a, b = torch.from_numpy(np.ascontiguousarray(got[k])), torch.from_numpy(np.ascontiguousarray(want[k]))
        assert a.dtype == b.dtype and torch.equal(a, b), k


# (L = 4 DP5(4) with the Hill term keeps mlp_hidden_blk; L = 3, and RK4 at L = 4, run the LDS-fed layer inside the rolled stage loop)
@pytest.mark.parametrize("name,L,taped,method", [("gd", 4, False, 0), ("gd_tape", 4, True, 0), ("gd_l3", 3, False, 0), ("gd_tape_l3", 3, True, 0),
                                                 ("rk4_gd_l4", 4, False, 1)])
def test_hill_term_bits(hode, weights, name, L, taped, method):
    inp, want = load(name)
    assert inp["x0"].shape == (3, 6) and inp["t"].shape == (5,) and inp["gd"].shape == (3, 5)      # gd_mode 2
    got = C.run(hode, torch, inp, A.sub_network(weights[0], C.H0, L), weights[1], C.H0, L, taped=taped, method=method)
    assert_same_bits(got, want, ("y", "status", "nsteps", "nfev") + (("gx0", "gnn") if taped else ()))
    assert int(got["status"].max()) == 0 and int(got["nsteps"].min()) >= 4


@pytest.mark.parametrize("name,L", [("multi", 4), ("multi_l3", 3)])        # L = 3: the wave's LDS buffer is reused by its second trajectory
def test_multi_routing_bits(hode, weights, name, L):
    _, want = load(name)
    inp = C.multi_inputs()
    assert inp["x0"].shape[0] == C.MULTI_B > 8192 and inp["t"].shape[0] == C.MULTI_T <= 4         # the MULTI routing's conditions
    out = C.run(hode, torch, inp, A.sub_network(weights[0], C.H0, L), weights[1], C.H0, L)
    assert int(out["status"].max()) == 0
    assert_same_bits(C.multi_digest(out), want, ("y", "status", "nsteps", "nfev", "y_sha256"))


def test_parameter_sets_bits(hode):
    inp, want = load("sets")
    assert inp["x0"].shape == (6, 6) and inp["ode"].shape == (3 * 17,)
    got = C.run(hode, torch, inp, inp["nn"], inp["ode"], C.H0, 3, n_sets=3)
    assert_same_bits(got, want, ("y", "status", "nsteps", "nfev"))
    assert int(got["status"].max()) == 0


def test_zero_hidden_input_bits(hode, weights):
    inp, want = load("zero_in")
    assert inp["x0"].shape == (2, 6) and inp["t"].shape == (4,)
    nn = C.zero_input_network(weights[0], 16, C.L0)
    assert not nn[:10 * 16].any() and nn[10 * 16:].any()
    got = C.run(hode, torch, inp, nn, weights[1], 16, C.L0)
    assert_same_bits(got, want, ("y", "status", "nsteps", "nfev"))
    assert int(got["status"].max()) == 0
