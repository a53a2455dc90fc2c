"""mlp_hidden_blk (csrc/hode_mlp.h) issues each rotation's DPP move and its two packed FMAs from one asm statement, and the
pads of the layer finish and of out_rot that no hazard needs are gone.  Same instructions, same order per accumulator: the
forward solve, the taping forward and its adjoint, the RHS kernel and the tangent-linear pass give the bits they gave before.

The fixtures under tests/golden/fwd_asm_merge/ were recorded on an MI355X from the library of the commit before that change
(tools/record_fwd_asm_merge.py); tests/_fwd_asm_merge_cases.py holds the cases."""
import os

import numpy as np
import pytest

import _fwd_asm_merge_cases as C

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


@pytest.mark.parametrize("case", C.SOLVE_CASES, ids=[c[0] for c in C.SOLVE_CASES])
def test_solve_bits(hode, weights, case):
    name, B, T, H, L, method, taped = case
    inp, want = load(name)
    assert inp["x0"].shape == (B, 6) and inp["t"].shape == (T,)
    got, _ = C.run_solve(hode, torch, inp, C.sub_network(weights[0], H, L), weights[1], H, L, method, taped)
    assert_same_bits(got, want, ("y", "status", "nsteps", "nfev") + (("gx0", "gnn") if taped else ()))
    assert int(got["status"].max()) == 0 and int(got["nsteps"].min()) >= T - 1


def test_rejected_steps_bits(hode, weights):
    inp, want = load("rejected")
    got, _ = C.run_solve(hode, torch, inp, C.sub_network(weights[0], C.H0, C.L0), weights[1], C.H0, C.L0, 0, False,
                         rtol=C.REJECT_RTOL, atol=C.REJECT_ATOL)
    assert_same_bits(got, want, ("y", "status", "nsteps", "nfev"))
    assert inp["x0"].shape == (1, 6) and int(got["nfev"][0]) > 2 + 6 * int(got["nsteps"][0])      # it did reject steps


def test_rhs_kernel_bits(hode, weights):
    inp, want = load("rhs")
    assert inp["x"].shape == (5, 6)
    assert_same_bits(C.run_rhs(hode, torch, inp, C.sub_network(weights[0], C.H0, C.L0), weights[1]), want, ("f",))


def test_jvp_bits(hode, weights):
    inp, want = load("jvp")
    assert inp["x0"].shape == (3, 6) and inp["t"].shape == (5,)
    got = C.run_jvp(hode, torch, inp, C.sub_network(weights[0], C.H0, C.L0), weights[1])
    assert_same_bits(got, want, ("y", "status", "nsteps", "nfev", "dy"))
