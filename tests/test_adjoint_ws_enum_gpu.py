"""GPU tests: the fp32 training adjoint (hode.solve_bwd: csrc/hode_solve_bwd_ws.hip for 2-4 hidden layers, the one-role kernel of
csrc/hode_solve_bwd.hip where that one declines) against the fp64 C oracle on the cases of tests/_adjoint_ws_cases.py -- one
parametrised test per part of the table (its docstring has the parts, the figures, the tolerances and the measured ratios).  Each test:
the path the launch takes at this device's compute-unit count, solve_fwd(want_tape) + solve_bwd, the comparison of the case module
(status / nsteps equal to the fp32 oracle's, gnn block by block and set by set, gx0 trajectory by trajectory, gode against s_e, exact
zeros), and the same bits on a second launch.  tests/test_adjoint_ws_oracle.py admits the cases on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _adjoint_ws_cases as WC

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.as_tensor(np.asarray(a)).to("cuda", torch.float32).contiguous()


def host(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O                          # checker only
    return O


@functools.lru_cache(maxsize=None)
def _refs(part, name):
    return WC.references(_oracle(), WC.find(part, name))


def _kernel(c, d):
    import hode
    tol = WC.fp32_tols(c)
    sol = hode.solve_fwd(dev(d["x0"]), dev(d["t"]), *(dev(v) for v in d["u"]), dev(d["ode"]), dev(d["nn"]), c["H"], WC.IC.layers(c["L"], c["act"]),
                         method=c["method"], rtol=tol["rtol"], atol=tol["atol"], max_steps=c["max_steps"], n_sets=c["n_sets"], want_tape=True)
    gy = dev(d["gy"])
    first = hode.solve_bwd(sol, gy, want_gnn=c["want_gnn"], want_gode=c["want_gode"])
    second = hode.solve_bwd(sol, gy, want_gnn=c["want_gnn"], want_gode=c["want_gode"])
    return sol, first, second


def _check(part, c):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    path = WC.ws_launch(c["B"], c["n_sets"], c["L"], c["want_gode"], cus)
    assert path == c["path"], (f"{cus} compute units: {c['n_sets']} sets x {c['B'] // c['n_sets']} trajectories take {path}, this case is about "
                               f"{c['path']} -- it needs another shape on this device")
    ref = _refs(part, c["name"])
    sol, (gx0, gnn, gode), second = _kernel(c, ref["d"])
    got = dict(status=host(sol.status), nsteps=host(sol.nsteps), gx0=host(gx0), gnn=host(gnn), gode=host(gode))
    bad, worst = WC.compare(c, got, ref)
    print(f"WORST {part}/{c['name']} ratio {worst[0]:.2f} at {worst[1]}[{worst[2]}], largest err {worst[3]:.3e}")
    for k, a, b in zip(("gx0", "gnn", "gode"), (gx0, gnn, gode), second):
        if a is not None and not torch.equal(a, b):
            bad.append(f"{part}/{c['name']} {k}: a second launch gives other bits")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("c", WC.CASES["a"], ids=WC.ids("a"))
def test_a_every_instantiation_with_its_slots_in_use(c):
    _check("a", c)


@pytest.mark.parametrize("c", WC.CASES["b"], ids=WC.ids("b"))
def test_b_row_bookkeeping(c):
    _check("b", c)


@pytest.mark.parametrize("c", WC.CASES["c"], ids=WC.ids("c"))
def test_c_mixed_lengths_inside_one_workgroup(c):
    _check("c", c)


@pytest.mark.parametrize("c", WC.CASES["d"], ids=WC.ids("d"))
def test_d_neighbouring_paths(c):
    _check("d", c)
