"""GPU tests: every input-gradient kernel (hode.solve_bwd_inputs, hode.rhs_bwd_inputs) against the fp64 C oracle on the cases of
tests/_input_grad_cases.py -- one parametrised test per part of the table (its docstring has the parts, the tolerances and the
measured error ratios).  Each test: solve_fwd(want_tape) + solve_bwd_inputs (or rhs_bwd_inputs), the oracle on the same arrays,
status / nsteps equal to the oracle's at the same dtype, every returned quantity by relative norm, structural zeros with ==.
tests/test_input_grads_oracle.py pins the oracle itself (fixture G10) and admits the cases on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _input_grad_cases as IC
from _input_grad_cases import KEYS, relnorm

pytestmark = pytest.mark.gpu

TORCH_DT = {"f64": torch.float64, "f32": torch.float32}


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.asarray(a)).to("cuda", TORCH_DT[dt]).contiguous()


def host(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O                          # checker only
    return O


def _find(part, name):
    return next(c for c in IC.SOLVE[part] if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _solve_refs(part, name, dt):
    """(data, fp64 oracle at the solver tolerances of dtype dt, oracle at dt) -- computed once per case and dtype."""
    c = _find(part, name)
    d = IC.solve_data(c)
    r64 = IC.oracle_solve(_oracle(), dict(c, **IC.solver_tols(c, dt)), "f64", d)
    return d, r64, (r64 if dt == "f64" else IC.oracle_solve(_oracle(), c, "f32", d))


def _kernel_solve(c, dt, d, want_inputs=KEYS):
    import hode
    tol = IC.solver_tols(c, dt)
    sol = hode.solve_fwd(dev(d["x0"], dt), dev(d["t"], dt), *(dev(v, dt) for v in d["u"]), dev(d["ode"], dt), dev(d["nn"], dt), c["H"],
                         IC.layers(c["L"], c["act"]), method=c["method"], rtol=tol["rtol"], atol=tol["atol"], max_steps=c["max_steps"],
                         n_sets=c["n_sets"], want_tape=True)
    gx0, gnn, gode, gin = hode.solve_bwd_inputs(sol, dev(d["gy"], dt), want_gnn=c["want_gnn"], want_gode=c["want_gode"],
                                                want_inputs=want_inputs)
    return sol, gx0, gnn, gode, gin


def _compare(part, label, kind, dt, got, r64, rdt, bad):
    """Every key by relative norm against the fp64 oracle; fp32: within FP32_MARGIN x the oracle's own fp32-against-fp64 distance."""
    for k in IC.ALL_KEYS:
        if r64[k] is None:
            if got[k] is not None:
                bad.append(f"{label} {k}: returned for an absent or unwanted quantity")
            continue
        if got[k] is None:
            bad.append(f"{label} {k}: missing")
            continue
        g = np.asarray(got[k]).reshape(r64[k].shape)
        err = relnorm(g, r64[k])
        d_ref = relnorm(rdt[k], r64[k]) if dt == "f32" else 0.0
        tol = IC.tolerance(part, kind, dt, d_ref)
        print(f"FIGURE {label} {k} err {err:.3e} d_ref {d_ref:.3e} ratio {err / d_ref if d_ref else float('nan'):.2f} tol {tol:.3e}")
        if not (np.isfinite(g).all() and err <= tol):
            bad.append(f"{label} {k}: err {err:.3e} > tol {tol:.3e} (d_ref {d_ref:.3e})")


def _check_solve(part, c, dt):
    d, r64, rdt = _solve_refs(part, c["name"], dt)
    sol, gx0, gnn, gode, gin = _kernel_solve(c, dt, d)
    label = f"{part}/{c['name']}-{dt}"
    st, ns = host(sol.status), host(sol.nsteps)
    assert np.array_equal(st, rdt["status"]) and (st == c["expect_status"]).all(), (label, st, rdt["status"])
    assert np.array_equal(ns, rdt["nsteps"]), (label, ns, rdt["nsteps"])
    got = dict(meal=host(gin["meal"]), tVNS=host(gin["tVNS"]), GD=host(gin["GD"]), gx0=host(gx0), gnn=host(gnn), gode=host(gode))
    bad = []
    _compare(part, label, c["method"], dt, got, r64["g"], rdt["g"], bad)
    for k, m in zip(KEYS, c["modes"]):
        if got[k] is None:
            continue
        assert got[k].shape == d["u"][KEYS.index(k)].shape, (label, k)
        if m == 2:
            # rows that bound no taped step -- and, after a failure, every row the oracle leaves at exactly 0 -- are exactly 0
            must0 = ~rdt["touched"] | ((rdt["g"][k] == 0) if c["expect_status"] else False)
            if not (got[k][must0] == 0).all():
                bad.append(f"{label} {k}: rows that must be exactly 0 are not: {np.argwhere(must0 & (got[k] != 0)).tolist()}")
            if c["zero_rows"] is not None and not (got[k][:, list(c["zero_rows"])] == 0).all():
                bad.append(f"{label} {k}: rows {c['zero_rows']} are not exactly 0")
    if c["gd_zero_rows"] == (0, 1):
        if not ((got["GD"][:, 0] == 0).all() and (got["GD"][:, 1] != 0).all()):
            bad.append(f"{label} GD: the interval between two GD rows of 0 must add exactly 0 to row 0, its neighbour not to row 1")
    assert not bad, "\n".join(bad)
    return sol, got


@pytest.mark.parametrize("c,dt", IC.params(IC.SOLVE["a"]), ids=IC.ids(IC.SOLVE["a"]))
def test_a_tuned_solve_instantiations(c, dt):
    assert c["H"] <= 64 and c["L"] <= 4 and c["act"] == IC.RELU
    _check_solve("a", c, dt)


@pytest.mark.parametrize("c,dt", IC.params(IC.SOLVE["b"]), ids=IC.ids(IC.SOLVE["b"]))
def test_b_generic_solve_families(c, dt):
    _check_solve("b", c, dt)


@pytest.mark.parametrize("c,dt", IC.params(IC.SOLVE["c"]), ids=IC.ids(IC.SOLVE["c"]))
def test_c_row_bookkeeping_edges(c, dt):
    _check_solve("c", c, dt)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("tag", [t for t, _, _ in IC.EDGE_NETS])
def test_c_want_inputs_subsets(tag, dt):
    """The wanted gradients are those of the launch that wants all three, bit for bit; the unwanted ones are None."""
    c = _find("c", f"{tag}-tbatched")
    d = IC.solve_data(c)
    _, gx0, gnn, gode, full = _kernel_solve(c, dt, d)
    for sub in IC.WANT_SUBSETS:
        _, gx0s, _, _, gin = _kernel_solve(c, dt, d, want_inputs=sub)
        assert torch.equal(gx0s, gx0), sub
        for k in KEYS:
            if k in sub:
                assert gin[k] is not None and torch.equal(gin[k], full[k]), (sub, k)
            else:
                assert gin[k] is None, (sub, k)


@pytest.mark.parametrize("c,dt", IC.params(IC.SOLVE["d"]), ids=IC.ids(IC.SOLVE["d"]))
def test_d_several_tapes_per_wave(c, dt):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    two = IC.waves_with_two_tapes(cus)
    assert two > 0, (f"{cus} compute units: {c['n_sets']} sets x {c['B'] // c['n_sets']} trajectories leave every wave of the tuned adjoint one "
                     "tape -- this case would not exercise a wave's second walk; it needs another shape on this device")
    _check_solve("d", c, dt)


@pytest.mark.parametrize("c,dt", IC.params(IC.SOLVE["e"]), ids=IC.ids(IC.SOLVE["e"]))
def test_e_failed_trajectory(c, dt):
    sol, got = _check_solve("e", c, dt)
    assert (host(sol.status) == 1).all() and (host(sol.nsteps) == c["max_steps"]).all()
    for k in KEYS:
        assert (got[k][:, -2:] == 0).all() and np.abs(got[k]).max() > 0, k


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("c", IC.RHS, ids=[c["name"] for c in IC.RHS])
def test_f_rhs(c, dt):
    import hode
    O = _oracle()
    bad = []
    for B in IC.RHS_B:
        for present in IC.RHS_SUBSETS:
            d = IC.rhs_data(c, B, present)
            r64 = IC.oracle_rhs(O, c, B, present, "f64", d)
            rdt = r64 if dt == "f64" else IC.oracle_rhs(O, c, B, present, "f32", d)
            gx, _, gnn, gode, gin = hode.rhs_bwd_inputs(dev(d["x"], dt), dev(d["t"], dt), *(dev(v, dt) for v in d["u"]), dev(d["ode"], dt),
                                                        dev(d["nn"], dt), c["H"], IC.layers(c["L"], c["act"]), dev(d["w"], dt),
                                                        want_gnn=True, want_gode=c["want_gode"])
            got = dict(meal=host(gin["meal"]), tVNS=host(gin["tVNS"]), GD=host(gin["GD"]), gx0=host(gx), gnn=host(gnn), gode=host(gode))
            label = f"f/{c['name']}-{dt}-B{B}-{'+'.join(present)}"
            _compare("f", label, "rhs", dt, got, r64, rdt, bad)
            if "GD" in present:
                special = np.concatenate(IC.rhs_gd_special(B))
                if not ((got["GD"][special] == 0).all() and (np.delete(got["GD"], special) != 0).all()):
                    bad.append(f"{label} GD: the gradient at GD <= 0 must be exactly 0, elsewhere not")
    assert not bad, "\n".join(bad)
