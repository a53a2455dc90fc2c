"""GPU tests: the training adjoint of generic networks (hode.solve_bwd: the multi-trajectory teams of csrc/hode_generic_bwd_multi.hip
above 256 fp32 trajectories, the one-trajectory teams of csrc/hode_generic_bwd.hip elsewhere) and K5 without input gradients
(hode.rhs_bwd) against the fp64 C oracle on the cases of tests/_generic_adjoint_cases.py -- one parametrised test per part of the
table (its docstring has the parts, the figures, the tolerances and the measured ratios).  Each solve test: solve_fwd(want_tape) +
solve_bwd, the comparison of the case module (status / nsteps equal to the oracle's, gnn block by block, row block by row block and set
by set, gx0 trajectory by trajectory, gode against s_e, exact zeros), and on every rows-mode and multi case the same bits on a second
launch.  tests/test_generic_adjoint_oracle.py admits the cases and checks the paths they name on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _generic_adjoint_cases as GC

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


@functools.lru_cache(maxsize=None)
def _refs(part, name):
    return GC.references(_oracle(), GC.find(part, name))


def _kernel(c, d):
    import hode
    dt = c["dt"]
    sol = hode.solve_fwd(dev(d["x0"], dt), dev(d["t"], dt), *(dev(v, dt) for v in d["u"]), dev(d["ode"], dt), dev(d["nn"], dt), c["H"],
                         GC.layers(c["L"], c["act"]), method=c["method"], rtol=c["rtol"], atol=c["atol"], max_steps=c["max_steps"],
                         n_sets=c["n_sets"], want_tape=True)
    gy = dev(d["gy"], dt)
    first = hode.solve_bwd(sol, gy, want_gnn=c["want_gnn"], want_gode=c["want_gode"])
    second = hode.solve_bwd(sol, gy, want_gnn=c["want_gnn"], want_gode=c["want_gode"])
    return sol, first, second


def _check(part, c):
    ref = _refs(part, c["name"])
    sol, (gx0, gnn, gode), second = _kernel(c, ref["d"])
    got = dict(status=host(sol.status), nsteps=host(sol.nsteps), gx0=host(gx0), gnn=host(gnn), gode=host(gode))
    bad, worst = GC.compare(c, got, ref)
    print(f"WORST {part}/{c['name']} figures {worst[4]} ratio {worst[0]:.2f} at {worst[1]}[{worst[2]}], largest err {worst[3]:.3e}")
    if c["takes"][0] == "multi" or c["takes"][3]:              # gradient rows, added in workgroup order: no floating-point atomics
        for k, a, b in zip(("gx0", "gnn", "gode"), (gx0, gnn, gode), second):
            if a is not None and not torch.equal(a, b):
                bad.append(f"{part}/{c['name']} {k}: a second launch gives other bits")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("c", GC.CASES["a"], ids=GC.ids("a"))
def test_a_every_multi_instantiation(c):
    _check("a", c)


@pytest.mark.parametrize("c", GC.CASES["b"], ids=GC.ids("b"))
def test_b_row_bookkeeping_inside_a_team(c):
    _check("b", c)


@pytest.mark.parametrize("c", GC.CASES["c"], ids=GC.ids("c"))
def test_c_sets_and_looping_workgroups(c):
    _check("c", c)


@pytest.mark.parametrize("c", GC.CASES["d"], ids=GC.ids("d"))
def test_d_one_trajectory_neighbours(c):
    _check("d", c)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("c", GC.RHS, ids=[c["name"] for c in GC.RHS])
def test_e_rhs_bwd_without_input_gradients(c, dt):
    import hode
    O = _oracle()
    bad, worst = [], (0.0, None)
    for B in GC.RHS_B:
        for present in GC.RHS_SUBSETS:
            d, r64, r32 = GC.rhs_refs(O, c, B, present)
            gx, gt, gnn, gode = hode.rhs_bwd(dev(d["x"], dt), dev(d["t"], dt), *(dev(v, dt) for v in d["u"]), dev(d["ode"], dt), dev(d["nn"], dt),
                                             c["H"], GC.layers(c["L"], c["act"]), dev(d["w"], dt), want_gt=(dt == "f64"), want_gnn=True,
                                             want_gode=c["want_gode"])
            label = f"{c['name']}-{dt}-B{B}-{'+'.join(present)}"
            for f in GC.compare_rhs(c, dt, label, dict(gx0=host(gx), gnn=host(gnn), gode=host(gode)), r64, r32, bad):
                worst = max(worst, (f[0], f"{label} {f[1]} err {f[2]:.3e} d_ref {f[3]:.3e}"))
            if dt == "f64":
                fd = GC.rhs_gt_reference(O, c, d)
                err = float(np.max(np.abs(host(gt) - fd)))
                print(f"FIGURE e/{label} gt err {err:.3e} scale {max(1.0, np.abs(fd).max()):.3e}")
                if not err < 1e-4 * max(1.0, np.abs(fd).max()):
                    bad.append(f"{label} gt: {err:.3e} from the central difference")
    print(f"WORST e/{c['name']}-{dt} ratio {worst[0]:.2f} at {worst[1]}")
    assert not bad, "\n".join(bad[:40])
