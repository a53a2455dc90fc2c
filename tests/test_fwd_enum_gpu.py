"""GPU tests: every forward-solve instantiation (hode.solve_fwd: the 64 one-trajectory kernels and the 4 MULTI kernels of
csrc/hode_solve_fwd.hip, and the generic team kernels of the same dispatch) against the fp64 C oracle in what it returns -- y, status,
nsteps, nfev -- on the cases of tests/_fwd_enum_cases.py; its docstring has the parts, the figures, the tolerances and the measured
error ratios.  One parametrised test per part: run the kernel (taped and untaped where the case has both, every launch twice), the
oracle on the same arrays, compare().  tests/test_fwd_enum_oracle.py admits the cases on the CPU."""
import numpy as np
import pytest
import torch

import _fwd_enum_cases as FE
import _input_grad_cases as IC

pytestmark = pytest.mark.gpu

TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
KEYS = ("y", "status", "nsteps", "nfev")


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.asarray(a)).to("cuda", TORCH_DT[dt]).contiguous()


def _run(c, dt, dd, tape, rows=None, n_sets=None):
    """One launch of hode.solve_fwd on the device arrays dd (rows: a slice of trajectories of ONE parameter set n_sets[1])."""
    import hode
    tol = IC.solver_tols(c, dt)
    P = IC.n_params(c["H"], c["L"])
    sl = slice(None) if rows is None else rows
    t = dd["t"][sl] if c["t_batched"] else dd["t"]
    nn, ode, ns = dd["nn"], dd["ode"], c["n_sets"]
    if n_sets is not None:
        s = n_sets[1]
        nn, ode, ns = nn[P * s:P * (s + 1)], ode[17 * s:17 * (s + 1)], 1
    sol = hode.solve_fwd(dd["x0"][sl], t, *(None if v is None else v[sl] for v in dd["u"]), ode, nn, c["H"], IC.layers(c["L"], c["act"]),
                         method=c["method"], rtol=tol["rtol"], atol=tol["atol"], max_steps=c["max_steps"], n_sets=ns, want_tape=tape)
    return {k: getattr(sol, k) for k in KEYS}


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _equal(a, b):
    # bits: row 0 of a trajectory with a NaN in x0 must compare equal to itself
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


def _check(part, c, dt, slices=False):
    d = FE.refs(part, c["name"], dt)[0]
    dd = dict(x0=dev(d["x0"], dt), t=dev(d["t"], dt), u=[dev(v, dt) for v in d["u"]], nn=dev(d["nn"], dt), ode=dev(d["ode"], dt))
    bad, first = [], None
    for tape in c["tapes"]:
        label = f"{part}/{c['name']}-{dt}-{'taped' if tape else 'untaped'}"
        got = _run(c, dt, dd, tape)
        again = _run(c, dt, dd, tape)
        if not _equal(got, again):
            bad.append(f"{label}: a second launch gives other bits")
        if first is None:
            first = got
            bad += FE.compare(part, c, dt, {k: v.cpu().numpy() for k, v in got.items()}, label=label)
        elif not _equal(got, first):
            bad.append(f"{label}: the taped run differs from the untaped one in " + ", ".join(k for k in KEYS if not torch.equal(_bits(got[k]), _bits(first[k]))))
    if slices:
        per = c["B"] // c["n_sets"]
        parts = [_run(c, dt, dd, False, slice(lo, min(lo + 8192, (s + 1) * per)), (1, s)) for s in range(c["n_sets"])
                 for lo in range(s * per, (s + 1) * per, 8192)]
        cat = {k: torch.cat([p[k] for p in parts]) for k in KEYS}
        if not _equal(cat, first):
            w = torch.nonzero((cat["y"] != first["y"]).flatten(1).any(1) | (cat["nfev"] != first["nfev"])).flatten()
            bad.append(f"{part}/{c['name']}: differs from the same rows run in slices of <= 8 192 at {len(w)} trajectories, first {w[:6].tolist()}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c,dt", FE.params("a"), ids=FE.ids("a"))
def test_a_one_trajectory_instantiations(c, dt):
    _check("a", c, dt)


@pytest.mark.parametrize("c,dt", FE.params("b"), ids=FE.ids("b"))
def test_b_row_bookkeeping(c, dt):
    _check("b", c, dt)


@pytest.mark.parametrize("c,dt", FE.params("c"), ids=FE.ids("c"))
def test_c_parameter_sets(c, dt):
    _check("c", c, dt)


@pytest.mark.parametrize("c,dt", FE.params("d"), ids=FE.ids("d"))
def test_d_multi_and_its_neighbours(c, dt):
    _check("d", c, dt, slices=True)


@pytest.mark.parametrize("c,dt", FE.params("e"), ids=FE.ids("e"))
def test_e_generic_teams_with_the_hill_term(c, dt):
    _check("e", c, dt)
