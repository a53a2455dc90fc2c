#!/usr/bin/env python3
"""Record the fixtures of tests/test_fwd_asm_merge_gpu.py (GPU box):

    HODE_LIB=<libhode.so of the commit BEFORE the change> python tools/record_fwd_asm_merge.py [out_dir]

The test holds the fp32 register path to the bits of that earlier library, so the fixtures are only ever recorded from a library
that predates the edit under test (HODE_LIB; without it the tree's own library is recorded, which checks nothing).  Every case is
computed twice and must give the same bits both times; the rejected-steps case is searched for among a few pulse heights and
kept only if the solve really rejected steps (nfev > 2 + 6 nsteps)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hode  # noqa: E402
import _fwd_asm_merge_cases as C  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else C.FIXTURE_DIR
os.makedirs(out_dir, exist_ok=True)
w = np.load(os.path.join(ROOT, "tests", "golden", "g0_weights_h64_l4.npz"))
ode = w["ode"].astype(np.float32)
print("library:", hode.lib_path(), hode.version())


def same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def save(name, inp, out):
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **{"in_" + k: v for k, v in inp.items()}, **{"out_" + k: v for k, v in out.items()})
    print(f"  {name}: {os.path.getsize(path) / 1024:.1f} KiB  " + "  ".join(f"{k}{list(v.shape)}" for k, v in out.items()))


for i, (name, B, T, H, L, method, taped) in enumerate(C.SOLVE_CASES):
    x0, t, meal, tvns = C.make_inputs(B, T, 100 + i)
    inp = dict(x0=x0, t=t, meal=meal, tvns=tvns)
    if taped:
        inp["c"] = np.random.default_rng(200 + i).standard_normal((B, T, 6)).astype(np.float32)
    nn = C.sub_network(w["nn_flat"], H, L)
    out, _ = C.run_solve(hode, torch, inp, nn, ode, H, L, method, taped)
    again, _ = C.run_solve(hode, torch, inp, nn, ode, H, L, method, taped)
    assert same(out, again), name
    assert int(out["status"].max()) == 0, (name, out["status"])
    print(f"  {name}: nsteps {out['nsteps'].tolist()} nfev {out['nfev'].tolist()}")
    save(name, inp, out)

# rejected steps: one trajectory, one meal pulse on an otherwise quiet grid, tolerances 1e-8 / 1e-10
nn = C.sub_network(w["nn_flat"], C.H0, C.L0)
chosen = None
for T, height in ((9, 1.0), (9, 10.0), (9, 50.0), (13, 100.0), (13, 500.0)):
    x0, t, _, _ = C.make_inputs(1, T, 300)
    meal = np.zeros((1, T), dtype=np.float32)
    meal[0, T // 2] = height
    inp = dict(x0=x0, t=t, meal=meal, tvns=np.zeros((1, T), dtype=np.float32))
    out, _ = C.run_solve(hode, torch, inp, nn, ode, C.H0, C.L0, 0, False, rtol=C.REJECT_RTOL, atol=C.REJECT_ATOL)
    rejected = int(out["nfev"][0]) - (2 + 6 * int(out["nsteps"][0]))
    print(f"  reject candidate T={T} pulse={height}: status {out['status'].tolist()} nsteps {out['nsteps'].tolist()} nfev {out['nfev'].tolist()} -> {rejected} beyond 2 + 6 nsteps")
    if rejected > 0 and (chosen is None or (int(chosen[1]["status"][0]) != 0 and int(out["status"][0]) == 0)):
        chosen = (inp, out)
assert chosen is not None, "no candidate rejected a step"
again, _ = C.run_solve(hode, torch, chosen[0], nn, ode, C.H0, C.L0, 0, False, rtol=C.REJECT_RTOL, atol=C.REJECT_ATOL)
assert same(chosen[1], again)
save("rejected", *chosen)

# the RHS kernel on five states
x0, _, meal, tvns = C.make_inputs(5, 1, 400)
inp = dict(x=x0, t=np.linspace(0.0, 2.0, 5).astype(np.float32), meal=meal[:, 0].copy(), tvns=tvns[:, 0].copy())
out = C.run_rhs(hode, torch, inp, nn, ode)
assert same(out, C.run_rhs(hode, torch, inp, nn, ode))
save("rhs", inp, out)

# the tangent-linear pass
x0, t, meal, tvns = C.make_inputs(3, 5, 500)
g = np.random.default_rng(501)
inp = dict(x0=x0, t=t, meal=meal, tvns=tvns, v_ode=g.standard_normal((1, 2, 17)).astype(np.float32),
           v_x0=g.standard_normal((3, 2, 6)).astype(np.float32))
out = C.run_jvp(hode, torch, inp, nn, ode)
assert same(out, C.run_jvp(hode, torch, inp, nn, ode))
save("jvp", inp, out)
print("recorded into", out_dir)
