#!/usr/bin/env python3
"""Time the Sobol study at the reference's size (plots/plot_all.py:139-224: n = 1 024 base samples, D = 7 constants, second-order
design = 16 384 parameter sets x 1 patient, 61 grid points, 100 bootstrap resamples): the forward solve
(HybridODENN.forward_ode_sets) and the analysis (inference.sobol_indices -> csrc/hode_sobol.hip) separately, for the
reference's three outputs and for the time-resolved study (61 x 6 = 366 columns of the same trajectories).

    python tools/sobol_time.py [--reps 10] [--log profiles/sobol_indices.log] [--host-columns 24]

Device times are HIP events around the calls, after a warm-up call, mean of --reps.  The baseline is the numpy restatement of the
same estimators (tests/_sobol_reference.py) on the same host and the same downloaded data: SALib, which the reference calls, is
not installed, and before this kernel there was no analysis to compare with.  The restatement runs every column of the three
outputs and --host-columns live columns of the time-resolved study (its time is per column; the study has 300 live ones)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def device_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--log", default=None)
    ap.add_argument("--host-columns", type=int, default=24)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import _sobol_reference as SR
    from inference import saltelli_design, sobol_indices, sobol_study
    from inference.sobol import default_outputs

    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n, D, R = 1024, 7, 100
    m = bench.class_model(dev)
    x0, t, meal, tvns = (v.to(dev) for v in bench.sobol_inputs())
    ext = {"meal": meal, "tVNS": tvns}
    bounds = dict(zip(bench.SOBOL_NAMES, map(tuple, bench.SOBOL_BOUNDS)))
    sets = saltelli_design(bounds, n)
    ode_sets = {k: torch.as_tensor(sets[:, i], dtype=torch.float32, device=dev) for i, k in enumerate(bench.SOBOL_NAMES)}
    y = m.forward_ode_sets(ode_sets, x0, t, ext)
    out3 = default_outputs(y, t, meal)
    say(f"# {torch.cuda.get_device_name(0)}; n = {n}, D = {D}, {sets.shape[0]} sets x {y.shape[1]} points, R = {R}, reps = {a.reps}")
    say(f"forward_ode_sets                          {device_ms(lambda: m.forward_ode_sets(ode_sets, x0, t, ext), a.reps):9.3f} ms")
    say(f"three outputs (default_outputs)           {device_ms(lambda: default_outputs(y, t, meal), a.reps):9.3f} ms")
    say(f"sobol_indices, 3 columns fp64             {device_ms(lambda: sobol_indices(out3, D, num_resamples=R), a.reps):9.3f} ms")
    say(f"sobol_indices, 3 columns, R = 0           {device_ms(lambda: sobol_indices(out3, D, num_resamples=0), a.reps):9.3f} ms")
    say(f"sobol_indices, 366 columns fp32 (y)       {device_ms(lambda: sobol_indices(y, D, num_resamples=R), a.reps):9.3f} ms")
    say(f"sobol_indices, 366 columns, R = 0         {device_ms(lambda: sobol_indices(y, D, num_resamples=0), a.reps):9.3f} ms")
    t0 = time.perf_counter()
    Si = sobol_study(m, bounds, x0, t, ext, n=n, time_resolved=True, num_resamples=R)
    torch.cuda.synchronize()
    say(f"sobol_study(time_resolved=True), wall     {1e3 * (time.perf_counter() - t0):9.3f} ms   (design on the host included; n_dropped = {Si.n_dropped})")
    # the numpy restatement on the same data
    o3 = out3.cpu().numpy()
    t0 = time.perf_counter()
    want = SR.analyze(o3, D, True, R, 0)
    host3 = time.perf_counter() - t0
    say(f"numpy restatement, 3 columns              {1e3 * host3:9.1f} ms")
    yh = y.cpu().numpy().reshape(y.shape[0], -1)
    live = np.flatnonzero(yh.max(0) != yh.min(0))
    pick = live[np.linspace(0, live.size - 1, min(a.host_columns, live.size)).astype(int)]
    t0 = time.perf_counter()
    wr = SR.analyze(yh[:, pick], D, True, R, 0)
    per = (time.perf_counter() - t0) / pick.size
    say(f"numpy restatement, time-resolved          {1e3 * per:9.1f} ms per column x {live.size} live columns = {per * live.size:.1f} s")
    d3 = max(float(np.nanmax(np.abs(Si[k].cpu().numpy() - want[k]))) for k in ("S1", "ST", "S2", "S1_conf", "ST_conf", "S2_conf"))
    dr = max(float(np.nanmax(np.abs(Si.resolved[k].reshape(366, *Si.resolved[k].shape[2:])[pick].cpu().numpy() - wr[k])))
             for k in ("S1", "ST", "S2", "S1_conf", "ST_conf", "S2_conf"))
    say(f"max |kernel - restatement|                {d3:.2e} (3 outputs)  {dr:.2e} (time-resolved sample)")
    for k, name in enumerate(Si.outputs):
        say(f"S1 {name:14s} " + " ".join(f"{p}={v:+.3f}+-{c:.3f}" for p, v, c in zip(Si.names, Si.S1[k].tolist(), Si.S1_conf[k].tolist())))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
