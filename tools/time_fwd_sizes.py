#!/usr/bin/env python3
"""Forward solve (with and without the stage tape) over batch sizes, 241 grid points, fp32, benchmark cohort and weights: HIP events,
and the least-squares fit  T(B) = a + b * B / 2048  over B >= 2 048 (a = the fixed cost of a launch, b = the cost of one round of the
chip's 2 048 wave slots).  HODE_LIB=<variant .so> times an experiment build; a tag for the log line goes in argv[1]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
import hode  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else ""
SIZES = (1024, 2048, 4096, 8192, 16384)
dev = torch.device("cuda")
full = [v.to(dev) for v in bench.synth_cohort(SIZES[-1], 1000)]
nn, ode = bench.synth_weights(0).to(dev), bench.ODE_DEFAULT.to(dev)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):                      # three groups of `reps`: the median group
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) / reps)
    return float(np.median(best))


lib = os.path.basename(hode.lib_path())
plain, taped = [], []
for B in SIZES:
    x0, t, meal, tvns = full[0][:B], full[1], full[2][:B], full[3][:B]
    sol = hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, 64, 4, want_tape=True)
    reps = max(4, 32768 // B)
    plain.append(timed(lambda: hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, 64, 4), reps))
    taped.append(timed(lambda: hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, 64, 4, want_tape=True, tape=sol.tape), reps))
    del sol
for name, ms in (("forward", plain), ("forward + tape", taped)):
    r = np.array([B / 2048 for B in SIZES if B >= 2048])
    y = np.array([m for B, m in zip(SIZES, ms) if B >= 2048])
    b, a = np.polyfit(r, y, 1)
    cells = "  ".join(f"B={B}: {m:.3f}" for B, m in zip(SIZES, ms))
    print(f"{tag:>10s} {lib:>24s} {name:>14s} ms  {cells}  | fit a={a:.3f} ms  b={b:.3f} ms/round")
