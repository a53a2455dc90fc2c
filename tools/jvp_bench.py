#!/usr/bin/env python3
"""Time the tangent-linear solve (hode.solve_jvp, csrc/hode_solve_jvp.hip) on the benchmark's flagship cohort -- 4 096 patients
x 241 grid points, DP5(4) 1e-6 / 1e-8, a 64 x 4 MLP, fp32 (bench.py's synth_cohort / synth_weights) -- against the forward
solve with and without a tape, and one Levenberg-Marquardt iteration of inference.fit_patients for 4 096 patients x the
reference's seven constants.

    python tools/jvp_bench.py [--K 1 4 7 16] [--reps 5] [--out profiles/jvp_bench.json]
    python tools/jvp_bench.py --hidden 128 --layers 5 [--batch 1024 --points 61]      -> profiles/jvp_generic_bench.json

With --hidden / --layers outside the tuned envelope (64 x 4) the same measurements are taken on a GENERIC network
(csrc/hode_generic_jvp.hip): the cohort and weights of tools/time_generic.py (the first `points` grid points of synth_cohort, a
gain-0.5 network), the LM iteration with `batch` patients.  Without them nothing changes: the recorded profiles/jvp_bench.json recipe.

The JVP's arithmetic per direction, counted from the shapes: every taped stage is one tangent through the network (first layer
6 inputs, L-1 hidden matrices, the output layer: 2 (6 H + (L-1) H^2 + 6 H) FLOP) plus ~40 FLOP of mechanistic terms and
stage combination; its fraction of the fp32 vector peak (157.3 TFLOP/s, /opt guides: MI355X spec) is that count over the
kernel time.  Times are host clocks around work that ends in a device synchronise, after warm-up."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, H, L = 4096, 64, 4                    # the defaults: the benchmark's flagship cohort and network
PEAK_FP32 = 157.3e12


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    global B, H, L
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=H)
    ap.add_argument("--layers", type=int, default=L)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 4, 7, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    generic = (args.hidden, args.layers) != (H, L)
    H, L = args.hidden, args.layers
    B = args.batch if args.batch is not None else (1024 if generic else B)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jvp_generic_bench.json" if generic else "jvp_bench.json")
    import torch
    import bench
    import hode
    dev = torch.device("cuda")
    x0, t, meal, tvns = (v.to(dev) for v in bench.synth_cohort(B, seed=0))
    nn = bench.synth_weights(0).to(dev)
    if generic:                                   # tools/time_generic.py's network
        g = torch.Generator().manual_seed(H + L)
        nn = (torch.randn(hode.n_params(H, L), generator=g) * (0.5 * (2.0 / (2 * H)) ** 0.5)).to(dev)
        nn[-(6 * H + 6):] *= 0.1
    ode = bench.ODE_DEFAULT.to(dev)
    if args.points is not None or generic:
        T = args.points if args.points is not None else 61
        t, meal, tvns = t[:T].contiguous(), meal[:, :T].contiguous(), tvns[:, :T].contiguous()
    T = t.shape[0]
    plain = timed(lambda: hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, H, L), args.reps)
    sol = hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, H, L, want_tape=True)
    taped = timed(lambda: hode.solve_fwd(x0, t, meal, tvns, None, ode, nn, H, L, tape=sol.tape), args.reps)
    assert int(sol.status.max()) == 0
    steps = int(sol.nsteps.sum())
    flop_dir = steps * 6 * (2 * (6 * H + (L - 1) * H * H + 6 * H) + 40)
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for K in args.K:
        v_ode = torch.randn(1, K, 17, device=dev, generator=g) * ode.abs()
        v_x0 = torch.randn(B, K, 6, device=dev, generator=g)
        s = timed(lambda: hode.solve_jvp(sol, v_ode, v_x0), args.reps)
        rows.append({"K": K, "jvp_ms": s * 1e3, "ms_per_direction": s * 1e3 / K, "bar_ms": K * plain * 1e3,
                     "vs_bar": s / (K * plain), "fp32_peak_fraction": K * flop_dir / s / PEAK_FP32})
        print(json.dumps(rows[-1]), flush=True)
    # one LM iteration at B (4 096) patients x 7 constants (max_iter = 1: taped solve + JVP, trial solve, taped solve + JVP)
    from inference import fit_patients
    from models.hybrid_ode_nn import HybridODENN
    m = HybridODENN(nn_hidden=H, nn_layers=L)
    with torch.no_grad():
        off = 0
        for p in m.nn_residual.parameters():
            p.copy_(nn[off:off + p.numel()].view_as(p).cpu())
            off += p.numel()
    obs = sol.y.detach() + 0.1 * torch.randn(sol.y.shape, device=dev, generator=g)          # glucose-only noisy records
    obs[:, :, 1:] = float("nan")
    batch = {"initial_state": x0, "time_points": t, "observations": obs, "external_inputs": {"meal": meal, "tVNS": tvns}}
    lm = {}
    for dt in (torch.float32, torch.float64):
        one = timed(lambda: fit_patients(m, batch, max_iter=1, dtype=dt), 2)
        zero = timed(lambda: fit_patients(m, batch, max_iter=0, dtype=dt), 2)
        lm[str(dt).replace("torch.", "")] = {"lm_iteration_ms": (one - zero) * 1e3, "fit_max_iter_1_ms": one * 1e3}
    out = {"workload": f"{B} patients x {T} points, DP5(4) 1e-6/1e-8, MLP {H}x{L}, fp32 (bench.py synth_cohort / "
                       f"{'tools/time_generic.py weights' if generic else 'synth_weights'})",
           "accepted_steps": steps, "fwd_plain_ms": plain * 1e3, "fwd_tape_ms": taped * 1e3, "jvp": rows,
           f"lm_iteration_{B}x7": lm, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if generic:                                   # one file for every (shape, batch) measured: runs add their entry
        try:
            with open(args.out) as f:
                runs = json.load(f)
        except (OSError, ValueError):
            runs = {}
        runs[f"{H}x{L}_B{B}_T{T}"] = out
        out = runs
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
