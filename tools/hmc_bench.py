#!/usr/bin/env python3
"""Time one multi-chain HMC sampling iteration (inference/hmc.py) at the reference's MCMC workload: a 64 x 4 HybridODENN,
a 32-window x 61-point 4GI batch, L leapfrog steps, the reference's seven constants + every MLP weight sampled.

    python tools/hmc_bench.py [--chains 64 256 1024] [--iters 5] [--leapfrog 16] [--out profiles/hmc_bench.json]
    python tools/hmc_bench.py --summarize <rocprofv3 kernel_stats.csv> --chains 256 --iters 3 --leapfrog 16

Prints one JSON line per chain count: seconds per iteration, gradient evaluations / s (C x L per iteration) and
chain-iterations / s.  --summarize reads a `rocprofv3 --kernel-trace --stats` table of a run of this tool and reports the
share of GPU time spent in the sampler's own kernels (csrc/hode_hmc.hip) and, per kernel, bytes moved / time against the
~6.3 TB/s achievable HBM rate (bytes: the arrays each pass must read and write, counted from the shapes)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, L_NN, B, T = 64, 4, 32, 61
HBM = 6.3e12


def batch(dev):
    import torch
    from hode.datagen import FourGIModel, GlucoseDataset
    gen = torch.Generator(device=dev).manual_seed(0)
    table, _ = FourGIModel("T2DM").generate_cohort(B, duration_hours=5, sampling_interval_min=5, meal_times=(0.5, 2.5),
                                                   meal_sizes=(75, 50), noise_cv=0.1, generator=gen)
    return GlucoseDataset(table, sequence_length=T, stride=T).batch(torch.arange(B))


def bench(C, iters, L, data):
    import torch
    from inference.hmc import _Sampler
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN(nn_hidden=H, nn_layers=L_NN, device="cuda")
    s = _Sampler(m, data, C, seed=0)
    s.initial_jitter()
    s.gradient()
    s.log_eps.fill_(-7.0)                  # a small step: every proposal stays where the solve is well behaved
    s.refresh(0)
    s.trajectory(L)
    s.accept(1, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, iters + 1):
        s.refresh(it)
        s.trajectory(L)
        s.accept(1, it)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return {"chains": C, "D": s.D, "leapfrog": L, "windows": B, "points": T, "s_per_iter": dt, "grad_evals_per_s": C * L / dt,
            "chain_iters_per_s": C / dt}


KERNELS = ("mse_sets_kernel", "refresh_kernel", "leapfrog_kernel", "accept_kernel", "welford_kernel")


def bytes_per_call(kernel, C, D, L, elem=4):
    """Bytes a call must move (the shapes of the passes; minv and other [D] vectors are cached and not counted)."""
    n = C * D * elem
    if kernel == "mse_sets_kernel":
        return 3 * C * B * T * 6 * elem - B * T * 6 * elem * (C - 1)       # y, gy per set; obs once
    if kernel == "refresh_kernel":
        return 5 * n                                                       # z, g in; p, z0, g0 out
    if kernel == "leapfrog_kernel":
        # per trajectory: 1 x (z, g, p in; p, z, nn_p out) + (L-1) x (z, gnn, p in; g, p, z, nn_p out) + 1 x (z, gnn, g, p in; g, p out)
        per = (6 * n + (L - 1) * 7 * n + 6 * n) / (L + 1)
        return int(per)
    if kernel == "accept_kernel":
        return 4 * n                                                       # reject: z0, g0 in, z, g out (upper bound)
    return C * D * elem


def summarize(path, C, iters, L):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"chains": C, "iters": iters, "leapfrog": L, "gpu_time_ns": tot, "kernels": {}}
    own = 0.0
    D = 7 + 13510
    for r in rows:
        name = r["Name"]
        k = next((k for k in KERNELS if k in name), None)
        if k is None:
            continue
        ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
        own += ns
        by = bytes_per_call(k, C, D, L)
        avg = ns / calls
        e = out["kernels"].setdefault(k, {"calls": 0, "ns": 0.0})
        e["calls"] += calls
        e["ns"] += ns
        e["avg_us"] = e["ns"] / e["calls"] / 1e3
        e["bytes_per_call"] = by
        e["TB_per_s"] = by / (e["ns"] / e["calls"]) / 1e3
        e["fraction_of_hbm"] = e["TB_per_s"] * 1e12 / HBM
    out["sampler_kernel_share"] = own / tot
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:6]
    out["top"] = [{"name": r["Name"][:80], "share": float(r["TotalDurationNs"]) / tot} for r in top]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--leapfrog", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        r = summarize(a.summarize, a.chains[0], a.iters, a.leapfrog)
        print(json.dumps(r))
        if a.out:
            json.dump(r, open(a.out, "w"), indent=1)
        return
    import torch
    import hode
    hode.build_info.ensure(may_build=False)
    data = batch(torch.device("cuda"))
    res = []
    for C in a.chains:
        r = bench(C, a.iters, a.leapfrog, data)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
