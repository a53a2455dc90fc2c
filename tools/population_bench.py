#!/usr/bin/env python3
"""Time the hierarchical population sampler (inference/population.py) at the reference's MCMC workload: a 64 x 4 HybridODENN,
the 32-window x 61-point 4GI batch of tools/hmc_bench.py, the reference's seven constants per patient (K = 7, D = 238).

    python tools/population_bench.py [--chains 16 64] [--iters 5] [--leapfrog 8] [--out profiles/population_bench.json]
    python tools/population_bench.py --summarize <rocprofv3 kernel_stats.csv> [--out ...]

Per chain count, one JSON line: the time of one `evaluate()` (hode_pop_params, taped solve, per-chain cotangent, adjoint for
gode, hode_pop_grad over C x 32 trajectories, each its own parameter set), of one HMC iteration with L leapfrog steps, and -- the
same run, the same box -- of one `evaluate()` of run_hmc's sampler with sample_nn=False at the same number of trajectories (C
chains x 32 shared patients).  --summarize reads a `rocprofv3 --kernel-trace --stats` table of a run of this tool (nothing else
traced) and reports the share of GPU time spent in the two population kernels and in the sampler's other passes."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from hmc_bench import B, H, L_NN, T, batch  # noqa: E402

POP_KERNELS = ("pop_params_kernel", "pop_grad_kernel")
PASS_KERNELS = ("mse_sets_kernel", "refresh_kernel", "leapfrog_kernel", "accept_kernel", "welford_kernel")


def _time(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench(C, iters, L, data):
    import torch
    from inference.hmc import _Sampler
    from inference.population import _PopulationTarget
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN(nn_hidden=H, nn_layers=L_NN, device="cuda")
    s = _Sampler(m, data, C, seed=0, target=_PopulationTarget(data))
    s.initial_jitter()
    s.gradient()
    s.log_eps.fill_(-7.0)                  # a small step: every proposal stays where the solve is well behaved
    it = [0]

    def iteration():
        s.refresh(it[0])
        s.trajectory(L)
        s.accept(1, it[0])
        it[0] += 1
    t_eval = _time(s.evaluate, iters)
    t_iter = _time(iteration, iters)
    h = _Sampler(m, data, C, sample_nn=False, seed=0)
    h.initial_jitter()
    h.gradient()
    t_hmc = _time(h.evaluate, iters)
    return {"chains": C, "patients": B, "points": T, "K": s.target.K, "D": s.D, "trajectories": C * B, "leapfrog": L,
            "evaluate_s": t_eval, "hmc_iteration_s": t_iter, "run_hmc_evaluate_s": t_hmc, "evaluate_ratio": t_eval / t_hmc,
            "network_copies_bytes": min(C * B, 1024) * s.nn_base.numel() * s.nn_base.element_size()}


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"gpu_time_ns": tot, "kernels": {}}
    for group, names in (("population", POP_KERNELS), ("passes", PASS_KERNELS)):
        share = 0.0
        for r in rows:
            k = next((k for k in names if k in r["Name"]), None)
            if k is None:
                continue
            ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
            share += ns
            e = out["kernels"].setdefault(k, {"calls": 0, "ns": 0.0})
            e["calls"] += calls
            e["ns"] += ns
            e["avg_us"] = e["ns"] / e["calls"] / 1e3
            e["share"] = e["ns"] / tot
        out[f"{group}_kernel_share"] = share / tot
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:6]
    out["top"] = [{"name": r["Name"][:80], "share": float(r["TotalDurationNs"]) / tot} for r in top]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--leapfrog", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        r = {"kernel_trace": summarize(a.summarize)}
        print(json.dumps(r))
        if a.out:
            old = json.load(open(a.out)) if os.path.exists(a.out) else {}
            old = old if isinstance(old, dict) else {"runs": old}
            old.update(r)
            json.dump(old, open(a.out, "w"), indent=1)
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
        json.dump({"runs": res}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
