#!/usr/bin/env python3
"""Time the observation model's kernel (csrc/hode_obs.hip) against hode_mse_sets at the samplers' workload of
tools/hmc_bench.py (C parameter sets of 32 windows x 61 points x 6 states, fp32), and the cost of the forward-only pre-pass
the marginal mode needs when a set is cut into tape-budget pieces.

    python tools/obs_bench.py [--sets 64 256] [--calls 400] [--baseline-lib <libhode.so of the parent commit>] [--out profiles/obs_bench.json]
    python tools/obs_bench.py --nuts-iters 6          (a few run_nuts iterations in marginal mode: run it under rocprofv3 --kernel-trace --stats)
    python tools/obs_bench.py --summarize <rocprofv3 kernel_stats.csv>

The yardstick hode_mse_sets is timed in the same process, the calls of the kernels alternating; with --baseline-lib it is the
one of that library (ctypes), else this tree's (csrc/hode_hmc.hip).  Bytes: hode_mse_sets reads y and obs once and writes gy
once; hode_obs_nll_sets reads y and obs (and the mask) twice and writes gy once."""
import argparse
import csv
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, T = 32, 61
LEN = B * T * 6


def timed(fns, calls):
    """Mean microseconds per call of each fn, the fns alternating call by call (device events around each call)."""
    import torch
    for f in fns.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for k in fns}
    for i in range(calls):
        for k, f in fns.items():
            ev[k][i][0].record()
            f()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[k])
        out[k] = {"mean_us": sum(t) / len(t), "median_us": t[len(t) // 2], "min_us": t[0]}
    return out


def kernels(n_sets, calls, baseline):
    import numpy as np
    import torch
    import hode
    cap = hode.capi
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randn(n_sets, LEN, device=dev, generator=g)
    obs = torch.randn(LEN, device=dev, generator=g)
    miss = obs.clone()
    miss[torch.rand(LEN, device=dev, generator=g) < 0.3] = float("nan")
    mask = torch.isfinite(miss).to(torch.uint8)
    n = mask.view(-1, 6).sum(0).double().cpu().numpy()
    ls = torch.zeros(n_sets, dtype=torch.float64, device=dev)
    sse = torch.zeros(n_sets, 6, dtype=torch.float64, device=dev)
    gy = torch.empty_like(y)
    one, two = np.ones(6), np.full(6, 2.0)
    lib = C.CDLL(baseline) if baseline else hode.load()
    six = lambda v: (C.c_double * 6)(*v)                                       # noqa: E731
    P = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    new = hode.load()
    w6, a6, b6, n6, n6c = six(one), six(two), six(one), six(n), six(np.full(6, LEN / 6))

    def obs_call(o, m, mode, flags=0):
        return lambda: new.hode_obs_nll_sets_f32(st, n_sets, C.c_int64(LEN), P(y), P(o), P(m) if m is not None else None, mode, flags,
                                                 w6 if mode == 0 else None, a6 if mode else None, b6 if mode else None,
                                                 (n6 if m is not None else n6c) if mode else None, P(sse), P(ls), P(gy))
    fns = {"mse_sets": lambda: lib.hode_mse_sets_f32(st, n_sets, C.c_int64(LEN), P(y), P(obs), C.c_float(0.5), P(ls), P(gy)),
           "obs_fixed_complete": obs_call(obs, None, cap.OBS_FIXED),
           "obs_fixed_masked": obs_call(miss, mask, cap.OBS_FIXED),
           "obs_marginal_complete": obs_call(obs, None, cap.OBS_MARGINAL),
           "obs_marginal_masked": obs_call(miss, mask, cap.OBS_MARGINAL),
           "obs_sums_only_masked": obs_call(miss, mask, cap.OBS_MARGINAL, cap.OBS_SUMS_ONLY)}
    r = timed(fns, calls)
    byt = {"mse_sets": 4 * (2 * n_sets * LEN + LEN)}
    for k in fns:
        if k.startswith("obs"):
            sweeps = 1 if "sums_only" in k else 2
            byt[k] = sweeps * (4 * n_sets * LEN + 4 * LEN + (LEN if "masked" in k else 0)) + (0 if sweeps == 1 else 4 * n_sets * LEN)
    for k in r:
        r[k]["bytes"] = byt[k]
        r[k]["gb_per_s"] = byt[k] / r[k]["median_us"] / 1e3
        r[k]["ratio_to_mse_sets"] = r[k]["median_us"] / r["mse_sets"]["median_us"]
    return {"sets": n_sets, "len": LEN, "calls": calls, "baseline": "parent library" if baseline else "this tree's hode_mse_sets", "kernels": r}


def sampler(C_, marginal=True):
    import torch
    from hmc_bench import H, L_NN, batch
    from inference.hmc import _Sampler
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN(nn_hidden=H, nn_layers=L_NN, device="cuda")
    data = batch(torch.device("cuda"))
    data = dict(data, observations=data["observations"].clone())
    data["observations"][..., 1:] = float("nan")                              # glucose only
    s = _Sampler(m, data, C_, seed=0, noise="marginal" if marginal else "fixed")
    s.initial_jitter()
    s.gradient()
    return s


def prepass(C_, reps, marginal=True):
    """Seconds per evaluation (solve + likelihood + adjoint of C x 32 trajectories): whole sets, and with the tape budget
    forced below one set (16 of its 32 trajectories per piece).  Marginal mode then runs the forward-only pre-pass before the
    taped pass; fixed mode (marginal=False) runs the taped pieces alone: the difference between the two is the pre-pass."""
    import time
    import torch
    import hode
    import models.hybrid_ode_nn as HN
    s = sampler(C_, marginal)

    def run():
        s.evaluate()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            s.evaluate()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    whole = run()
    U0 = s.loss_sum.clone()
    elem = s.x0.element_size()
    steps = HN._small_tape_steps(s.C * s.N, s.T, s.method, elem, s.L, s.H, None) or HN._tape_steps(s.T, s.method, None)
    keep = HN.TAPE_BUDGET_BYTES
    HN.TAPE_BUDGET_BYTES = 16 * hode.capi.tape_nbytes(1, steps, elem, s.L, s.H)
    try:
        cut = run()
    finally:
        HN.TAPE_BUDGET_BYTES = keep
    return {"sets": C_, "noise": "marginal" if marginal else "fixed", "s_per_eval_whole_sets": whole, "s_per_eval_cut_sets": cut, "ratio": cut / whole,
            "nll_rel_diff": float(((s.loss_sum - U0).abs() / U0.abs()).max())}


def nuts(iters):
    import torch
    from hmc_bench import H, L_NN, batch
    from inference.nuts import run_nuts
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN(nn_hidden=H, nn_layers=L_NN, device="cuda")
    data = batch(torch.device("cuda"))
    data = dict(data, observations=data["observations"].clone())
    data["observations"][..., 1:] = float("nan")
    r = run_nuts(m, data, iters, iters, 0.8, 5, None, n_chains=64, seed=0, noise="marginal")
    torch.cuda.synchronize()
    print(json.dumps({"nuts_iters": 2 * iters, "chains": 64, "mean_leapfrog": float(r.stats["n_leapfrog"].mean())}))


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    name = lambda r: r.get("Name") or r.get("KernelName") or ""                # noqa: E731
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = [r for r in rows if "obs_nll_sets_kernel" in name(r)]
    t = sum(float(r["TotalDurationNs"]) for r in mine)
    return {"gpu_time_ns": tot, "obs_nll_sets_ns": t, "obs_nll_sets_calls": sum(int(r["Calls"]) for r in mine), "share": t / tot}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nuts-iters", type=int, default=0)
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        print(json.dumps(summarize(a.summarize)))
        return
    if a.nuts_iters:
        nuts(a.nuts_iters)
        return
    out = {"kernel": [kernels(c, a.calls, a.baseline_lib) for c in a.sets], "prepass": [prepass(64, 5, True), prepass(64, 5, False)]}
    for row in out["kernel"] + out["prepass"]:
        print(json.dumps(row))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
