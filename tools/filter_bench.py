#!/usr/bin/env python3
"""Time the bootstrap particle filter (inference/filter.py, csrc/hode_filter.hip) at 64 patients x 1 024 particles x 241 grid
points, fp32, a 64 x 4 HybridODENN, glucose observed at every 5th grid point (48 filter steps + the initial one).

    python tools/filter_bench.py [--patients 64] [--particles 1024] [--points 241] [--every 5] [--iters 50] [--out profiles/filter_bench.json]

One JSON line:
  pf_step_us          one launch of the step kernel (device events around each of --iters launches, median), for a step that
                      resamples every patient (ess_frac 1) and for one that resamples none (ess_frac 0);
  torch_step_us       a torch composition of the same step (randn noise, the Gaussian weight, logsumexp, cumsum, searchsorted,
                      gather) with and without the resampling half: the baseline, since there was no filter before;
  run_filter_s        the whole run_filter (host clock, ends in a synchronise), and its split into the segment solves and the
                      steps (device events around every call of hode.solve_fwd / hode.capi.pf_step inside it).
Everything is warmed up once before it is timed; the profiler is off."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _events(fn, iters, before=None):
    """Median / min device time of fn() in microseconds; `before` runs untimed ahead of every call."""
    import torch
    fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    us = [1e3 * a.elapsed_time(b) for a, b in pairs]
    return {"median": statistics.median(us), "min": min(us)}


def torch_step(x, obs, sigma, q, dt, lw, resample, gen):
    """The same step composed from torch operations (fp64 weights, as the kernel's): the baseline."""
    import torch
    B, N, _ = x.shape
    s = (q * dt.sqrt().unsqueeze(1)).unsqueeze(1)                                  # [B, 1, 6]
    xd = x.double() * torch.exp(s * torch.randn(B, N, 6, dtype=torch.float64, device=x.device, generator=gen) - 0.5 * s * s)
    seen = torch.isfinite(obs).unsqueeze(1)
    z = (torch.where(seen, obs.double().unsqueeze(1), xd) - xd) / sigma
    lw = lw + torch.where(seen, -0.5 * z * z - sigma.log() - 0.9189385332046727, torch.zeros_like(z)).sum(2)
    lse = torch.logsumexp(lw, 1, keepdim=True)
    w = torch.exp(lw - lse)
    ess = 1.0 / (w * w).sum(1)
    mean = (w.unsqueeze(2) * xd).sum(1)
    var = (w.unsqueeze(2) * (xd - mean.unsqueeze(1)) ** 2).sum(1)
    if not resample:
        return xd.to(x.dtype), lw, ess, mean, var
    c = torch.cumsum(w, 1)
    u = torch.rand(B, 1, dtype=torch.float64, device=x.device, generator=gen)
    target = (torch.arange(N, device=x.device, dtype=torch.float64).unsqueeze(0) + u) / N * c[:, -1:]
    anc = torch.searchsorted(c, target).clamp_max(N - 1)
    return xd.gather(1, anc.unsqueeze(2).expand(B, N, 6)).to(x.dtype), torch.zeros_like(lw), ess, mean, var


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--points", type=int, default=241)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import hode
    import inference.filter as F
    from models.hybrid_ode_nn import HybridODENN
    hode.build_info.ensure(may_build=False)
    dev = torch.device("cuda")
    B, N, T = a.patients, a.particles, a.points
    torch.manual_seed(0)
    model = HybridODENN(nn_hidden=64, nn_layers=4, device=dev)
    with torch.no_grad():
        for p in model.nn_residual.parameters():
            p.normal_(0.0, 0.05)
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.tensor([8.0, 90.0, 80.0, 10.0, 0.0, 0.5], device=dev) * (1 + 0.1 * torch.randn(B, 6, device=dev, generator=g))
    t = torch.linspace(0.0, 4.0, T, device=dev)
    meal = torch.zeros(B, T, device=dev)
    meal[:, T // 8:T // 8 + 6] = 30.0
    with torch.no_grad():
        truth = model.forward(x0, t, {"meal": meal})
    sig = 0.02 * float(truth[..., 0].mean())
    obs = torch.full_like(truth, float("nan"))
    obs[:, ::a.every, 0] = truth[:, ::a.every, 0] + sig * torch.randn(B, len(range(0, T, a.every)), device=dev, generator=g)
    data = {"initial_state": x0, "time_points": t, "external_inputs": {"meal": meal}, "observations": obs}
    sigma = [sig, 1.0, 1.0, 1.0, 1.0, 1.0]

    # ---- the step alone, on a cloud like the filter's
    f64 = dict(dtype=torch.float64, device=dev)
    x = (x0.unsqueeze(1) * torch.exp(0.1 * torch.randn(B, N, 6, device=dev, generator=g))).contiguous()
    ob = obs[:, a.every].contiguous()
    sg, q, dt = torch.tensor(sigma, **f64), torch.full((6,), 0.05, **f64), torch.full((B,), 0.1, **f64)
    lw0 = 0.5 * torch.randn(B, N, generator=g, **f64)
    lw = lw0.clone()
    ode = torch.zeros(B, N, 17, device=dev)
    out = (torch.empty_like(x), torch.empty(B, N, dtype=torch.int32, device=dev), torch.empty(B, 16, **f64), torch.empty_like(ode))
    res = {"patients": B, "particles": N, "points": T, "dtype": "float32", "pf_step_us": {}, "torch_step_us": {}}
    for name, frac in (("resampling", 1.0), ("no_resampling", 0.0)):
        res["pf_step_us"][name] = _events(lambda: hode.capi.pf_step(x, ob, sg, q, dt, lw, 1, seed=3, link=1, ess_frac=frac, aux_in=ode, out=out),
                                          a.iters, before=lambda: lw.copy_(lw0))
        res["torch_step_us"][name] = _events(lambda: torch_step(x, ob, sg, q, dt, lw0, frac > 0, g), a.iters)

    # ---- the whole filter, split into solves and steps
    marks = []

    def timed(kind, fn):
        def wrapper(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*args, **kw)
            e.record()
            marks.append((kind, s, e))
            return r
        return wrapper
    kw = dict(n_particles=N, process_noise=0.05, noise_sigma=sigma, initial_spread=0.1, seed=0)
    F.run_filter(model, data, **kw)                                    # warm-up at the timed shapes
    torch.cuda.synchronize()
    solve_fwd, pf_step = hode.solve_fwd, hode.capi.pf_step
    hode.solve_fwd, hode.capi.pf_step = timed("solve", solve_fwd), timed("step", pf_step)
    try:
        t0 = time.perf_counter()
        r = F.run_filter(model, data, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        hode.solve_fwd, hode.capi.pf_step = solve_fwd, pf_step
    split = {k: sum(s.elapsed_time(e) for kind, s, e in marks if kind == k) / 1e3 for k in ("solve", "step")}
    res["run_filter_s"] = {"total": wall, "solves": split["solve"], "steps": split["step"], "filter_steps": len(r.step_index),
                           "resampled_share": float(r.resampled.float().mean()), "alive_min": int(r.alive.min())}
    print(json.dumps(res), flush=True)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
