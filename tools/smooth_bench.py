#!/usr/bin/env python3
"""Time backward-simulation smoothing (FilterResult.smooth, csrc/hode_smooth.hip) over the stored filter of tools/filter_bench.py:
64 patients x 1 024 particles x 1 024 trajectories x the 49 stored steps (241 grid points, glucose observed at every 5th), fp32,
a 64 x 4 HybridODENN.  (The initial gastric state is 0.3, not the filter benchmark's 0: under the log link a state at exactly 0
has no transition density, and every trajectory would be lost at the first steps.)

    python tools/smooth_bench.py [--patients 64] [--particles 1024] [--trajectories 1024] [--points 241] [--every 5] [--iters 20]
                                 [--out profiles/smooth_bench.json]

One JSON line:
  pf_smooth_ms        the ONE launch of the whole backward pass (device events around each of --iters launches after a warm-up,
                      median and minimum), and the peak device memory the call adds (its two outputs);
  torch_smooth_ms     the same pass composed from torch operations, per step the [B, M, N] fp64 logits, logsumexp, cumsum,
                      searchsorted, gather (torch.rand for the uniforms): the yardstick, since there was no smoother before;
                      its time (events around the whole pass, median of --torch-iters) and the peak memory it adds;
  ratio               torch / kernel;  lost: trajectories without a candidate alive;  distinct_step0: the median over the
                      patients of the distinct step-0 slots among the trajectories, next to the genealogy trace's.
The profiler is off."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_smooth(hist, lwh, pred, q, dt, M, gen):
    """The backward pass composed from torch operations (log link, fp64 logits as the kernel's) -> idx [S, B, M]."""
    import torch
    S, B, N, _ = hist.shape
    dev = hist.device
    rows = torch.arange(B, device=dev).unsqueeze(1)
    out = torch.empty(S, B, M, dtype=torch.int64, device=dev)

    def draw(logits):                                              # [B, M, N] -> [B, M]
        w = torch.exp(logits - torch.logsumexp(logits, 2, keepdim=True))
        c = torch.cumsum(w, 2)
        u = torch.rand(B, M, 1, dtype=torch.float64, device=dev, generator=gen)
        return torch.searchsorted(c, u * c[..., -1:]).clamp_max(N - 1).squeeze(2)
    k = draw(lwh[S - 1].unsqueeze(1).expand(B, M, N))
    out[S - 1] = k
    for s in range(S - 2, -1, -1):
        sg = q * dt[s + 1].sqrt().unsqueeze(1)                                          # [B, 6]
        a = torch.log(hist[s + 1].double()[rows, k])                                    # [B, M, 6]: the gather
        c = torch.log(pred[s + 1].double()) - 0.5 * (sg * sg).unsqueeze(1)              # [B, N, 6]
        logits = lwh[s].unsqueeze(1).expand(B, M, N).clone()
        for j in range(6):
            z = (a[:, :, j].unsqueeze(2) - c[:, :, j].unsqueeze(1)) / sg[:, j].reshape(B, 1, 1)
            logits -= 0.5 * z * z
        k = draw(torch.nan_to_num(logits, nan=float("-inf")))
        out[s] = k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1024)
    ap.add_argument("--trajectories", type=int, default=1024)
    ap.add_argument("--points", type=int, default=241)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import hode
    import inference.filter as F
    from models.hybrid_ode_nn import HybridODENN
    hode.build_info.ensure(may_build=False)
    dev = torch.device("cuda")
    B, N, M, T = a.patients, a.particles, a.trajectories, a.points
    torch.manual_seed(0)
    model = HybridODENN(nn_hidden=64, nn_layers=4, device=dev)
    with torch.no_grad():
        for p in model.nn_residual.parameters():
            p.normal_(0.0, 0.05)
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.tensor([8.0, 90.0, 80.0, 10.0, 0.3, 0.5], device=dev) * (1 + 0.1 * torch.randn(B, 6, device=dev, generator=g))
    t = torch.linspace(0.0, 4.0, T, device=dev)
    meal = torch.zeros(B, T, device=dev)
    meal[:, T // 8:T // 8 + 6] = 30.0
    with torch.no_grad():
        truth = model.forward(x0, t, {"meal": meal})
    sig = 0.02 * float(truth[..., 0].mean())
    obs = torch.full_like(truth, float("nan"))
    obs[:, ::a.every, 0] = truth[:, ::a.every, 0] + sig * torch.randn(B, len(range(0, T, a.every)), device=dev, generator=g)
    data = {"initial_state": x0, "time_points": t, "external_inputs": {"meal": meal}, "observations": obs}
    r = F.run_filter(model, data, n_particles=N, process_noise=0.05, noise_sigma=[sig, 1.0, 1.0, 1.0, 1.0, 1.0], initial_spread=0.1, seed=0,
                     store_particles=True)
    S = len(r.step_index)
    q = torch.full((6,), 0.05, dtype=torch.float64, device=dev)
    args = (r.history, r.log_weight_history, r.predicted, q, r.step_dt)
    res = {"patients": B, "particles": N, "trajectories": M, "steps": S, "dtype": "float32", "pairs": B * M * N * S}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    # ---- the kernel: one launch
    (idx, paths), mib = peak(lambda: hode.capi.pf_smooth(*args, M, seed=0, link=1))
    out = (idx, paths)
    pairs = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hode.capi.pf_smooth(*args, M, seed=0, link=1, out=out)
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in pairs]
    res["pf_smooth_ms"] = {"median": statistics.median(ms), "min": min(ms), "peak_mib": mib}
    sm = r.smooth(n_trajectories=M)
    anc = torch.arange(N, device=dev).expand(B, N)
    for s in range(S - 1, 0, -1):
        anc = r.ancestors[s].long().gather(1, anc)
    res["lost"] = int(sm.lost.sum())
    res["distinct_step0"] = {"backward_simulation": float(sm.distinct()[:, 0].double().median()),
                             "genealogy": statistics.median(len(set(row.tolist())) for row in anc)}
    del sm, idx, paths, out

    # ---- the torch composition
    _, mib = peak(lambda: torch_smooth(*args, M, g))
    ms = []
    for _ in range(a.torch_iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_smooth(*args, M, g)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    res["torch_smooth_ms"] = {"median": statistics.median(ms), "min": min(ms), "peak_mib": mib}
    res["ratio"] = res["torch_smooth_ms"]["median"] / res["pf_smooth_ms"]["median"]
    print(json.dumps(res), flush=True)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
