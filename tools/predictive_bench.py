#!/usr/bin/env python3
"""Time the posterior-predictive fold and score kernels (csrc/hode_predictive.hip) against the same summary computed with
torch from the materialised [draws, N] block, as `VariationalInference.posterior_predictive` does it (mean(0), std(0)) plus the
CDF mean and the metric sums.

    python tools/predictive_bench.py [--reps 20] [--piece 64] [--out profiles/predictive_fold.json]

Workloads, fp32: 256 draws x 64 windows x 61 points and 1 024 draws x 64 windows x 241 points (x 6 states).  Times are HIP
events around each call, the two routes alternating, after warm-up.  Bytes the fold MUST move: the draws once (S N 4) plus the
state read and written once per call (44 N each way) plus obs (4 N); `hbm_fraction` is that over the time over 6.3 TB/s, the
achievable HBM rate.  Peak memory: torch's allocator high-water mark of each route -- the fold route holds ONE piece of
`--piece` draws and the state, the torch route the whole block and its temporaries."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM = 6.3e12
WORKLOADS = ((256, 64, 61), (1024, 64, 241))


def timed(fns, reps):
    """Median / min milliseconds per call of each fn, the fns alternating call by call."""
    import torch
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for i in range(reps):
        for k, f in fns.items():
            ev[k][i][0].record()
            f()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        t = sorted(a.elapsed_time(b) for a, b in ev[k])
        out[k] = {"median_ms": t[len(t) // 2], "min_ms": t[0]}
    return out


def torch_summary(y, obs, sigma, thr):
    """The parent commit's route on the materialised block: several passes over y."""
    import torch
    S, N = y.shape
    mean, sd = y.mean(0), y.std(0)
    sig = sigma.float().view(S, 1, 6) * math.sqrt(2.0)
    pit = (0.5 * torch.erfc(-(obs.view(-1, 6) - y.view(S, -1, 6)) / sig)).mean(0).reshape(-1)
    sd = torch.sqrt(sd * sd + (sigma.float() ** 2).mean(0).repeat(N // 6))
    e = (mean - obs).double().view(-1, 6)
    s6, o6 = sd.double().view(-1, 6), obs.double().view(-1, 6)
    ne = e.abs() / (s6 + 1e-6)
    lo, hi = (mean.double().view(-1, 6) - 1.96 * s6), (mean.double().view(-1, 6) + 1.96 * s6)
    pen = 40.0 * ((lo - o6).clamp(min=0) + (o6 - hi).clamp(min=0))
    cols = [(e * e).sum(0), e.abs().sum(0), s6.sum(0), ne.sum(0), ((hi - lo) + pen).sum(0), ((o6 >= lo) & (o6 <= hi)).double().sum(0)]
    cols += [(ne <= t).double().sum(0) for t in thr]
    return mean, sd, pit, torch.stack(cols, 1)


def workload(S, B, T, reps, piece):
    import torch
    import hode
    cap = hode.capi
    dev = torch.device("cuda")
    N = B * T * 6
    g = torch.Generator(device=dev).manual_seed(0)
    scale = torch.tensor([120.0, 15.0, 60.0, 8.0, 0.5, 0.4], device=dev).repeat(N // 6)
    obs = scale * (1 + 0.05 * torch.randn(N, device=dev, generator=g))
    sigma = (0.05 * scale[:6].double() * (0.5 + torch.rand(S, 6, device=dev, generator=g, dtype=torch.float64))).contiguous()
    from inference.predictive import half_normal_thresholds
    thr = half_normal_thresholds(10)
    out = {"draws": S, "windows": B, "points": T, "N": N, "block_bytes": S * N * 4}

    # ---- the fold route, memory: one piece of draws + the state
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yp = scale * (1 + 0.05 * torch.randn(piece, N, device=dev, generator=g))
    st = cap.pred_state(N, dev)
    for lo in range(0, S, piece):
        cap.pred_fold(yp[:min(piece, S - lo)], st, obs, None, sigma[lo:lo + piece], None)
    res = cap.pred_score(st, torch.float32, obs, None, (sigma ** 2).mean(0).tolist(), thr)
    torch.cuda.synchronize()
    out["fold_route_peak_bytes"] = torch.cuda.max_memory_allocated() - base
    del yp, res

    # ---- the torch route, memory: the block + temporaries
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = scale * (1 + 0.05 * torch.randn(S, N, device=dev, generator=g))
    ref = torch_summary(y, obs, sigma, thr)
    torch.cuda.synchronize()
    out["torch_route_peak_bytes"] = torch.cuda.max_memory_allocated() - base

    # ---- agreement of the two routes on the same block (fp32 torch sums against the fp64 fold)
    st = cap.pred_state(N, dev)
    cap.pred_fold(y, st, obs, None, sigma, None)
    mean, sd, pit, table = cap.pred_score(st, torch.float32, obs, None, (sigma ** 2).mean(0).tolist(), thr)
    rel = lambda a, b: float(((a - b).abs() / (b.abs() + 1e-30)).max())                             # noqa: E731
    out["max_rel_diff_vs_torch"] = {"mean": rel(ref[0], mean), "sd": rel(ref[1], sd), "pit_abs": float((ref[2] - pit).abs().max()),
                                    "sum_sq_err": rel(ref[3][:, 0], table[:, 1])}
    del ref

    states = {k: cap.pred_state(N, dev) for k in ("noise", "plain", "pieces")}
    ev = (sigma ** 2).mean(0).tolist()

    def pieces():
        for lo in range(0, S, piece):
            cap.pred_fold(y[lo:lo + piece], states["pieces"], obs, None, sigma[lo:lo + piece], None)
    fns = {"fold_noise": lambda: cap.pred_fold(y, states["noise"], obs, None, sigma, None),
           "fold_plain": lambda: cap.pred_fold(y, states["plain"], obs, None, None, None),
           f"fold_noise_in_pieces_of_{piece}": pieces,
           "score": lambda: cap.pred_score(st, torch.float32, obs, None, ev, thr),
           "torch_from_block": lambda: torch_summary(y, obs, sigma, thr)}
    r = timed(fns, reps)
    n_calls = {k: 1 for k in fns}
    n_calls[f"fold_noise_in_pieces_of_{piece}"] = -(-S // piece)
    for k in r:
        if k.startswith("fold"):
            byt = S * N * 4 + n_calls[k] * (2 * 44 * N + 4 * N)
            r[k]["bytes"] = byt
            r[k]["tb_per_s"] = byt / (r[k]["median_ms"] * 1e-3) / 1e12
            r[k]["hbm_fraction"] = byt / (r[k]["median_ms"] * 1e-3) / HBM
    r["torch_from_block"]["ratio_to_fold_noise_plus_score"] = r["torch_from_block"]["median_ms"] / (r["fold_noise"]["median_ms"] + r["score"]["median_ms"])
    out["timings"] = r
    out["workgroups_of_the_fold"] = -(-N // 256)                              # one entry per lane, 256 lanes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--piece", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("predictive_bench.py needs the GPU: it measures, it does not estimate")
    rows = [workload(S, B, T, a.reps, a.piece) for S, B, T in WORKLOADS]
    out = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps, "workloads": rows}
    for row in rows:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
