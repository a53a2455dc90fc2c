#!/usr/bin/env python3
"""Time the tail and quantile kernels (csrc/hode_predictive.hip, "Posterior bands") against the same quantiles computed with
torch from the held [draws, N] block: torch.sort(dim=0), two rows gathered per level, a lerp (torch.quantile refuses more than
16 M elements).

    python tools/quantile_bench.py [--reps 20] [--out profiles/predictive_tails.json]

Workloads, fp32, levels (0.025, 0.975): those of tools/predictive_bench.py, 256 draws x 64 windows x 61 points and 1 024 draws
x 64 windows x 241 points (x 6 states), the draws taken whole and in 16 pieces.  Times are HIP events around each call, the
routes alternating, after warm-up; the fold without observation noise is timed in the same run: it reads each draw once and
is the floor of any route that does.  Peak memory is torch's allocator high-water mark of each route.  The kernel route's peak
is CHECKED, not just recorded: one piece of draws + (2 K + 1) N values of state + the outputs, each tensor rounded up as torch's
caching allocator rounds it (to 512 bytes; a tensor of 1 MiB or more may keep the rest of its 2 MiB-granular block).  The inserts per entry and tail, and the share of (wave, draw) pairs in which at least one lane
walks a heap, are counted on the host for the first 256 entries."""
import argparse
import heapq
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = ((256, 64, 61), (1024, 64, 241))
LEVELS = (0.025, 0.975)
PIECES = 16


def allocator_size(b):
    """What torch's caching allocator may account for a tensor of b bytes: multiples of 512 bytes below 1 MiB; from there the
    blocks are cut from 2 MiB-granular segments and a remainder under 1 MiB is not split off."""
    return -(-b // 512) * 512 if b < (1 << 20) else -(-b // (2 << 20)) * (2 << 20)


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


def fill(y, scale, g):
    """y <- scale (1 + 0.05 randn), in place: no temporary of y's size."""
    return y.normal_(generator=g).mul_(0.05).add_(1.0).mul_(scale)


def torch_quantiles(y, levels):
    """The route on the held block: a full sort along the draws, then numpy's "linear" interpolation."""
    import torch
    S = y.shape[0]
    srt = torch.sort(y, dim=0).values
    out = []
    for q in levels:
        h = q * (S - 1)
        j = int(math.floor(h))
        a, b = srt[j], srt[min(j + 1, S - 1)]
        out.append(a + (b - a) * (h - j))
    return torch.stack(out)


def count_inserts(y, K):
    """Host count over the columns of y [S, n]: inserts per entry into the lower buffer after it is full, the same for the
    upper one, and the share of (wave of 64 entries, draw) pairs in which at least one lane inserts into either."""
    S, n = y.shape
    hit = [[False] * S for _ in range(n)]
    lo_ins = hi_ins = 0
    for i in range(n):
        lo, hi = [], []                                # heapq min-heaps: lo holds negated values
        for s in range(S):
            v = float(y[s, i])
            if s < K:
                heapq.heappush(lo, -v)
                heapq.heappush(hi, v)
                hit[i][s] = True
                continue
            if v < -lo[0]:
                heapq.heapreplace(lo, -v)
                lo_ins += 1
                hit[i][s] = True
            if hi[0] < v:
                heapq.heapreplace(hi, v)
                hi_ins += 1
                hit[i][s] = True
    waves = [range(w, min(w + 64, n)) for w in range(0, n, 64)]
    busy = sum(any(hit[i][s] for i in w) for w in waves for s in range(S))
    lane_busy = sum(sum(r) for r in hit)
    return {"entries_counted": n, "inserts_per_entry_lower_incl_fill": lo_ins / n + K, "inserts_per_entry_upper_incl_fill": hi_ins / n + K,
            "expected_K_1_plus_ln_S_over_K": K * (1.0 + math.log(S / K)),
            "share_of_wave_draws_with_an_insert": busy / (len(waves) * S), "share_of_lane_draws_with_an_insert": lane_busy / (n * S)}


def workload(S, B, T, reps):
    import torch
    import hode
    from inference.predictive import tail_size
    cap = hode.capi
    dev = torch.device("cuda")
    N = B * T * 6
    K = tail_size(LEVELS, S)
    piece = -(-S // PIECES)
    g = torch.Generator(device=dev).manual_seed(0)
    scale = torch.tensor([120.0, 15.0, 60.0, 8.0, 0.5, 0.4], device=dev).repeat(N // 6)
    out = {"draws": S, "windows": B, "points": T, "N": N, "K": K, "levels": list(LEVELS), "piece": piece, "block_bytes": S * N * 4}

    # ---- the kernel route, memory: one piece of draws + the tail state + the quantiles
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yp = torch.empty(piece, N, device=dev)
    ts = cap.pred_tail_state(N, K, torch.float32, dev)
    for lo in range(0, S, piece):
        n = min(piece, S - lo)
        fill(yp[:n], scale, g)
        cap.pred_tails(yp[:n], ts)
    res, _ = cap.pred_quantiles(ts, LEVELS)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    up = allocator_size
    bound = up(piece * N * 4) + up(4 * N) + 2 * up(K * N * 4) + up(len(LEVELS) * N * 4)
    out["kernel_route_peak_bytes"], out["kernel_route_peak_bound_bytes"] = peak, bound
    out["kernel_route_tensor_bytes"] = piece * N * 4 + (2 * K + 1) * N * 4 + len(LEVELS) * N * 4
    assert peak <= bound, f"the kernel route held {peak} bytes, more than a piece + the state + the outputs = {bound}"
    del yp, res, ts

    # ---- the torch route, memory: the block + the sorted copy and the sort's indices
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fill(torch.empty(S, N, device=dev), scale, g)
    ref = torch_quantiles(y, LEVELS)
    torch.cuda.synchronize()
    out["torch_route_peak_bytes"] = torch.cuda.max_memory_allocated() - base

    # ---- agreement on the same block (the torch route interpolates in fp32)
    ts = cap.pred_tail_state(N, K, torch.float32, dev)
    cap.pred_tails(y, ts)
    got, _ = cap.pred_quantiles(ts, LEVELS)
    out["max_rel_diff_vs_torch"] = float(((got - ref).abs() / ref.abs()).max())
    assert int(ts["cnt"].min()) == S and not bool(torch.isnan(got).any())
    del ref, got

    states = {k: cap.pred_tail_state(N, K, torch.float32, dev) for k in ("whole", "pieces", "pair")}
    plain = cap.pred_state(N, dev)

    def whole():
        states["whole"]["cnt"].zero_()
        cap.pred_tails(y, states["whole"])

    def pieces():
        states["pieces"]["cnt"].zero_()
        for lo in range(0, S, piece):
            cap.pred_tails(y[lo:lo + piece], states["pieces"])

    def pair():
        states["pair"]["cnt"].zero_()
        cap.pred_tails(y, states["pair"])
        cap.pred_quantiles(states["pair"], LEVELS)
    fns = {"tails": whole, f"tails_in_{PIECES}_pieces": pieces, "quantiles": lambda: cap.pred_quantiles(ts, LEVELS),
           "tails_plus_quantiles": pair, "torch_sort_from_block": lambda: torch_quantiles(y, LEVELS),
           "fold_plain": lambda: cap.pred_fold(y, plain, None, None, None, None)}
    r = timed(fns, reps)
    r["tails_plus_quantiles"]["ratio_to_torch_sort"] = r["tails_plus_quantiles"]["median_ms"] / r["torch_sort_from_block"]["median_ms"]
    r["tails_plus_quantiles"]["ratio_to_fold_plain"] = r["tails_plus_quantiles"]["median_ms"] / r["fold_plain"]["median_ms"]
    r["tails"]["ratio_to_fold_plain"] = r["tails"]["median_ms"] / r["fold_plain"]["median_ms"]
    out["timings"] = r
    out["inserts"] = count_inserts(y[:, :256].cpu().numpy(), K)
    out["workgroups"] = -(-N // 256)                                          # one entry per lane, 256 lanes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("quantile_bench.py needs the GPU: it measures, it does not estimate")
    rows = [workload(S, B, T, a.reps) for S, B, T in WORKLOADS]
    out = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "reps": a.reps, "workloads": rows}
    for row in rows:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
