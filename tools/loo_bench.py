#!/usr/bin/env python3
"""Time the LOO kernels (csrc/hode_loo.hip, "Model comparison") against PSIS-LOO computed with torch from the held [draws, N]
fp64 block of pointwise log likelihoods: torch.topk(M + 1, dim=0) of the importance ratios, a generalised Pareto fit vectorised
over the entries, the smoothed tail scattered back into the block and two logsumexp over the draws -- what arviz.loo does with
its [draws, N] array, and what a user of this package would write today.

    python tools/loo_bench.py [--reps 20] [--out profiles/predictive_loo.json]

Workloads, fp32 draws, r_eff = 1: those of tools/quantile_bench.py, 256 draws x 64 windows x 61 points and 1 024 draws x 64
windows x 241 points (x 6 states), the draws folded whole and in 16 pieces.  Times are HIP events around each call, the routes
alternating, after warm-up; the fold WITH observation noise (hode_pred_fold_*: the same l, a PIT and one log-sum-exp) is timed in
the same run for scale.  Peak memory is torch's allocator high-water mark of each route; the kernel route's peak is CHECKED
against one piece of draws + the state ((K + 6.5) * 8 N bytes) and, in the finish, the state + the scratch buffer
((K - 1 + 30 + floor(sqrt(K - 1))) * 8 N bytes) + the outputs, each tensor rounded up as torch's caching allocator rounds it.  The inserts
per entry into the heap, and the share of (wave, draw) pairs in which at least one lane walks it, are counted on the host for
the first 256 entries."""
import argparse
import heapq
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from quantile_bench import allocator_size, fill, timed  # noqa: E402

WORKLOADS = ((256, 64, 61), (1024, 64, 241))
PIECES = 16
HALF_LOG_2PI = 0.91893853320467274178


def torch_loo(y, obs, sigma, M):
    """PSIS-LOO from the held block: (elpd_loo [N], pareto_k [N], tie [N]) in fp64.  y [S, N] fp32, obs [N], sigma [S, 6].  It takes the
    M largest ratios as the tail; `tie` marks the entries where the M-th largest equals the cut (fp32 draws do tie), for which
    the specification -- and the kernel -- take a shorter tail."""
    import torch
    S, N = y.shape
    sig = sigma[:, None, :].expand(S, N // 6, 6).reshape(S, N)
    z = (obs.double()[None] - y.double()) / sig
    l = -0.5 * z * z - torch.log(sig) - HALF_LOG_2PI                                             # the [S, N] fp64 block
    del z, sig
    top = torch.topk(-l, M + 1, dim=0)
    c = top.values[0]
    x = top.values - c
    x_cut = torch.clamp(x[M], min=math.log(sys.float_info.min))
    e_cut = torch.exp(x_cut)
    a = torch.exp(x[:M].flip(0)) - e_cut                                                           # [M, N] ascending
    m = 30 + int(math.floor(math.sqrt(M)))
    q = torch.arange(1, m + 1, dtype=torch.float64, device=y.device)
    b = (1.0 - torch.sqrt(m / (q - 0.5)))[:, None] / (3.0 * a[int(M / 4.0 + 0.5) - 1])[None] + (1.0 / a[-1])[None]      # [m, N]
    kq = torch.stack([torch.log1p(-b[i] * a).mean(0) for i in range(m)])
    L = M * (torch.log(-(b / kq)) - kq - 1.0)
    w = torch.stack([1.0 / torch.exp(L - L[i]).sum(0) for i in range(m)])
    w = torch.where(w >= 10.0 * 2.0 ** -52, w, torch.zeros_like(w))
    w = w / w.sum(0)
    bp = (w * b).sum(0)
    kp = torch.log1p(-bp * a).mean(0)
    sg = -kp / bp
    k = (M * kp + 5.0) / (M + 10.0)
    p = ((torch.arange(1, M + 1, dtype=torch.float64, device=y.device) - 0.5) / M)[:, None]
    xs = torch.clamp(torch.log(sg * torch.expm1(-k * torch.log1p(-p)) / k + e_cut), max=0.0)       # [M, N] ascending
    ok = torch.isfinite(k) & (sg > 0)
    xs = torch.where(ok, xs, x[:M].flip(0))
    xa = -l - c                                                                                    # every draw's log weight
    xa.scatter_(0, top.indices[:M].flip(0), xs)
    return torch.logsumexp(xa + l, 0) - torch.logsumexp(xa, 0), k, top.values[M - 1] == top.values[M]


def count_inserts(r, K):
    """Host count over the columns of r [S, n]: values that enter the heap (fill included) per entry, and the share of (wave of
    64 entries, draw) pairs in which at least one lane's value does."""
    S, n = r.shape
    hit = [[False] * S for _ in range(n)]
    ins = 0
    for i in range(n):
        h = []
        for s in range(S):
            v = float(r[s, i])
            if s < K:
                heapq.heappush(h, v)
                hit[i][s] = True
                ins += 1
            elif h[0] < v:
                heapq.heapreplace(h, v)
                hit[i][s] = True
                ins += 1
    waves = [range(w, min(w + 64, n)) for w in range(0, n, 64)]
    busy = sum(any(hit[i][s] for i in w) for w in waves for s in range(S))
    return {"entries_counted": n, "inserts_per_entry_incl_fill": ins / n, "expected_K_1_plus_ln_S_over_K": K * (1.0 + math.log(S / K)),
            "share_of_wave_draws_with_an_insert": busy / (len(waves) * S), "share_of_lane_draws_with_an_insert": ins / (n * S)}


def workload(S, B, T, reps):
    import torch
    import hode
    from inference.predictive import loo_tail_size
    cap = hode.capi
    dev = torch.device("cuda")
    N = B * T * 6
    K = loo_tail_size(S)
    M = K - 1
    piece = -(-S // PIECES)
    g = torch.Generator(device=dev).manual_seed(0)
    scale6 = torch.tensor([120.0, 15.0, 60.0, 8.0, 0.5, 0.4], device=dev)
    scale = scale6.repeat(N // 6)
    obs = fill(torch.empty(N, device=dev), scale, g)
    sigma = (0.05 * scale6.double()).reshape(1, 6).repeat(S, 1).contiguous()
    rows = cap.pred_loo_fit_rows(K)
    out = {"draws": S, "windows": B, "points": T, "N": N, "K": K, "M": M, "fit_rows": rows, "piece": piece, "loglik_block_bytes": S * N * 8}

    # ---- the kernel route, memory: one piece of draws + the state, then the state + the finish's scratch + the outputs
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yp = torch.empty(piece, N, device=dev)
    ls = cap.pred_loo_state(N, K, dev)
    for lo in range(0, S, piece):
        n = min(piece, S - lo)
        fill(yp[:n], scale, g)
        cap.pred_loo_fold(yp[:n], ls, obs, None, sigma[lo:lo + n])
    torch.cuda.synchronize()
    fold_peak = torch.cuda.max_memory_allocated() - base
    del yp
    torch.cuda.reset_peak_memory_stats()
    res, table = cap.pred_loo_finish(ls, torch.float32)
    torch.cuda.synchronize()
    finish_peak = torch.cuda.max_memory_allocated() - base
    up = allocator_size
    state = up(4 * N) + 6 * up(8 * N) + up(K * N * 8)
    fold_bound = up(piece * N * 4) + state
    finish_bound = state + up(rows * N * 8) + 5 * up(4 * N) + 2 * up(128 * 6 * 13 * 8)
    out.update(kernel_route_fold_peak_bytes=fold_peak, kernel_route_fold_bound_bytes=fold_bound, kernel_route_finish_peak_bytes=finish_peak,
               kernel_route_finish_bound_bytes=finish_bound, state_bytes=4 * N + (K + 6) * 8 * N, fit_bytes=rows * N * 8)
    assert fold_peak <= fold_bound, f"the fold held {fold_peak} bytes, more than a piece + the state = {fold_bound}"
    assert finish_peak <= finish_bound, f"the finish held {finish_peak} bytes, more than the state + its scratch + the outputs = {finish_bound}"
    del res, table, ls

    # ---- the torch route, memory: the fp64 block, topk's buffers, the weights
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fill(torch.empty(S, N, device=dev), scale, g)
    ref, ref_k, tie = torch_loo(y, obs, sigma, M)
    torch.cuda.synchronize()
    out["torch_route_peak_bytes"] = torch.cuda.max_memory_allocated() - base

    # ---- agreement on the same block
    ls = cap.pred_loo_state(N, K, dev)
    cap.pred_loo_fold(y, ls, obs, None, sigma)
    got, table = cap.pred_loo_finish(ls, torch.float32)
    assert int(ls["cnt"].min()) == S and not bool(torch.isnan(got["elpd_loo"]).any())
    de = (got["elpd_loo"].double() - ref).abs()
    dk = (got["pareto_k"].double() - ref_k).abs()
    off = (de > 1e-5 * ref.abs().clamp(min=1.0)) | ~(dk <= 1e-5 * ref_k.abs().clamp(min=1.0))       # (the outputs are fp32)
    out["entries_with_a_tie_at_the_cut"] = int(tie.sum())
    out["entries_that_differ_from_torch"] = int(off.sum())
    out["entries_that_differ_without_a_tie"] = int((off & ~tie).sum())
    out["max_abs_diff_elpd_vs_torch_no_tie"] = float(de[~tie].max())
    out["max_abs_diff_k_vs_torch_no_tie"] = float(dk[~tie].max())
    out["max_abs_diff_elpd_vs_torch"] = float(de.max())
    out["pareto_k_counts"] = table[:, 8:12].sum(0).tolist()
    print(json.dumps({k: v for k, v in out.items() if "diff" in k or "tie" in k}), flush=True)
    assert out["entries_that_differ_without_a_tie"] == 0
    del ref, ref_k, got, de, dk, off, tie

    states = {k: cap.pred_loo_state(N, K, dev) for k in ("whole", "pieces", "pair")}
    plain = cap.pred_state(N, dev)

    def reset(st):
        st["cnt"].zero_()
        for k in ("lmean", "lm2", "psum", "rsum"):
            st[k].zero_()
        st["pmax"].fill_(float("-inf"))
        st["rmax"].fill_(float("-inf"))

    def whole():
        reset(states["whole"])
        cap.pred_loo_fold(y, states["whole"], obs, None, sigma)

    def pieces():
        reset(states["pieces"])
        for lo in range(0, S, piece):
            cap.pred_loo_fold(y[lo:lo + piece], states["pieces"], obs, None, sigma[lo:lo + piece])

    def pair():
        reset(states["pair"])
        cap.pred_loo_fold(y, states["pair"], obs, None, sigma)
        cap.pred_loo_finish(states["pair"], torch.float32)
    fns = {"state_reset": lambda: reset(states["whole"]), "loo_fold": whole, f"loo_fold_in_{PIECES}_pieces": pieces,
           "loo_finish": lambda: cap.pred_loo_finish(ls, torch.float32), "loo_fold_plus_finish": pair,
           "torch_psis_from_block": lambda: torch_loo(y, obs, sigma, M), "fold_with_noise": lambda: cap.pred_fold(y, plain, obs, None, sigma, None)}
    r = timed(fns, reps)
    r["loo_fold_plus_finish"]["ratio_to_torch"] = r["loo_fold_plus_finish"]["median_ms"] / r["torch_psis_from_block"]["median_ms"]
    r["loo_fold"]["ratio_to_fold_with_noise"] = r["loo_fold"]["median_ms"] / r["fold_with_noise"]["median_ms"]
    out["timings"] = r
    sig256 = sigma[:, None, :].expand(S, 256 // 6 + 1, 6).reshape(S, -1)[:, :256]
    z = (obs[:256].double()[None] - y[:, :256].double()) / sig256
    out["inserts"] = count_inserts((0.5 * z * z + torch.log(sig256)).cpu().numpy(), K)
    out["workgroups"] = -(-N // 256)                                          # one entry per lane, 256 lanes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("loo_bench.py needs the GPU: it measures, it does not estimate")
    rows = [workload(S, B, T, a.reps) for S, B, T in WORKLOADS]
    out = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "reps": a.reps, "workloads": rows}
    for row in rows:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
