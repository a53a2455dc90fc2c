#!/usr/bin/env python3
"""Time the latent initial-state layer (inference/initial_state.py, csrc/hode_x0.hip) at the reference's MCMC workload: a 64 x 4
HybridODENN, the 32-window x 61-point 4GI batch of tools/hmc_bench.py, C = 64 chains, the reference's seven constants.

    python tools/initial_state_bench.py [--chains 64] [--leapfrog 8] [--repeats 10] [--out profiles/initial_state_bench.json]

One JSON line: the time of one HMC iteration (refresh, L leapfrog steps, accept) of run_hmc(sample_nn=False)'s sampler without
and with a latent initial state (the four states the 4GI data observe -- G, I, Glu, GLP1 -- of every patient latent, a cohort
prior from the batch: D = 7 -> 7 + 32 x 4), in the same process on the same box, the two alternating, each the median of
`repeats` windows timed with device events; likewise one `evaluate()` of each; and
the time per call of the two kernels hode_x0_params / hode_x0_grad at that shape (A = 64, B = 32, K = 7; a window of 200 calls
between two events, the median of `repeats` windows).  The reference is the run without a latent state: gx0 is computed by the
adjoint either way, and the layer moves A x B x 6 values each way."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from hmc_bench import B, H, L_NN, T, batch  # noqa: E402


def _window(fn, calls):
    """Seconds per call of `calls` calls between two device events."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def _alternate(fns, calls, repeats):
    """The median window of every function, the functions alternating window by window (after one warm-up window each)."""
    for fn in fns:
        _window(fn, 1)
    times = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            times[i].append(_window(fn, calls))
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def bench(C, L, repeats, data):
    import torch
    import hode
    from inference import InitialStatePrior
    from inference.hmc import _Sampler
    from inference.initial_state import _LatentTarget
    from models.hybrid_ode_nn import HybridODENN
    torch.manual_seed(0)
    m = HybridODENN(nn_hidden=H, nn_layers=L_NN, device="cuda")
    prior = InitialStatePrior.from_batch(data, states=("G", "I", "Glu", "GLP1"), inflate=1.0)
    plain = _Sampler(m, data, C, sample_nn=False, seed=0)
    latent = _Sampler(m, data, C, seed=0, target=_LatentTarget(prior, data))
    its = []
    for s in (plain, latent):
        s.initial_jitter()
        s.gradient()
        s.log_eps.fill_(-7.0)                  # a small step: every proposal stays where the solve is well behaved
        it = [0]

        def iteration(s=s, it=it):
            s.refresh(it[0])
            s.trajectory(L)
            s.accept(1, it[0])
            it[0] += 1
        its.append(iteration)
    (t_plain, t_latent), (r_plain, r_latent) = _alternate(its, 1, repeats)
    (e_plain, e_latent), _ = _alternate([plain.evaluate, latent.evaluate], 1, repeats)
    tg, cap = latent.target, hode.capi
    lat = tg.lat
    args = (C, lat.B, lat.n_lat, latent.P, tg.off, latent.nn_p, lat.lat_mask, lat.link_code, tg.m_d, tg.s_d)
    gx0 = torch.randn(C * lat.B, 6, dtype=latent.dt, device=latent.dev)
    gode = torch.randn(C, 17, dtype=latent.dt, device=latent.dev)

    def k_params():
        cap.x0_params(*args, latent.x0, latent.x0_rows, tg.g_K, tg.g_mask, tg.g_mu, tg.g_sd, latent.ode_base, latent.ode_p)

    def k_grad():
        cap.x0_grad(*args, gx0, latent.glik, tg.g_K, tg.g_mask, tg.g_sd, gode)
    (k_p, k_g), _ = _alternate([k_params, k_grad], 200, repeats)
    return {"chains": C, "patients": B, "points": T, "K": tg.g_K, "n_lat": lat.n_lat, "D_plain": plain.D, "D_latent": latent.D,
            "trajectories": C * B, "leapfrog": L, "repeats": repeats,
            "hmc_iteration_s": {"plain": t_plain, "latent": t_latent, "ratio": t_latent / t_plain,
                                "plain_min_max": r_plain, "latent_min_max": r_latent},
            "evaluate_s": {"plain": e_plain, "latent": e_latent, "ratio": e_latent / e_plain},
            "kernel_us_per_call": {"x0_params": k_p * 1e6, "x0_grad": k_g * 1e6},
            "layer_share_of_evaluate": (k_p + k_g) / e_latent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--leapfrog", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import hode
    hode.build_info.ensure(may_build=False)
    data = batch(torch.device("cuda"))
    r = bench(a.chains, a.leapfrog, a.repeats, data)
    print(json.dumps(r), flush=True)
    if a.out:
        json.dump(r, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
