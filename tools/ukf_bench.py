#!/usr/bin/env python3
"""Time the unscented Kalman filter (inference/ukf.py, csrc/hode_ukf.hip) next to the particle filter, fp32, a 64 x 4
HybridODENN, 241 grid points, glucose observed at every 5th grid point (48 filter steps + the initial one): the workload of
tools/filter_bench.py.

    python tools/ukf_bench.py [--patients 64] [--cohort 4096] [--points 241] [--every 5] [--iters 50] [--seeds 8] [--out profiles/ukf_bench.json]

One JSON line:
  ukf_step_us         one launch of the step kernel (device events around each of --iters launches, median) at B = --patients and
                      B = --cohort, without learned constants (P = 0, K = 13) and with three (P = 3, K = 19);
  torch_step_us       a torch composition of the same step (batched torch.linalg.cholesky / solve_triangular in fp64): the baseline;
  run_ukf_s           the whole run_ukf at --patients and at --cohort (host clock, ends in a synchronise; the median of 5 after a
                      warm-up), and at --patients its split into the segment solves and the steps (device events around every call);
  run_filter_s        run_filter at --patients x 1 024 particles in the same session, the same way;
  against_pf          on the --patients case: the UKF's log-evidence and filtered glucose mean against the particle filter's
                      (N = 4 096) mean over --seeds seeds, in units of the particle filter's own seed-to-seed standard deviation.
The record's fifth state starts at exactly 0, which a Gaussian on the logarithm cannot hold, so both filters run with additive
noise here (5 % of every state's typical size per sqrt(time), none on the fifth): the same state model for both.
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


def _events(fn, iters):
    """Median / min device time of fn() in microseconds."""
    import torch
    fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    us = [1e3 * a.elapsed_time(b) for a, b in pairs]
    return {"median": statistics.median(us), "min": min(us)}


def torch_step(x_in, aux_in, cols, obs0, sigma0, s2, w):
    """The same step composed from torch operations in fp64 (log link on the states and the constants, glucose observed): the
    baseline.  x_in [B, K, 6], aux_in [B, K, 17], s2 [n] the added variances, w = (gamma, wm0, wc0, wi)."""
    import torch
    gamma, wm0, wc0, wi = w
    B, K, _ = x_in.shape
    n = 6 + len(cols)
    wm = torch.full((K,), wi, dtype=torch.float64, device=x_in.device)
    wc = wm.clone()
    wm[0], wc[0] = wm0, wc0

    def points(m, P):
        L = torch.linalg.cholesky(P)
        return torch.cat([m.unsqueeze(1), m.unsqueeze(1) + gamma * L.transpose(1, 2), m.unsqueeze(1) - gamma * L.transpose(1, 2)], 1)
    Z = torch.cat([x_in.double(), aux_in[:, :, cols].double()], 2).log()
    m = torch.einsum("k,bkj->bj", wm, Z)
    D = Z - m.unsqueeze(1)
    P = torch.einsum("k,bki,bkj->bij", wc, D, D) + torch.diag_embed(s2.expand(B, n))
    m = m.clone()
    m[:, :6] -= 0.5 * s2[:6]
    X = points(m, P)
    Y = X[:, :, :1].exp()
    yh = torch.einsum("k,bkj->bj", wm, Y)
    Dy, Dx = Y - yh.unsqueeze(1), X - m.unsqueeze(1)
    S = torch.einsum("k,bki,bkj->bij", wc, Dy, Dy) + sigma0 * sigma0
    C = torch.einsum("k,bki,bkj->bij", wc, Dx, Dy)
    LS = torch.linalg.cholesky(S)
    Wt = torch.linalg.solve_triangular(LS, C.transpose(1, 2), upper=False)          # [B, d, n]
    z = torch.linalg.solve_triangular(LS, (obs0.double() - yh).unsqueeze(2), upper=False)
    m = m + (Wt.transpose(1, 2) @ z).squeeze(2)
    P = P - Wt.transpose(1, 2) @ Wt
    P = 0.5 * (P + P.transpose(1, 2))
    inc = -0.5 * ((z * z).sum((1, 2)) + 2 * LS.diagonal(dim1=1, dim2=2).log().sum(1) + 1.8378770664093453)
    nat = points(m, P).exp()
    aux_out = aux_in[:, :1].repeat(1, K, 1)
    aux_out[:, :, cols] = nat[:, :, 6:].to(aux_in.dtype)
    mu = torch.einsum("k,bkj->bj", wm, nat[:, :, :6])
    var = torch.einsum("k,bkj->bj", wc, (nat[:, :, :6] - mu.unsqueeze(1)) ** 2)
    return nat[:, :, :6].to(x_in.dtype), aux_out, m, P, inc, mu, var


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=64)
    ap.add_argument("--cohort", type=int, default=4096)
    ap.add_argument("--points", type=int, default=241)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hode
    import inference.filter as F
    import inference.ukf as U
    from models.hybrid_ode_nn import HybridODENN
    hode.build_info.ensure(may_build=False)
    dev = torch.device("cuda")
    T = a.points
    torch.manual_seed(0)
    model = HybridODENN(nn_hidden=64, nn_layers=4, device=dev)
    with torch.no_grad():
        for p in model.nn_residual.parameters():
            p.normal_(0.0, 0.05)

    def record(B):
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
        size = (truth.abs().mean((0, 1)) + 0.1).double().cpu().numpy()
        return {"initial_state": x0, "time_points": t, "external_inputs": {"meal": meal}, "observations": obs}, sig, size, truth
    f64 = dict(dtype=torch.float64, device=dev)
    res = {"patients": a.patients, "cohort": a.cohort, "points": T, "dtype": "float32", "ukf_step_us": {}, "torch_step_us": {}}

    # ---- (a) the step alone, on points like the filter's: log links, glucose observed
    for B in (a.patients, a.cohort):
        for cols in ([], [2, 8, 11]):
            n, mode = 6 + len(cols), [2 if c in cols else 0 for c in range(17)]
            K = 2 * n + 1
            w = hode.capi.ukf_weights(n)
            g = torch.Generator(device=dev).manual_seed(2)
            centre = torch.tensor([8.0, 90.0, 80.0, 10.0, 1.0, 0.5], device=dev)
            x = (centre * torch.exp(0.1 * torch.randn(B, K, 6, device=dev, generator=g))).contiguous()
            aux = torch.exp(0.1 * torch.randn(B, K, 17, device=dev, generator=g)).contiguous()
            ob = torch.full((B, 6), float("nan"), device=dev)
            ob[:, 0] = 8.0
            sg, q, walk = torch.tensor([0.3, 1, 1, 1, 1, 1.0], **f64), torch.full((6,), 0.05, **f64), torch.full((17,), 0.02, **f64)
            dt, alive = torch.full((B,), 0.1, **f64), torch.ones(B, dtype=torch.int32, device=dev)
            mean, cov = torch.empty(B, n, **f64), torch.empty(B, n, n, **f64)
            out = (torch.empty_like(x), torch.empty_like(aux), torch.empty(B, 16, **f64))
            key = f"B{B}_P{len(cols)}"
            res["ukf_step_us"][key] = _events(lambda: hode.capi.ukf_step(x, aux, mode, ob, sg, q, walk, dt, alive, mean, cov, w, predict=True,
                                                                         link=1, out=out), a.iters)
            assert int(alive.sum()) == B
            s2 = torch.cat([q * q, walk[cols] * walk[cols]]) * 0.1
            res["torch_step_us"][key] = _events(lambda: torch_step(x, aux, cols, ob[:, :1], 0.3, s2, w), a.iters)
            ref = torch_step(x, aux, cols, ob[:, :1], 0.3, s2, w)
            res.setdefault("step_agreement", {})[key] = float((ref[2] - mean).abs().max())     # the two compute the same step

    # ---- (b), (c) the whole filters
    def wall(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return statistics.median(times)

    def split(run, step_name):
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
        solve_fwd, step = hode.solve_fwd, getattr(hode.capi, step_name)
        hode.solve_fwd = timed("solve", solve_fwd)
        setattr(hode.capi, step_name, timed("step", step))
        try:
            run()
            torch.cuda.synchronize()
        finally:
            hode.solve_fwd = solve_fwd
            setattr(hode.capi, step_name, step)
        return {k: sum(s.elapsed_time(e) for kind, s, e in marks if kind == k) / 1e3 for k in ("solve", "step")}
    data, sig, size, truth = record(a.patients)
    sigma = [sig, 1.0, 1.0, 1.0, 1.0, 1.0]
    noise = dict(process_noise=0.05 * size * np.array([1, 1, 1, 1, 0, 1.0]), initial_spread=0.1 * size * np.array([1, 1, 1, 1, 0, 1.0]),
                 noise_sigma=sigma, noise_link="additive")
    ukf = lambda d=data: U.run_ukf(model, d, **noise)                                                          # noqa: E731
    r = ukf()
    sp = split(ukf, "ukf_step")
    res["run_ukf_s"] = {f"B{a.patients}": {"total": wall(ukf), "solves": sp["solve"], "steps": sp["step"], "filter_steps": len(r.step_index),
                                           "trajectories": a.patients * 13, "alive": int(r.alive[:, -1].sum())}}
    pf = lambda seed=0, N=1024: F.run_filter(model, data, n_particles=N, seed=seed, **noise)                  # noqa: E731
    sp = split(pf, "pf_step")
    res["run_filter_s"] = {f"B{a.patients}_N1024": {"total": wall(pf), "solves": sp["solve"], "steps": sp["step"]}}
    log_kw = dict(n_particles=1024, process_noise=0.05, noise_sigma=sigma, initial_spread=0.1, seed=0)       # tools/filter_bench.py's run
    res["run_filter_s"][f"B{a.patients}_N1024_log_link"] = {"total": wall(lambda: F.run_filter(model, data, **log_kw))}
    big, _, _, _ = record(a.cohort)
    rb = ukf(big)
    res["run_ukf_s"][f"B{a.cohort}"] = {"total": wall(lambda: ukf(big), reps=3), "trajectories": a.cohort * 13,
                                        "alive": int(rb.alive[:, -1].sum())}

    # ---- (d) against the particle filter at N = 4 096 over seeds
    ev, gl = [], []
    for seed in range(a.seeds):
        p = pf(seed, 4096)
        ev.append(p.log_evidence_steps.sum(1))
        gl.append(p.mean[..., 0])
    ev, gl = torch.stack(ev), torch.stack(gl)                                       # [seeds, B], [seeds, B, S]
    d_ev = (r.log_evidence_steps.sum(1) - ev.mean(0)) / ev.std(0)
    d_gl = (r.mean[..., 0] - gl.mean(0)) / gl.std(0)
    half = slice(len(r.step_index) // 2, None)
    rmse = lambda m: float(((m[:, half] - truth[:, r.step_index][:, half, 0].double()) ** 2).mean().sqrt())    # noqa: E731
    res["against_pf"] = {"seeds": a.seeds, "particles": 4096,
                         "log_evidence": {"ukf_mean": float(r.log_evidence_steps.sum(1).mean()), "pf_mean": float(ev.mean()),
                                          "pf_seed_sd_median": float(ev.std(0).median()),
                                          "abs_diff_in_sd": {"median": float(d_ev.abs().median()), "max": float(d_ev.abs().max())}},
                         "glucose_mean": {"pf_seed_sd_median": float(gl.std(0).median()),
                                          "abs_diff_in_sd": {"median": float(d_gl.abs().median()), "max": float(d_gl.abs().max())},
                                          "abs_diff_median": float((r.mean[..., 0] - gl.mean(0)).abs().median())},
                         "glucose_rmse_second_half": {"ukf": rmse(r.mean[..., 0]), "pf": rmse(gl.mean(0)), "sigma": sig}}
    print(json.dumps(res), flush=True)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
