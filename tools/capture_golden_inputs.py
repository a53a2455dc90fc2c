#!/usr/bin/env python3
"""Capture the input-gradient fixture G10 from the reference implementation.

Runs ONLY where the reference checkout exists (it imports the reference's `models` package) and writes data only --
inputs, weights and torch fp64 autograd results -- to tests/golden/g10_input_grads.npz:

  (a) d ode_residual / d {meal, tVNS, GD} (models/hybrid_ode_nn.py:108-134) at random states, GD > 0 so the Hill term of
      k_GE is live, cotangent w: grads of sum(w * f) for three networks: 64 x 4 ReLU, 128 x 5 ReLU, 96 x 6 tanh
      (keys  a_<tag>_*; the network of <tag>: <tag>_nn_flat, fp32 values used in fp64, and <tag>_ode);
  (b) a classic RK4 loop, one step per grid interval, inputs lerped on the grid as the reference's forward does
      (hybrid_ode_nn.py:217-231), built here on top of the reference's ode_residual in .double(): y and
      d<gy, y>/d inputs for [B,T] inputs and for [B] inputs, B = 8, T = 25, networks 64 x 4 and 128 x 5 ReLU
      (keys  b_<tag>_<mode>_*).

Usage:  python tools/capture_golden_inputs.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "g10_input_grads.npz")
sys.path.insert(0, REF)

from models.hybrid_ode_nn import HybridODENN  # noqa: E402
from models.nn_residual import NNResidual  # noqa: E402

torch.set_num_threads(1)
CPU = torch.device("cpu")
ODE_NAMES = ["a_GI", "k_I", "rho", "G_b", "I_b", "E_max", "EC_50", "Glu_b", "V_max", "K_m",
             "k_L", "k_GE0", "IGD_50", "g", "p_7", "p_8", "p_9"]
KEYS = ("meal", "tVNS", "GD")


def model(hidden, layers, act, seed):
    torch.manual_seed(seed)
    m = HybridODENN(nn_hidden=hidden, nn_layers=layers, device=CPU)
    if act != "relu":
        m.nn_residual = NNResidual(input_dim=9, hidden_dim=hidden, output_dim=6, n_layers=layers, activation=act)
    with torch.no_grad():
        m.nn_residual.network[-1].weight.normal_(0, 0.05)
        m.nn_residual.network[-1].bias.normal_(0, 0.01)
        for lin in [l for l in m.nn_residual.network[:-1] if isinstance(l, torch.nn.Linear)]:
            lin.bias.normal_(0, 0.1)
    return m.double()          # (fp32 weights, exactly representable: the fixture stores them as fp32)


def flat_nn(m):
    return torch.cat([p.detach().reshape(-1) for p in m.nn_residual.parameters()]).numpy().astype(np.float32)


def ode_vec(m):
    return np.array([float(getattr(m.ode_core, n)) for n in ODE_NAMES], dtype=np.float64)


def states(n, g):
    base = torch.tensor([5., 60., 80., 10., 0.5, 1.], dtype=torch.float64)
    return base * (1 + 0.2 * torch.randn(n, 6, generator=g, dtype=torch.float64))


def part_a(out, tag, m, seed):
    g = torch.Generator().manual_seed(seed)
    n = 48
    x = states(n, g)
    t = torch.rand(n, generator=g, dtype=torch.float64) * 20
    u = {"meal": torch.rand(n, generator=g, dtype=torch.float64) * 10,
         "tVNS": torch.rand(n, generator=g, dtype=torch.float64),
         "GD": 50 + 1000 * torch.rand(n, generator=g, dtype=torch.float64)}
    w = torch.randn(n, 6, generator=g, dtype=torch.float64)
    ur = {k: v.clone().requires_grad_(True) for k, v in u.items()}
    f = m.ode_residual(t, x, ur)
    grads = torch.autograd.grad((f * w).sum(), [ur[k] for k in KEYS])
    out[f"a_{tag}_x"], out[f"a_{tag}_t"], out[f"a_{tag}_w"] = x.numpy(), t.numpy(), w.numpy()
    out[f"a_{tag}_f"] = f.detach().numpy()
    for k, gk in zip(KEYS, grads):
        out[f"a_{tag}_{k}"] = u[k].numpy()
        out[f"a_{tag}_g_{k}"] = gk.numpy()


def rk4(m, x0, t, u):
    """classic RK4, one step per interval; stage inputs u_k + alpha (u_{k+1} - u_k) for [B,T] inputs, u[b] for [B] ones"""
    B, T = x0.shape[0], t.shape[0]
    ys = [x0]
    y = x0
    for k in range(T - 1):
        h = t[k + 1] - t[k]

        def inp(alpha):
            return {key: (v[:, k] + alpha * (v[:, k + 1] - v[:, k])) if v.dim() == 2 else v for key, v in u.items()}

        def f(tau, yy, alpha):
            return m.ode_residual(tau.expand(B), yy, inp(alpha))
        k1 = f(t[k], y, 0.0)
        k2 = f(t[k] + h / 2, y + h / 2 * k1, 0.5)
        k3 = f(t[k] + h / 2, y + h / 2 * k2, 0.5)
        k4 = f(t[k] + h, y + h * k3, 1.0)
        y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        ys.append(y)
    return torch.stack(ys, 1)


def part_b(out, tag, m, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = 8, 25
    x0 = states(B, g)
    t = torch.linspace(0, 6, T, dtype=torch.float64)
    gy = torch.randn(B, T, 6, generator=g, dtype=torch.float64)
    series = {"meal": 5 * torch.rand(B, T, generator=g, dtype=torch.float64),
              "tVNS": torch.rand(B, T, generator=g, dtype=torch.float64),
              "GD": 100 + 800 * torch.rand(B, T, generator=g, dtype=torch.float64)}
    const = {"meal": 5 * torch.rand(B, generator=g, dtype=torch.float64),
             "tVNS": torch.rand(B, generator=g, dtype=torch.float64),
             "GD": 100 + 800 * torch.rand(B, generator=g, dtype=torch.float64)}
    out[f"b_{tag}_x0"], out[f"b_{tag}_t"], out[f"b_{tag}_gy"] = x0.numpy(), t.numpy(), gy.numpy()
    for mode, u in (("series", series), ("const", const)):
        ur = {k: v.clone().requires_grad_(True) for k, v in u.items()}
        y = rk4(m, x0, t, ur)
        grads = torch.autograd.grad((y * gy).sum(), [ur[k] for k in KEYS])
        out[f"b_{tag}_{mode}_y"] = y.detach().numpy()
        for k, gk in zip(KEYS, grads):
            out[f"b_{tag}_{mode}_{k}"] = u[k].numpy()
            out[f"b_{tag}_{mode}_g_{k}"] = gk.numpy()


def main():
    out = {}
    nets = {"h64l4": (64, 4, "relu", 1), "h128l5": (128, 5, "relu", 2), "h96l6tanh": (96, 6, "tanh", 3)}
    for tag, (H, L, act, seed) in nets.items():
        m = model(H, L, act, seed)
        out[f"{tag}_nn_flat"], out[f"{tag}_ode"] = flat_nn(m), ode_vec(m)      # fp32 weights (exact in fp64), fp64 constants
        part_a(out, tag, m, 100 + seed)
        if act == "relu":
            part_b(out, tag, m, 200 + seed)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
