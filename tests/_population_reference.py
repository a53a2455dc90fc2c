"""A numpy fp64 restatement of the population model of inference/population.py / csrc/hode_population.hip: the row layout, the
map from chain coordinates to per-patient constants, and its transpose."""
import numpy as np


def layout(K, B):
    """A row is [ m_0..m_{K-1} | s_0..s_{K-1} | z_{0,0}..z_{0,K-1} | ... | z_{B-1,K-1} ]: D = K (B + 2) values."""
    return {"m": slice(0, K), "s": slice(K, 2 * K), "z": slice(2 * K, K * (B + 2)), "D": K * (B + 2)}


def split(coords, K, B):
    """coords [..., >= D] -> (m [..., K], s [..., K], z [..., B, K]) in fp64."""
    c = np.asarray(coords, dtype=np.float64)
    lay = layout(K, B)
    return c[..., lay["m"]], c[..., lay["s"]], c[..., lay["z"]].reshape(*c.shape[:-1], B, K)


def hyper(coords, K, B, mu0, sd0, tau0, omega):
    """(mu_pop [..., K], tau [..., K])."""
    m, s, _ = split(coords, K, B)
    return np.asarray(mu0, np.float64) + np.asarray(sd0, np.float64) * m, np.asarray(tau0, np.float64) * np.exp(omega * s)


def pop_map(coords, K, B, mu0, sd0, tau0, omega):
    """theta [..., B, K] = mu_pop + tau z."""
    mu, tau = hyper(coords, K, B, mu0, sd0, tau0, omega)
    return mu[..., None, :] + tau[..., None, :] * split(coords, K, B)[2]


def pop_params(coords, K, B, idx, mu0, sd0, tau0, omega, ode_base):
    """ode_p [A, B, 17]: the sampled constants (ODE indices idx, ascending) from the map, the others from ode_base."""
    th = pop_map(coords, K, B, mu0, sd0, tau0, omega)
    out = np.broadcast_to(np.asarray(ode_base, np.float64), th.shape[:-1] + (17,)).copy()
    out[..., list(idx)] = th
    return out


def pop_transpose(coords, G, K, B, sd0, tau0, omega):
    """The transposed map at coords: G [..., B, K] = d NLL / d theta -> the gradient with respect to the D coordinates [..., D]
    and, for error bounds, the sum of the absolute values of the terms of every entry."""
    G = np.asarray(G, dtype=np.float64)
    _, s, z = split(coords, K, B)
    tau = np.asarray(tau0, np.float64) * np.exp(omega * s)
    sd0 = np.asarray(sd0, np.float64)
    g = np.concatenate([sd0 * G.sum(-2), omega * tau * (G * z).sum(-2), (tau[..., None, :] * G).reshape(*G.shape[:-2], B * K)], -1)
    mag = np.concatenate([np.abs(sd0) * np.abs(G).sum(-2), omega * tau * np.abs(G * z).sum(-2),
                          np.abs(tau[..., None, :] * G).reshape(*G.shape[:-2], B * K)], -1)
    return g, mag


def pooling(offsets):
    """Gelman-Pardoe pooling factor [K] from the offsets tau_k z_bk of all draws, [S, B, K]."""
    e = np.asarray(offsets, np.float64)
    return 1.0 - e.mean(0).var(0, ddof=1) / e.var(1, ddof=1).mean(0)
