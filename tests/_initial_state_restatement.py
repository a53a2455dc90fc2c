"""NumPy fp64 restatement of the initial-state layer (csrc/hode_x0.hip; include/hode.h, "Initial-state model"), written from the
specification: the map from chain coordinates to one initial state per (row, patient), the optional global-constants block, and
the transposes.  `lat` lists the latent state indices in ascending order; link 0 is the identity, 1 the log link."""
import numpy as np


def x0_lat(w, m, s, lat, link):
    """w [..., B, n_lat] -> the latent entries of x0 [..., B, n_lat]; m, s [B, 6]."""
    ml, sl = np.asarray(m, dtype=np.float64)[:, lat], np.asarray(s, dtype=np.float64)[:, lat]
    return ml * np.exp(sl * w) if link else ml + sl * w


def split(coords, off, B, n_lat):
    """coords [A, ld] -> w [A, B, n_lat]: columns off .. off + B n_lat - 1, patient-major."""
    A = coords.shape[0]
    return np.asarray(coords, dtype=np.float64)[:, off:off + B * n_lat].reshape(A, B, n_lat)


def x0_params(coords, off, B, lat, link, m, s, x0_base):
    """-> (x0 [A, B, 6], the summed magnitudes of the terms of the latent entries [A, B, n_lat]): |m| + |s w| for the identity
    link, |x0| (1 + |s w|) for the log link (an ulp of exp's argument is that much of x0)."""
    w = split(coords, off, B, len(lat))
    A = w.shape[0]
    x = x0_lat(w, m, s, lat, link)
    out = np.broadcast_to(np.asarray(x0_base, dtype=np.float64), (A, B, 6)).copy()
    out[..., lat] = x
    sw = np.abs(np.asarray(s, dtype=np.float64)[:, lat] * w)
    mag = np.abs(x) * (1 + sw) if link else np.abs(np.asarray(m, dtype=np.float64)[:, lat]) + sw
    return out, mag


def ode_params(coords, idx, mu, sd, ode_base):
    """-> (ode_p [A, 17], the summed magnitudes |mu| + |sd z| of the K sampled entries [A, K])."""
    c = np.asarray(coords, dtype=np.float64)
    K = len(idx)
    out = np.broadcast_to(np.asarray(ode_base, dtype=np.float64), (c.shape[0], 17)).copy()
    z = c[:, :K]
    out[:, idx] = np.asarray(mu)[:K] + np.asarray(sd)[:K] * z
    return out, np.abs(np.asarray(mu)[:K]) + np.abs(np.asarray(sd)[:K] * z)


def dx0_dw(coords, off, B, lat, link, m, s):
    """d x0[b, j] / d w[b, rank(j)] [A, B, n_lat]: s, or s x0 for the log link."""
    w = split(coords, off, B, len(lat))
    sl = np.asarray(s, dtype=np.float64)[:, lat]
    return sl * x0_lat(w, m, s, lat, link) if link else np.broadcast_to(sl, w.shape).copy()


def x0_transpose(coords, off, B, lat, link, m, s, gx0):
    """gx0 [A, B, 6] -> (the likelihood gradient of w [A, B n_lat], its magnitudes): one term per entry."""
    g = np.asarray(gx0, dtype=np.float64)[..., lat] * dx0_dw(coords, off, B, lat, link, m, s)
    return g.reshape(g.shape[0], -1), np.abs(g).reshape(g.shape[0], -1)


def ode_transpose(gode, idx, sd):
    """gode [A, 17] -> the likelihood gradient of the K constants' coordinates [A, K]."""
    return np.asarray(sd, dtype=np.float64)[:len(idx)] * np.asarray(gode, dtype=np.float64)[:, idx]


def from_batch(first_obs, lat, inflate=1.0):
    """The cohort prior: per latent state the mean and the ddof-1 sd, times inflate, of the finite first observations [B, 6]."""
    mean, sd = np.zeros(6), np.ones(6)
    for j in lat:
        v = first_obs[:, j]
        v = v[np.isfinite(v)]
        mean[j], sd[j] = v.mean(), v.std(ddof=1) * inflate
    return mean, sd
