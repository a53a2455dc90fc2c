"""The layouts, shapes, coordinate maps and seeded inputs that tests/test_chain_kernels_host.py (the margin condition, on the
CPU) and tests/test_chain_kernels_gpu.py (the kernels, one call at a time) share, and the one driver both use to walk a NUTS
tree call by call.  numpy only."""
import math

import numpy as np

import _chain_reference as R

DTYPES = (np.float32, np.float64)

# (D, ld, element offset of the base pointer).  ld % 4 == 0 with a 16-byte aligned base is the vector path, everything else
# the scalar one: (8, 8, 1) takes it with an aligned shape, (5, 7, 0) has a pad the scalar path must not touch, 1023 / 1024 /
# 1029 straddle one pass of 256 lanes x 4, (1029, 1032, 0) leaves a tail of one in lane 1 of the second pass.
LAYOUTS = ((1, 1, 0), (3, 4, 0), (5, 7, 0), (7, 7, 0), (7, 8, 0), (8, 8, 1), (17, 17, 0), (17, 20, 0), (1023, 1023, 0),
           (1024, 1024, 0), (1029, 1032, 0), (2051, 2051, 0))
TREE_LAYOUTS = ((7, 7, 0), (7, 8, 0), (1029, 1032, 0), (2051, 2051, 0))
CHAINS = (1, 3, 5)
COMPACT_C = (1, 63, 64, 65, 255, 256, 257, 600)
COMPACT_PATTERNS = ("on", "off", "alternating", "last", "random")
N_TRAJ = (None, 1, 257, 300)
SPARSE_MASK = (1 << 0) | (1 << 2) | (1 << 7) | (1 << 13) | (1 << 16)
THREE_MASK = (1 << 1) | (1 << 5) | (1 << 9)
LIK_SCALE = 0.7


def is_vec(layout, dtype):
    D, ld, off = layout
    return ld % 4 == 0 and (off * np.dtype(dtype).itemsize) % 16 == 0


def partner(layout, dtype):
    """The same D through the other path: a scalar layout's vector partner, a vector layout's misaligned twin."""
    D, ld, off = layout
    return (D, ld, 1) if is_vec(layout, dtype) else (D, (D + 3) // 4 * 4, 0)


def maps_for(D):
    """The coordinate maps (ode_mask, sample_nn, P) that give this D."""
    out = [(0, 1, D), (1 << 16, int(D > 1), D - 1)]
    if D >= 5:
        out.append((SPARSE_MASK, int(D > 5), D - 5))
    if D == 17:
        out.append(((1 << 17) - 1, 0, 0))
    if D > 3:
        out.append((THREE_MASK, 1, D - 3))
    return out


def n_ode_of(cmap):
    return bin(cmap[0]).count("1")


def rnd(a, dtype):
    """a as the kernel's type stores it, back in fp64."""
    return np.asarray(a, np.float64).astype(dtype).astype(np.float64)


def compact_pattern(C, pattern, seed=0):
    on = {"on": np.ones(C, bool), "off": np.zeros(C, bool), "alternating": np.arange(C) % 2 == 0,
          "last": np.arange(C) == C - 1, "random": np.random.default_rng(seed + C).random(C) < 0.4}[pattern]
    ist = np.random.default_rng(seed).integers(-5, 5, (C, 8)).astype(np.int32)
    ist[:, R.ACTIVE] = np.where(on, np.random.default_rng(seed + 1).integers(1, 4, C), 0)     # any non-zero is active
    return ist


def status_array(rows, n_traj, hit):
    """[rows][n_traj] zeros; with hit, the single non-zero entry is the last trajectory of the last row."""
    if n_traj is None:
        return None
    st = np.zeros((rows, n_traj), np.int32)
    if hit:
        st[-1, -1] = 3
    return st


def chain_inputs(D, C, dtype, cmap, seed):
    """A complete, seeded input state of the HMC passes, every real array as the kernel's type stores it."""
    g = np.random.default_rng(seed)
    n_ode, P = n_ode_of(cmap), cmap[2]
    r = lambda a: rnd(a, dtype)                                                   # noqa: E731
    s = dict(z=r(g.standard_normal((C, D))), p=r(g.standard_normal((C, D))), g=r(g.standard_normal((C, D))),
             z0=r(g.standard_normal((C, D))), g0=r(g.standard_normal((C, D))), minv=r(g.uniform(0.5, 2.0, D)),
             U=g.uniform(1, 20, C), U0=g.uniform(1, 20, C), ke=g.uniform(1, 20, C), ke0=g.uniform(1, 20, C),
             eps=0.01 * 100.0 ** (np.arange(C) / max(C - 1, 1)) * g.uniform(0.9, 1.1, C),  # per chain, 100 x apart
             log_eps=g.uniform(-3, -1, C), failed=(np.arange(C) % 2).astype(np.int32),
             mu=g.uniform(0.5, 2.0, n_ode), sd=g.uniform(0.1, 0.5, n_ode),
             gnn=r(g.standard_normal((C, max(P, 1)))), gode=r(g.standard_normal((C, 17))), loss_sum=g.uniform(0, 30, C),
             nn_p=r(g.standard_normal((C, max(P, 1)))), ode_p=r(g.standard_normal((C, 17))))
    return s


# ------------------------------------------------------------------------------------------------ accept: one chain per edge
ACCEPT_EDGES = ("dH<0", "dH=0", "small+ keep", "positive reject", "dH=999.9", "dH=1000.1", "U=inf", "U=nan", "ke=nan",
                "failed dH<0")


def accept_edges(D, dtype, seed, it, n_ode=0):
    """One chain per edge of the Metropolis test; u is the chain's own Philox word, so dH is placed on either side of it."""
    C = len(ACCEPT_EDGES)
    s = chain_inputs(D, C, dtype, (0, 1, D), seed)
    g = np.random.default_rng(seed + 1)
    s["mu"], s["sd"] = g.uniform(0.5, 2.0, n_ode), g.uniform(0.1, 0.5, n_ode)
    s["failed"] = np.zeros(C, np.int32)
    u = np.array([R.uniform(seed, c, it, R.ACCEPT, 0) for c in range(C)])
    dH = np.array([-0.7, 0.0, -math.log((u[2] + 1) / 2), -math.log(u[3] / 2), 999.9, 1000.1, 0, 0, 0, -0.3])
    s["U"] = g.uniform(1, 20, C)
    s["ke"] = (s["U0"] + s["ke0"]) + dH - s["U"]
    s["U"][1], s["ke"][1] = s["U0"][1], s["ke0"][1]
    s["U"][6], s["U"][7], s["ke"][8] = math.inf, math.nan, math.nan
    s["failed"][9] = 1
    return s


def accept_edge_cases(D, dtype):
    """Every (mode, slot, draws given, seed, iteration, n_ode, inputs) the edges run with at this D."""
    n_ode = min(D, 3)
    n = 0
    for mode in (R.SAMPLE, R.ADAPT):
        for slot in (-1, 0, 2):
            for with_draws in (False, True):
                it = n % 4
                s = accept_edges(D, dtype, 40 + it, it, n_ode)
                C = s["z"].shape[0]
                s.update(da=np.random.default_rng(n).uniform(0.1, 1, (C, 4)) * [1, 1, 1, 0] + [0, 0, 0, n % 3],
                         search=np.zeros((C, 2), np.int32))
                yield mode, slot, with_draws, 40 + it, it, n_ode, s
                n += 1


SEQ_LAYOUTS = ((5, 7, 0), (1029, 1032, 0))                # where the search grid, the search and the adaptation sequences run
SEARCH_STATES = ((0, 0), (1, 0), (-1, 0), (1, 1), (-1, 1))
SEARCH_LW = ("above", "below", "failed", "nan")


def search_grid(D, dtype, seed):
    """Every (dir, done) state against every kind of log weight, one chain each."""
    C = len(SEARCH_STATES) * len(SEARCH_LW)
    s = chain_inputs(D, C, dtype, (0, 1, D), seed)
    s["failed"] = np.zeros(C, np.int32)
    s["search"] = np.array([st for st in SEARCH_STATES for _ in SEARCH_LW], np.int32)
    for c in range(C):
        kind = SEARCH_LW[c % 4]
        dH = {"above": 0.1, "below": 0.5}.get(kind, -0.2)
        s["ke"][c] = (s["U0"][c] + s["ke0"][c]) + dH - s["U"][c]
        if kind == "failed":
            s["failed"][c] = 1
        if kind == "nan":
            s["U"][c] = math.nan
    return s


# ------------------------------------------------------------------------------------------------ NUTS trees
class TreeCase:
    """C = 5 chains on a quadratic likelihood over the natural parameters: loss = sum a (theta - b)^2, so that
    U(z) = LIK_SCALE loss + |z|^2 / 2.  The step sizes run from one that reaches the depth limit to one that diverges."""
    C, it = 5, 3
    # out of chain order, so that the chains that stay active sit in slots below their own index
    EPS = {7: (0.45, 40.0, 0.8, 0.02, 1.1), 1029: (0.25, 40.0, 0.45, 0.004, 0.6), 2051: (0.3, 40.0, 0.45, 0.003, 0.6)}
    SEEDS = {7: 86, 1029: 116, 2051: 73}                   # seeds for which tests/test_chain_kernels_host.py finds every margin wide

    def __init__(self, layout, dtype, max_depth=4, seed=None):
        seed = self.SEEDS[layout[0]] if seed is None else seed
        self.layout, self.dtype, self.max_depth, self.seed = layout, dtype, max_depth, seed
        D = self.D = layout[0]
        self.cmap = (SPARSE_MASK, 1, D - 5) if D != 1029 else (THREE_MASK, 1, D - 3)
        self.n_ode, self.P = n_ode_of(self.cmap), self.cmap[2]
        g = np.random.default_rng(seed + D)
        r = lambda a: rnd(a, dtype)                                               # noqa: E731
        self.minv = r(g.uniform(0.5, 2.0, D))
        self.z = r(0.5 * g.standard_normal((self.C, D)))
        self.mu, self.sd = g.uniform(0.5, 2.0, self.n_ode), g.uniform(0.1, 0.5, self.n_ode)
        self.a_nn, self.b_nn = g.uniform(0.1, 0.6, self.P), 0.3 * g.standard_normal(self.P)
        self.a_ode, self.b_ode = g.uniform(0.5, 4.0, self.n_ode), self.mu + 0.1 * g.standard_normal(self.n_ode)
        self.log_eps = np.log(np.array(self.EPS[D]))
        self.idx = R.ode_indices(self.cmap[0])

    def likelihood(self, nn_p, ode_p, A):
        """gnn [C][P], gode [C][17], loss_sum [C] of the first A slots from the parameters pre wrote there; the slots past A
        and the unsampled constants hold values no chain may read."""
        C = self.C
        gnn, gode, loss = np.full((C, self.P), 1e30), np.full((C, 17), 1e30), np.full(C, 1e30)
        for s in range(A):
            dn, do = nn_p[s, :self.P] - self.b_nn, ode_p[s, self.idx] - self.b_ode
            loss[s] = math.fsum(self.a_nn * dn * dn) + math.fsum(self.a_ode * do * do)
            gnn[s] = LIK_SCALE * 2 * self.a_nn * dn
            gode[s, self.idx] = LIK_SCALE * 2 * self.a_ode * do
        return rnd(gnn, self.dtype), rnd(gode, self.dtype), loss

    def u_grad(self, z):
        """U, grad U of one chain in chain coordinates (for the transition-level restatement)."""
        th = z.copy()
        th[:self.n_ode] = self.mu + self.sd * z[:self.n_ode]
        do, dn = th[:self.n_ode] - self.b_ode, th[self.n_ode:] - self.b_nn
        U = LIK_SCALE * (math.fsum(self.a_ode * do * do) + math.fsum(self.a_nn * dn * dn)) + 0.5 * math.fsum(z * z)
        g = np.concatenate([LIK_SCALE * 2 * self.a_ode * do * self.sd, LIK_SCALE * 2 * self.a_nn * dn]) + z
        return U, g, False

    def start(self):
        """The state hode_hmc_refresh leaves: (z, g, U) at the start, fresh momenta, eps = exp(log_eps) (no jitter)."""
        C = self.C
        ug = [self.u_grad(self.z[c]) for c in range(C)]
        g, U = rnd(np.stack([x[1] for x in ug]), self.dtype), np.array([x[0] for x in ug])
        o = R.refresh(self.seed, self.it, 0.0, self.minv, self.log_eps, self.z, g, U)
        return dict(z=self.z, p=rnd(o["p"], self.dtype), g=g, U=U, U0=o["U0"], ke0=o["ke0"], eps=o["eps"])


class RefOps:
    """The calls of one tree through the restatement, every stored real rounded to the kernel's type: what the host file
    walks to check the margins, and what the GPU file compares each kernel call with."""

    def __init__(self, case):
        self.case, self.decisions = case, []

    def r(self, a):
        return rnd(a, self.case.dtype)

    def begin(self, st):
        T = R.nuts_begin(st["z"], st["p"], st["g"], st["U"], st["U0"], st["ke0"])
        T["ckpt_rows"] = np.full((self.case.C, self.case.max_depth, 2, self.case.D), np.nan)
        return T

    def compact(self, T):
        return R.nuts_compact(T["ist"])

    @staticmethod
    def ckpt_dict(rows):
        return {(c, k + 1): (rows[c, k, 0], rows[c, k, 1]) for c in range(rows.shape[0]) for k in range(rows.shape[1])}

    def pre(self, T, eps, rank):
        cs = self.case
        nn_p, ode_p = np.full((cs.C, max(cs.P, 1)), np.nan), np.full((cs.C, 17), np.nan)
        T2, nn_p, ode_p, dec = R.nuts_pre(T, cs.seed, cs.it, eps, cs.minv, rank, cs.cmap, cs.mu, cs.sd, nn_p, ode_p)
        self.decisions += dec
        T2["tree"], T2["ckpt_rows"] = self.r(T2["tree"]), T["ckpt_rows"]
        return T2, self.r(nn_p), self.r(ode_p)

    def post(self, T, eps, rank, gnn, gode, loss, status=None):
        cs = self.case
        Tin = dict(T, ckpt=self.ckpt_dict(T["ckpt_rows"]))
        T2, dec = R.nuts_post(Tin, cs.seed, cs.it, eps, cs.minv, rank, cs.cmap, cs.max_depth, cs.sd, gnn, gode, loss, LIK_SCALE, status)
        self.decisions += dec
        rows = T["ckpt_rows"].copy()
        for (c, k) in T2["written"]:
            rows[c, k - 1, 0], rows[c, k - 1, 1] = self.r(T2["ckpt"][(c, k)][0]), self.r(T2["ckpt"][(c, k)][1])
        T2["tree"], T2["ckpt_rows"] = self.r(T2["tree"]), rows
        return T2

    def finish(self, T, st):
        cs = self.case
        C = cs.C
        return R.nuts_finish(T, 0, 0.8, st["z"], st["g"], st["U"], cs.log_eps, np.zeros((C, 4)), cs.n_ode, cs.mu, cs.sd,
                             np.full((C, 2, cs.D), np.nan), np.full((C, 2, 6), np.nan), 1)


def drive_tree(case, ops):
    """begin, then (pre, the test's likelihood, post, compact) until no chain is active, then finish.  Returns the finish
    outputs and, per chain, the number of global steps it stayed active."""
    st = case.start()
    T = ops.begin(st)
    rank, count = ops.compact(T)
    alive = np.zeros(case.C, int)
    while count > 0:
        alive += rank >= 0
        T, nn_p, ode_p = ops.pre(T, st["eps"], rank)
        gnn, gode, loss = case.likelihood(nn_p, ode_p, count)
        T = ops.post(T, st["eps"], rank, gnn, gode, loss)
        rank, count = ops.compact(T)
    return ops.finish(T, st), T, alive


# ------------------------------------------------------------------------------------------------ accept: sequences
def accept_ref(mode, seed, it, s, n_ode=0, draws=None, stats=None, slot=-1, delta=0.8):
    """hode_hmc_accept of the state dict s through the restatement."""
    return R.accept(mode, seed, it, delta, s["z"], s["z0"], s["g"], s["g0"], s["U"], s["U0"], s["ke0"], s["ke"], s["failed"],
                    s["log_eps"], s["da"], s["search"], n_ode, s["mu"], s["sd"], draws, stats, slot)


SEARCH_START = (-3.0, -1.0, 0.5, 2.0, 3.0)


def drive_search(D, dtype, seed, call, trials=12):
    """The initial step-size search of five chains, one trial per call: dH = 0.05 (c + 1) eps^2 from the log_eps the previous
    call left, so the chains double or halve for different numbers of trials and then stay done.  call(it, s) -> outputs."""
    C = len(SEARCH_START)
    s = chain_inputs(D, C, dtype, (0, 1, D), seed)
    s.update(failed=np.zeros(C, np.int32), log_eps=np.array(SEARCH_START), da=np.zeros((C, 4)), search=np.zeros((C, 2), np.int32))
    history = []
    for it in range(trials):
        dH = 0.05 * (np.arange(C) + 1) * np.exp(2 * s["log_eps"])
        s["ke"] = (s["U0"] + s["ke0"]) + dH - s["U"]
        o = call(it, s)
        history.append((s["search"].copy(), s["log_eps"].copy(), o["search"].copy(), o["log_eps"].copy()))
        s = dict(s, z=o["z"], g=o["g"], U=o["U"], log_eps=o["log_eps"], search=o["search"])
        s["U"] = np.random.default_rng(seed + it).uniform(1, 20, C)
    return history


def drive_adapt(D, dtype, seed, call, n=50):
    """n ADAPT calls of three chains: fresh energies every call (dH in [-0.5, 2]), log_eps and da carried from the previous
    call's outputs.  call(it, s) -> outputs."""
    C = 3
    s = chain_inputs(D, C, dtype, (0, 1, D), seed)
    s.update(failed=np.zeros(C, np.int32), da=np.zeros((C, 4)), search=np.zeros((C, 2), np.int32))
    s["da"][:, 0] = math.log(10.0) + s["log_eps"]
    g = np.random.default_rng(seed + 5)
    out = []
    for it in range(n):
        s["U"], s["U0"], s["ke0"] = g.uniform(1, 20, C), g.uniform(1, 20, C), g.uniform(1, 20, C)
        s["ke"] = (s["U0"] + s["ke0"]) + g.uniform(-0.5, 2.0, C) - s["U"]
        o = call(it, s)
        out.append(o)
        s = dict(s, z=o["z"], g=o["g"], log_eps=o["log_eps"], da=o["da"])
    return out


def walk_status_slots(cs, ops):
    """Chains 1 and 3 are made inactive after begin, so chain 4 sits in slot 2.  One pre, then one post per (n_traj, slot)
    with a single failing status, the last trajectory of that slot.  Yields (n_traj, slot, the state after that post)."""
    st = cs.start()
    T = ops.begin(st)
    T["ist"][[1, 3], R.ACTIVE] = 0
    rank, count = ops.compact(T)
    T, nn_p, ode_p = ops.pre(T, st["eps"], rank)
    gnn, gode, loss = cs.likelihood(nn_p, ode_p, count)
    for n_traj in (1, 257, 300):
        for slot in (2, 4):
            status = np.zeros((cs.C, n_traj), np.int32)
            status[slot, -1] = 5
            yield n_traj, slot, rank, ops.post(T, st["eps"], rank, gnn, gode, loss, status)


def status_case(dtype):
    cs = TreeCase((7, 8, 0), dtype)
    cs.log_eps = np.log(np.full(5, 0.3))
    return cs
