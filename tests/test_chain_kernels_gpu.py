"""Every HMC and NUTS chain kernel (csrc/hode_hmc.hip, csrc/hode_nuts.hip, the ld4 / st4 helpers and chain reductions of
csrc/hode_chains.h) against the fp64 restatement of tests/_chain_reference.py, ONE call at a time, through hode.capi with raw
(C, D, ld) and carved buffers, so that every layout of tests/_chain_cases.py is reached: the scalar branch (ld % 4 != 0, or a
misaligned base), pads, a second pass of the row loop, tails of one.

Protocol.  The complete input state is set by hand from a seeded generator, one kernel call is made, everything is copied
back and compared with the restatement of that one call on the same inputs.  In a sequence (a tree, a search, 50 adaptation
steps) the restatement's next input is the KERNEL's read-back state, so rounding never compounds and a decision depends on
one call's arithmetic only; tests/test_chain_kernels_host.py asserts that every decision of every case here sits more than
100 rounding bounds from its threshold, so every flag and integer must be equal.

Every buffer is carved out of a larger allocation filled with a sentinel bit pattern: guard cells before and after, and for
the scalar layouts with ld > D inside the pad.  Whatever the restatement leaves unchanged must keep its bits.

Tolerances are derived, never measured: an entry computed from k roundings in unit roundoff u (2^-53; 2^-24 for the fp32
kernels' real-typed arithmetic) is held to (k + 1) u sum |terms|, the count written next to each bound.  Chain sums are
compared with math.fsum over the kernel's own stored rows (checked entry by entry first) to n_terms 2^-53 sum |terms|."""
import math

import numpy as np
import pytest
import torch

import hode
import _chain_cases as K
import _chain_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
cap = hode.capi
U64 = R.U64
GUARD = 64                                                   # cells: 256 or 512 bytes, keeps the carved base 16-byte aligned
_UINT = {4: np.uint32, 8: np.uint64}
_SENT = {np.dtype(np.float32): 0x7FC0DEAD, np.dtype(np.float64): 0x7FF8DEADBEEF0123, np.dtype(np.int32): 0x5A5A5A5A}
DT = pytest.mark.parametrize("dtype", K.DTYPES, ids=["f32", "f64"])
LAY = pytest.mark.parametrize("layout", K.LAYOUTS, ids=str)


def _bits(a):
    return np.ascontiguousarray(a).view(_UINT[a.dtype.itemsize])


class Buf:
    """rows x D logical cells at row stride ld, `off` cells into an allocation of sentinels with guards on both sides."""

    def __init__(self, data, dtype, shape=None, ld=None, off=0, pad_in=None, pad_out=None):
        dtype = np.dtype(dtype)
        self.shape = tuple(shape if data is None else np.shape(data))
        rows, D = (1, int(np.prod(self.shape))) if len(self.shape) != 2 or ld is None else self.shape
        self.rows, self.D, self.ld, self.lo, self.pad_out = rows, D, ld or D, GUARD + off, pad_out
        h = np.empty(GUARD + off + rows * self.ld + GUARD, dtype)
        _bits(h)[:] = _SENT[dtype]
        body = h[self.lo:self.lo + rows * self.ld].reshape(rows, self.ld)
        if pad_in is not None:
            body[:, D:] = pad_in
        if data is not None:
            body[:, :D] = np.asarray(data).reshape(rows, D)
        self.before = h.copy()
        self.dev = torch.from_numpy(h).to(DEV)
        self.t = self.dev[self.lo:self.lo + rows * self.ld]

    def read(self):
        """The logical cells after the call; the guards and the pad keep their bits (or hold exactly pad_out)."""
        a = self.dev.cpu().numpy()
        hi = self.lo + self.rows * self.ld
        assert np.array_equal(_bits(a[:self.lo]), _bits(self.before[:self.lo])), "guard before the buffer"
        assert np.array_equal(_bits(a[hi:]), _bits(self.before[hi:])), "guard after the buffer"
        body, was = a[self.lo:hi].reshape(self.rows, self.ld), self.before[self.lo:hi].reshape(self.rows, self.ld)
        if self.pad_out is None:
            assert np.array_equal(_bits(body[:, self.D:]), _bits(was[:, self.D:])), "pad cells"
        else:
            assert np.array_equal(_bits(body[:, self.D:]), _bits(np.full_like(body[:, self.D:], self.pad_out))), "pad value"
        return body[:, :self.D].reshape(self.shape).copy()

    def untouched(self):
        assert np.array_equal(_bits(self.dev.cpu().numpy()), _bits(self.before)), "an input buffer was written"


class Frame:
    """The buffers of one kernel call in one layout."""

    def __init__(self, layout, dtype):
        self.D, self.ld, self.off = layout
        self.dtype, self.vec = np.dtype(dtype), K.is_vec(layout, dtype)
        self.b = {}

    def rows(self, name, data, kind="z", nrows=None):
        """Row data [r][D] (None: nrows rows of sentinels).  Pads of the vector layouts: z-like rows hold 0 before and after,
        minv holds 1, an output-only buffer holds sentinels before and 0 after; scalar layouts keep their sentinels."""
        pin, pout = {"z": (0.0, 0.0), "minv": (1.0, 1.0), "out": (None, 0.0), "junk": (3.0, 3.0)}[kind] if self.vec else (None, None)
        if data is not None:
            data = np.asarray(data).reshape(-1, self.D)
        self.b[name] = Buf(data, self.dtype, shape=(nrows, self.D), ld=self.ld, off=self.off, pad_in=pin, pad_out=pout)
        return self.b[name].t

    def flat(self, name, data, dtype=np.float64, shape=None):
        if data is None and shape is None:
            return None                                      # a NULL pointer
        self.b[name] = Buf(None if data is None else np.asarray(data), dtype, shape=shape)
        return self.b[name].t

    def real(self, name, data, shape=None):
        return self.flat(name, data, self.dtype, shape)

    def read(self, *names):
        torch.cuda.synchronize()
        return {n: self.b[n].read() for n in names}

    def inputs_untouched(self, *names):
        for n in names:
            if n in self.b:
                self.b[n].untouched()


def same_bits(a, b, what):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def three_ways(run, layout, dtype):
    """run(layout) on the layout, again (same bits), and through the other path with the same D (same bits)."""
    o = run(layout)
    same_bits(o, run(layout), "two identical calls")
    same_bits(o, run(K.partner(layout, dtype)), "vector and scalar path")
    return o


def check(name, got, want, before=None, tol=0.0):
    """got within tol of want; where the restatement leaves `before` unchanged, got must equal it exactly; a non-finite want
    must be met exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    if before is not None:
        before = np.asarray(before, np.float64)
        keep = (want == before) | (np.isnan(want) & np.isnan(before))
        assert np.array_equal(got[keep], before[keep], equal_nan=True), (name, "a cell the call must not change", np.argwhere(keep & ~((got == before) | (np.isnan(got) & np.isnan(before))))[:4])
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (name, "non-finite")
    err = np.abs(got[fin] - want[fin])
    bad = err > tol[fin]
    if bad.any():
        worst = int(np.argmax(err - tol[fin]))
        raise AssertionError(f"{name}: {int(bad.sum())} entries past their bound, worst at {np.argwhere(fin)[worst].tolist()}: got {got[fin][worst]!r}, "
                             f"want {want[fin][worst]!r}, error {err[worst]:.3e}, bound {tol[fin][worst]:.3e}")


def sum_check(name, got, terms, extra=0.0, scale=1.0):
    """A chain sum the kernel took in fp64 against math.fsum over the same stored terms: n_terms u64 sum |terms| (+ the
    products' roundings: 3 per term)."""
    terms = np.asarray(terms, np.float64).ravel()
    want = scale * math.fsum(terms) + extra
    tol = (terms.size + 3) * U64 * (abs(scale) * math.fsum(np.abs(terms)) + abs(extra))
    assert abs(got - want) <= tol, (name, got, want, tol)


# ------------------------------------------------------------------------------------------------ refresh
def run_refresh(layout, dtype, s, seed, it, jitter):
    f = Frame(layout, dtype)
    C = s["z"].shape[0]
    args = (f.rows("minv", s["minv"], "minv"), f.flat("log_eps", s["log_eps"]), f.rows("z", s["z"]), f.rows("g", s["g"]), f.flat("U", s["U"]),
            f.rows("p", None, "out", C), f.rows("z0", None, "out", C), f.rows("g0", None, "out", C), f.flat("U0", None, shape=(C,)),
            f.flat("ke0", None, shape=(C,)), f.flat("eps", None, shape=(C,)), f.flat("failed", np.full(C, 7), np.int32))
    cap.hmc_refresh(C, f.D, f.ld, seed, it, jitter, *args)
    o = f.read("p", "z0", "g0", "U0", "ke0", "eps", "failed")
    f.inputs_untouched("minv", "log_eps", "z", "g", "U")
    return o


@LAY
@DT
def test_refresh(layout, dtype):
    D, u = layout[0], R.unit(dtype)
    base = K.chain_inputs(D, 5, dtype, (0, 1, D), 11)
    p_of = {}
    for i, C in enumerate(K.CHAINS):
        s = {k: (v[:C] if k != "minv" else v) for k, v in base.items() if k in ("minv", "log_eps", "z", "g", "U")}
        seed, it, jitter = 0x1234567890ABCDEF, 1000 + i % 2, (0.0, 0.1)[i % 2]
        o = three_ways(lambda lay: run_refresh(lay, dtype, s, seed, it, jitter), layout, dtype)
        want = R.refresh(seed, it, jitter, s["minv"], s["log_eps"], s["z"], s["g"], s["U"])
        # p = (R)(xi / sqrt(minv)): xi = r cos(a) in fp64 with r <= sqrt(-2 log 2^-33) = 6.77; roundings in units of u64: u01 1,
        # log 2 (1 ulp), the radius 2, the angle 7 (its absolute error 2 pi u moves cos by as much), cos 4 (2 ulp), the product
        # 1, sqrt(minv) 1, the quotient 1 = 19; then the rounding to R
        tol_p = 20 * U64 * 6.77 / np.sqrt(s["minv"]) + (2 * u * np.abs(want["p"]) if dtype == np.float32 else 0.0)
        check("p", o["p"], want["p"], tol=tol_p)
        check("z0", o["z0"], s["z"])
        check("g0", o["g0"], s["g"])
        check("U0", o["U0"], s["U"])
        assert not o["failed"].any()
        for c in range(C):
            pc = o["p"][c].astype(np.float64)
            sum_check("ke0", o["ke0"][c], pc * pc * s["minv"], scale=0.5)
        # eps = exp(log_eps) (1 + jitter (2 u - 1)): exp 2, the bracket 3, the product 1
        check("eps", o["eps"], want["eps"], tol=7 * U64 * np.abs(want["eps"]) * 2)
        if jitter == 0.0:
            check("eps without jitter", o["eps"], np.exp(s["log_eps"]), tol=3 * U64 * np.exp(s["log_eps"]))
        p_of[(C, it)] = o["p"]
    # a chain's momentum does not depend on C: chain 0 of C = 1 and of C = 5 (same iteration)
    assert np.array_equal(_bits(p_of[(1, 1000)][0]), _bits(p_of[(5, 1000)][0]))
    s3 = {k: (v[:3] if k != "minv" else v) for k, v in base.items() if k in ("minv", "log_eps", "z", "g", "U")}
    o3 = run_refresh(layout, dtype, s3, 0x1234567890ABCDEF, 1000, 0.0)
    assert np.array_equal(_bits(o3["p"][2]), _bits(p_of[(5, 1000)][2]))


# ------------------------------------------------------------------------------------------------ leapfrog
def run_leapfrog(layout, dtype, s, flags, kick, cmap, nulls, status, pg_kind="z"):
    f = Frame(layout, dtype)
    C = s["z"].shape[0]
    mask, sample_nn, P = cmap
    n_traj = 0 if status is None else status.shape[1]
    get = lambda k: None if k in nulls else s[k]             # noqa: E731
    args = (f.flat("eps", s["eps"]), f.rows("minv", s["minv"], "minv"), f.rows("z", s["z"]), f.rows("p", s["p"], pg_kind), f.rows("g", s["g"], pg_kind),
            f.real("gnn", get("gnn")), f.real("gode", get("gode")), P, f.flat("loss_sum", get("loss_sum")), K.LIK_SCALE,
            f.flat("status", status, np.int32), n_traj, f.flat("U", s["U"]), f.flat("ke", s["ke"]), f.flat("failed", s["failed"], np.int32),
            mask, f.flat("mu", s["mu"] if len(s["mu"]) else None), f.flat("sd", s["sd"] if len(s["sd"]) else None), sample_nn,
            f.real("nn_p", s["nn_p"]), f.real("ode_p", s["ode_p"]))
    cap.hmc_leapfrog(C, f.D, f.ld, flags, kick, *args)
    o = f.read("z", "p", "g", "U", "ke", "failed", "nn_p", "ode_p")
    f.inputs_untouched("eps", "minv", "gnn", "gode", "loss_sum", "status", "mu", "sd")
    return o


A_, K_, D_, E_, P_ = R.ASSEMBLE, R.KICK, R.DRIFT, R.KE, R.PARAMS
LEAPFROG_FLAGS = (K_ | D_, A_ | K_ | D_, A_ | K_ | E_, A_, P_, A_ | K_ | E_ | D_, K_ | E_)
LEAPFROG_NULLS = ((), ("gnn", "gode"), ("gode",), ("loss_sum",), ("gnn", "gode", "loss_sum"))


def check_params(o, s, cmap, u, written):
    """nn_p / ode_p: the sampled entries from the kernel's own stored z (nn_p its bits; ode_p = (R)(mu + sd z): the product,
    the sum and the rounding to R, (1 + 1) u (|mu| + |sd z|) + 3 u64 of the same), every other entry untouched."""
    n_ode, P = K.n_ode_of(cmap), cmap[2]
    idx = R.ode_indices(cmap[0])
    want_nn, want_ode, tol_ode = s["nn_p"].copy(), s["ode_p"].copy(), np.zeros_like(s["ode_p"])
    if written:
        z = o["z"].astype(np.float64)
        if cmap[1]:
            want_nn[:, :P] = z[:, n_ode:]
        want_ode[:, idx] = s["mu"] + s["sd"] * z[:, :n_ode]
        tol_ode[:, idx] = (2 * u + 3 * U64) * (np.abs(s["mu"]) + np.abs(s["sd"] * z[:, :n_ode]))
    check("nn_p", o["nn_p"], want_nn)
    check("ode_p", o["ode_p"], want_ode, s["ode_p"], tol_ode)


@LAY
@DT
def test_leapfrog(layout, dtype):
    D, u = layout[0], R.unit(dtype)
    n = 0
    for cmap in K.maps_for(D):
        n_ode = K.n_ode_of(cmap)
        for flags in LEAPFROG_FLAGS:
            C, kick = K.CHAINS[n % 3], (0.5, 1.0)[n % 2]
            nulls = LEAPFROG_NULLS[n % 5] if flags & A_ else ()
            n_traj = K.N_TRAJ[n % 4]
            status = K.status_array(C, n_traj, hit=n % 3 != 1)
            s = K.chain_inputs(D, C, dtype, cmap, 100 + n)
            n += 1
            o = three_ways(lambda lay: run_leapfrog(lay, dtype, s, flags, kick, cmap, nulls, status), layout, dtype)
            gnn, gode, loss = (None if k in nulls else s[k] for k in ("gnn", "gode", "loss_sum"))
            w = R.leapfrog(flags, kick, s["eps"], s["minv"], s["z"], s["p"], s["g"], s["U"], s["ke"], s["failed"], cmap, s["mu"], s["sd"],
                           gnn, gode, loss, K.LIK_SCALE, status, s["nn_p"], s["ode_p"])
            lik = np.abs(np.stack([R._lik_grad(c, D, cmap, s["sd"], gnn, gode) for c in range(C)])) if flags & A_ else 0.0
            # g = lik + z with lik = gode (R)sd for a constant (the conversion, the product, the sum: 3) or gnn (the sum: 1)
            k_g = np.where(np.arange(D) < n_ode, 3, 1) if flags & A_ else 0
            mag_g = lik + np.abs(s["z"]) if flags & A_ else np.abs(s["g"])
            check("g", o["g"], w["g"], s["g"], (k_g + 1) * u * mag_g)
            # p -= ek g, ek = (R)(kick eps): the conversion, the product, the difference: 3, on top of g's
            ek = np.abs(kick * s["eps"])[:, None]
            k_p = 3 + k_g if flags & K_ else 0
            mag_p = np.abs(s["p"]) + (ek * mag_g if flags & K_ else 0.0)
            check("p", o["p"], w["p"], s["p"], (k_p + 1) * u * mag_p)
            # z += ed minv p, ed = (R)eps: the conversion, two products, the sum: 4, on top of p's
            ed = np.abs(s["eps"])[:, None]
            check("z", o["z"], w["z"], s["z"], (k_p + 4 + 1) * u * (np.abs(s["z"]) + ed * s["minv"] * mag_p))
            check("failed", o["failed"], w["failed"])
            assert ((o["failed"] != 0) >= (s["failed"] != 0)).all()           # only ever set
            for c in range(C):
                if flags & A_:
                    zc = s["z"][c]
                    sum_check("U", o["U"][c], zc * zc, extra=K.LIK_SCALE * loss[c] if loss is not None else 0.0, scale=0.5)
                if flags & E_:
                    pc = o["p"][c].astype(np.float64)
                    sum_check("ke", o["ke"][c], pc * pc * s["minv"], scale=0.5)
            if not flags & A_:
                check("U", o["U"], s["U"])
            if not flags & E_:
                check("ke", o["ke"], s["ke"])
            check_params(o, s, cmap, u, bool(flags & (D_ | P_)))


@pytest.mark.parametrize("layout", [(3, 4, 0), (7, 8, 0), (1029, 1032, 0)], ids=str)
@DT
def test_leapfrog_ke_ignores_the_pads_of_p_and_g(layout, dtype):
    """include/hode.h fixes the pads of z (0) and minv (1) only: whatever the pads of p and g hold stays out of ke."""
    D = layout[0]
    s = K.chain_inputs(D, 3, dtype, (0, 1, D), 9)
    o = run_leapfrog(layout, dtype, s, E_, 1.0, (0, 1, D), (), None, pg_kind="junk")
    for c in range(3):
        sum_check("ke", o["ke"][c], s["p"][c] * s["p"][c] * s["minv"], scale=0.5)
    for k in ("z", "p", "g", "U", "failed", "nn_p", "ode_p"):
        check(k, o[k], s[k])


# ------------------------------------------------------------------------------------------------ accept
def run_accept(layout, dtype, s, mode, seed, it, n_ode=0, draws=None, stats=None, n_slots=0, slot=-1):
    f = Frame(layout, dtype)
    C = s["z"].shape[0]
    args = (f.rows("z", s["z"]), f.rows("z0", s["z0"]), f.rows("g", s["g"]), f.rows("g0", s["g0"]), f.flat("U", s["U"]), f.flat("U0", s["U0"]),
            f.flat("ke0", s["ke0"]), f.flat("ke", s["ke"]), f.flat("failed", s["failed"], np.int32), f.flat("log_eps", s["log_eps"]),
            f.flat("da", s["da"]), f.flat("search", s["search"], np.int32), n_ode, f.flat("mu", s["mu"] if n_ode else None),
            f.flat("sd", s["sd"] if n_ode else None), f.real("draws", draws), f.flat("stats", stats), n_slots, slot)
    cap.hmc_accept(C, f.D, f.ld, mode, seed, it, 0.8, *args)
    o = f.read("z", "g", "U", "log_eps", "da", "search", *(["draws"] if draws is not None else []), *(["stats"] if stats is not None else []))
    f.inputs_untouched("z0", "g0", "U0", "ke0", "ke", "failed", "mu", "sd")
    return o


def da_tolerance(da_in, a, tol_a, delta=0.8):
    """Bounds of one dual-averaging update, in units of u64: H bar = (1 - eta) H bar + eta (delta - a): eta 2, the two
    products, the two differences, the sum = 7; log eps = mu - sqrt(t) / 0.05 H bar: sqrt, quotient, product, difference = 4
    on top of H bar's; log eps bar = w le + (1 - w) bar with w = pow (2 ulp = 4): 4 + 4 on top of le's."""
    t = da_in[:, 3] + 1
    eta, amp = 1 / (t + 10), np.sqrt(t) / 0.05
    hb = (1 - eta) * da_in[:, 2] + eta * (delta - a)
    t_h = 8 * U64 * (np.abs(da_in[:, 2]) + delta + np.abs(a)) + eta * tol_a
    le = da_in[:, 0] - amp * hb
    t_le = 5 * U64 * (np.abs(da_in[:, 0]) + amp * np.abs(hb)) + amp * t_h
    t_bar = 9 * U64 * (np.abs(le) + np.abs(da_in[:, 1])) + t_le
    return np.stack([np.zeros_like(t), t_bar, t_h, np.zeros_like(t)], axis=1), t_le


def compare_accept(o, s, w, mode, u, n_ode, slot, tol_a):
    check("z", o["z"], w["z"], s["z"])
    check("g", o["g"], w["g"], s["g"])
    check("U", o["U"], w["U"], s["U"])
    check("search", o["search"], w["search"])
    if mode == R.ADAPT:
        t_da, t_le = da_tolerance(s["da"], w["stats_a"], tol_a)
        check("da", o["da"], w["da"], s["da"], t_da)
        check("log_eps", o["log_eps"], w["log_eps"], s["log_eps"], t_le)
    elif mode == R.SEARCH:
        check("da", o["da"], s["da"])
        check("log_eps", o["log_eps"], w["log_eps"], s["log_eps"], 3 * U64 * (np.abs(s["log_eps"]) + math.log(2)))   # += dir log 2: 2
    else:
        check("da", o["da"], w["da"], s["da"], 3 * U64 * (math.log(10) + np.abs(s["log_eps"]))[:, None] if mode == R.DA_RESTART else 0.0)
        check("log_eps", o["log_eps"], w["log_eps"], s["log_eps"])
    if "stats" in o:
        t = np.zeros_like(w["stats"])
        if slot >= 0:
            t[:, slot, 0] = tol_a
        check("stats", o["stats"], w["stats"], s["stats_in"], t)
    if "draws" in o:
        # natural coordinates of the kernel's own kept z: (R)(mu + sd z), (1 + 1) u (|mu| + |sd z|) + 3 u64; the weights: bits
        want, t = s["draws_in"].copy(), np.zeros_like(s["draws_in"])
        if slot >= 0 and mode in (R.SAMPLE, R.ADAPT):
            z = o["z"].astype(np.float64)
            want[:, slot] = z
            want[:, slot, :n_ode] = s["mu"] + s["sd"] * z[:, :n_ode]
            t[:, slot, :n_ode] = (2 * u + 3 * U64) * (np.abs(s["mu"]) + np.abs(s["sd"] * z[:, :n_ode]))
        check("draws", o["draws"], want, s["draws_in"], t)


def accept_call(layout, dtype, s, mode, seed, it, n_ode=0, with_draws=False, n_slots=0, slot=-1):
    """One hode_hmc_accept call three ways against the restatement; returns the kernel's outputs."""
    C, D, u = s["z"].shape[0], layout[0], R.unit(dtype)
    g = np.random.default_rng(7)
    stats_in = g.standard_normal((C, n_slots, 4)) if n_slots else None
    draws_in = K.rnd(g.standard_normal((C, n_slots, D)), dtype) if with_draws else None
    s = dict(s, stats_in=stats_in, draws_in=draws_in)
    o = three_ways(lambda lay: run_accept(lay, dtype, s, mode, seed, it, n_ode, draws_in, stats_in, n_slots, slot), layout, dtype)
    w = K.accept_ref(mode, seed, it, s, n_ode, draws_in, stats_in, slot)
    # the accept probability a = exp(-dH), dH from four energies in fp64 (3): a (4 u64 sum |energies|) + exp's 2 u64 a
    dH = (s["U"] + s["ke"]) - (s["U0"] + s["ke0"])
    ok = np.isfinite(dH) & (dH > 0) & (dH <= 1000) & (s["failed"] == 0)
    a = np.where(ok, np.exp(-np.where(ok, dH, 0.0)), np.where(np.isfinite(dH) & (dH <= 0) & (s["failed"] == 0) & np.isfinite(s["U"] + s["ke"]), 1.0, 0.0))
    energies = np.where(ok, np.abs(s["U"]) + np.abs(s["ke"]) + np.abs(s["U0"]) + np.abs(s["ke0"]), 0.0)
    tol_a = a * 4 * U64 * energies + 2 * U64 * a * ok
    w["stats_a"] = a
    compare_accept(o, s, w, mode, u, n_ode, slot, tol_a)
    return o


@LAY
@DT
def test_accept_edges(layout, dtype):
    for mode, slot, with_draws, seed, it, n_ode, s in K.accept_edge_cases(layout[0], dtype):
        accept_call(layout, dtype, s, mode, seed, it, n_ode, with_draws, 3, slot)


SEQ_LAYOUTS = pytest.mark.parametrize("layout", K.SEQ_LAYOUTS, ids=str)


@SEQ_LAYOUTS
@DT
def test_accept_search_grid_and_sequence(layout, dtype):
    D = layout[0]
    s = K.search_grid(D, dtype, 50)
    s["da"] = np.random.default_rng(2).standard_normal((s["z"].shape[0], 4))
    o = accept_call(layout, dtype, s, R.SEARCH, 50, 0, with_draws=True, n_slots=2, slot=1)     # SEARCH stores no draws
    # direction 0 takes the side of log 0.8 the weight is on, and never stops in the same trial it starts
    for c in range(4):
        assert tuple(o["search"][c]) == ((1, 0) if K.SEARCH_LW[c] == "above" else (-1, 0)), (c, o["search"][c])
    history = K.drive_search(D, dtype, 60, lambda it, st: accept_call(layout, dtype, st, R.SEARCH, 60, it))
    done_at = [next(i for i, h in enumerate(history) if h[2][c, 1]) for c in range(len(K.SEARCH_START))]
    assert len(set(done_at)) >= 3 and max(done_at) < 11, done_at
    for c, d in enumerate(done_at):                       # after done, nothing changes
        for h in history[d + 1:]:
            assert np.array_equal(h[2][c], history[d][2][c]) and h[3][c] == history[d][3][c]


@SEQ_LAYOUTS
@DT
def test_accept_adapt_sequence_restart_finish(layout, dtype):
    D = layout[0]
    outs = K.drive_adapt(D, dtype, 61, lambda it, st: accept_call(layout, dtype, st, R.ADAPT, 61, it, n_slots=1, slot=0))
    assert (outs[-1]["da"][:, 3] == 50).all()
    C = 3
    s = K.chain_inputs(D, C, dtype, (0, 1, D), 62)
    s.update(da=np.random.default_rng(3).standard_normal((C, 4)), search=np.array([[1, 1], [-1, 0], [0, 0]], np.int32))
    o = accept_call(layout, dtype, s, R.DA_RESTART, 0, 0)
    assert not o["search"].any() and not o["da"][:, 1:].any()
    s["da"][:, 3] = [0, 3, 50]                              # DA_FINISH: t = 0 leaves log_eps, t > 0 takes the average
    o = accept_call(layout, dtype, s, R.DA_FINISH, 0, 0)
    assert o["log_eps"][0] == s["log_eps"][0] and (o["log_eps"][1:] == s["da"][1:, 1]).all()


# ------------------------------------------------------------------------------------------------ welford
def run_welford(dtype, D, ld, flags, z, wf, minv):
    f = Frame((D, ld, 0), dtype)
    f.vec = False                                           # the kernel addresses single cells: pads keep their sentinels
    C = 1 if z is None else z.shape[0]
    args = (f.rows("z", z, nrows=C), f.flat("wf", wf), f.rows("minv", minv))
    cap.hmc_welford(C, D, ld, flags, *args)
    o = f.read("wf", "minv")
    f.inputs_untouched("z")
    return o


@pytest.mark.parametrize("D", [1, 64, 65, 130])
@DT
def test_welford(D, dtype):
    ld, u = D + 3, R.unit(dtype)
    g = np.random.default_rng(D)

    def step(flags, z, wf, minv):
        o = run_welford(dtype, D, ld, flags, z, wf, minv)
        same_bits(o, run_welford(dtype, D, ld, flags, z, wf, minv), "two identical calls")
        w_wf, w_minv = R.welford(flags, z, wf, minv[0])
        if flags & R.W_ACCUM and not flags & R.W_FINISH:
            # n exact; the mean: C updates of 3 roundings each, (3 C + 1) u64 max |x|; M2: its terms dl (x - m), each factor
            # off by the mean's bound d_m: sum (|dl| + |x - m| + d_m) d_m + (3 C + 1) u64 M2
            C, xm = z.shape[0], np.abs(z).max(0)
            d_m = (3 * (C + wf[0]) + 1) * U64 * np.maximum(xm, np.abs(wf[1]))
            dev = np.abs(z - w_wf[1]).sum(0) + np.abs(wf[1] - w_wf[1]) * wf[0]
            check("wf", o["wf"], w_wf, tol=np.stack([np.zeros(D), d_m, (2 * dev + d_m) * d_m * (C + wf[0]) + (3 * C + 1) * U64 * w_wf[2]]))
            check("minv", o["minv"], minv)
        return o, w_wf, w_minv

    # three chains, three ACCUM calls, then FINISH: values of order 1e4 with spread 1e-2
    wf, minv = np.zeros((3, D)), K.rnd(g.uniform(0.5, 2, (1, D)), dtype)
    rows = []
    for _ in range(3):
        z = K.rnd(1e4 + 1e-2 * g.standard_normal((3, D)), dtype)
        rows.append(z)
        o, _, _ = step(R.W_ACCUM, z, wf, minv)
        wf = o["wf"]
    assert (wf[0] == 9).all()
    pooled = np.concatenate(rows)
    var = pooled.var(0, ddof=1)
    # against numpy on the pooled rows: the two-pass variance of 9 values near 1e4 carries 9 u64 1e4 per deviation
    d_dev = 20 * U64 * 1e4
    t_var = (2 * np.abs(pooled - pooled.mean(0)).sum(0) * d_dev + 9 * d_dev ** 2) / 8 + 30 * U64 * var
    check("M2 / (n - 1) against numpy.var", wf[2] / 8, var, tol=t_var)
    o = run_welford(dtype, D, ld, R.W_FINISH, None, wf, minv)
    # minv = (R)(n / (n + 5) var + 1e-3 5 / (n + 5)) from the kernel's own M2: 7 roundings in fp64, one in R
    want = 9 / 14 * (wf[2] / 8) + 1e-3 * 5 / 14
    check("minv", o["minv"][0], want, tol=(2 * u if dtype == np.float32 else 0) * want + 8 * U64 * want)
    assert not o["wf"].any()
    # accumulate and finish in one call, from the pooled rows
    o2 = run_welford(dtype, D, ld, R.W_ACCUM | R.W_FINISH, pooled, np.zeros((3, D)), minv)
    check("minv, one call", o2["minv"][0], 9 / 14 * var + 1e-3 * 5 / 14, tol=9 / 14 * t_var + (2 * u if dtype == np.float32 else 0) * want + 8 * U64 * want)
    assert not o2["wf"].any()
    # one chain alone: n = 1, FINISH leaves minv untouched and still resets
    o1 = run_welford(dtype, D, ld, R.W_ACCUM, rows[0][:1], np.zeros((3, D)), minv)
    check("wf of one row", o1["wf"], np.stack([np.ones(D), rows[0][0], np.zeros(D)]), tol=np.stack([np.zeros(D), U64 * rows[0][0], np.zeros(D)]))
    o1 = run_welford(dtype, D, ld, R.W_FINISH, None, o1["wf"], minv)
    check("minv after n = 1", o1["minv"], minv)
    assert not o1["wf"].any()
    o1 = run_welford(dtype, D, ld, R.W_ACCUM | R.W_FINISH, rows[0][:1], np.zeros((3, D)), minv)
    check("minv after n = 1, one call", o1["minv"], minv)
    assert not o1["wf"].any()


# ------------------------------------------------------------------------------------------------ nuts_compact
@pytest.mark.parametrize("C", K.COMPACT_C)
def test_nuts_compact(C):
    for pattern in K.COMPACT_PATTERNS:
        ist = K.compact_pattern(C, pattern)
        outs = []
        for _ in range(2):
            f = Frame((1, 1, 0), np.float64)
            cap.nuts_compact(C, f.flat("ist", ist, np.int32), f.flat("rank", np.full(C, 99), np.int32), f.flat("count", np.full(1, 99), np.int32))
            outs.append(f.read("rank", "count"))
            f.inputs_untouched("ist")
        same_bits(outs[0], outs[1], "two identical calls")
        rank, count = R.nuts_compact(ist)
        on = ist[:, R.ACTIVE] != 0
        assert np.array_equal(outs[0]["rank"], rank) and int(outs[0]["count"][0]) == count == int(on.sum()), (C, pattern)
        assert (rank[~on] == -1).all() and np.array_equal(rank[on], np.arange(count))   # exclusive count in chain order


# ------------------------------------------------------------------------------------------------ nuts: begin / pre / post / finish
def run_begin(layout, dtype, st, tree0, dst0, ist0):
    f = Frame(layout, dtype)
    C = st["z"].shape[0]
    args = (f.rows("z", st["z"]), f.rows("p", st["p"]), f.rows("g", st["g"]), f.flat("U", st["U"]), f.flat("U0", st["U0"]), f.flat("ke0", st["ke0"]),
            f.rows("tree", tree0), f.flat("dst", dst0), f.flat("ist", ist0, np.int32))
    cap.nuts_begin(C, f.D, f.ld, *args)
    o = f.read("tree", "dst", "ist")
    f.inputs_untouched("z", "p", "g", "U", "U0", "ke0")
    return o


def run_pre(layout, dtype, cs, T, eps, rank, nn0, ode0):
    f = Frame(layout, dtype)
    mask, sample_nn, P = cs.cmap
    args = (f.flat("eps", eps), f.rows("minv", cs.minv, "minv"), f.rows("tree", T["tree"]), f.flat("ist", T["ist"], np.int32),
            f.flat("rank", rank, np.int32), mask, f.flat("mu", cs.mu), f.flat("sd", cs.sd), sample_nn, P, f.real("nn_p", nn0), f.real("ode_p", ode0))
    cap.nuts_pre(cs.C, f.D, f.ld, cs.seed, cs.it, *args)
    o = f.read("tree", "ist", "nn_p", "ode_p")
    f.inputs_untouched("eps", "minv", "rank", "mu", "sd")
    return o


def run_post(layout, dtype, cs, T, eps, rank, gnn, gode, loss, status):
    f = Frame(layout, dtype)
    mask, sample_nn, P = cs.cmap
    n_traj = 0 if status is None else status.shape[1]
    args = (f.flat("eps", eps), f.rows("minv", cs.minv, "minv"), f.rows("tree", T["tree"]), f.rows("ckpt", T["ckpt_rows"]), f.flat("dst", T["dst"]),
            f.flat("ist", T["ist"], np.int32), f.flat("rank", rank, np.int32), f.real("gnn", gnn), f.real("gode", gode), P, f.flat("loss_sum", loss),
            K.LIK_SCALE, f.flat("status", status, np.int32), n_traj, mask, f.flat("sd", cs.sd), sample_nn)
    cap.nuts_post(cs.C, f.D, f.ld, cs.max_depth, cs.seed, cs.it, *args)
    o = f.read("tree", "ckpt", "dst", "ist")
    f.inputs_untouched("eps", "minv", "rank", "gnn", "gode", "loss_sum", "status", "sd")
    return o


def run_finish(layout, dtype, cs, T, st, adapt, log_eps, da, draws, stats, n_slots, slot):
    f = Frame(layout, dtype)
    args = (f.rows("z", st["z"]), f.rows("g", st["g"]), f.flat("U", st["U"]), f.rows("tree", T["tree"]), f.flat("dst", T["dst"]),
            f.flat("ist", T["ist"], np.int32), f.flat("log_eps", log_eps), f.flat("da", da), cs.n_ode, f.flat("mu", cs.mu), f.flat("sd", cs.sd),
            f.real("draws", draws), f.flat("stats", stats), n_slots, slot)
    cap.nuts_finish(cs.C, f.D, f.ld, adapt, 0.8, *args)
    o = f.read("z", "g", "U", "log_eps", "da", *(["draws"] if draws is not None else []), *(["stats"] if stats is not None else []))
    f.inputs_untouched("tree", "dst", "ist", "mu", "sd")
    return o


class KernelOps(K.RefOps):
    """Every call of a tree on the GPU, three ways, against the restatement of that call on the same inputs; the state handed
    on is the kernel's."""

    def __init__(self, case, layout):
        super().__init__(case)
        self.layout, self.u, self.g = layout, R.unit(case.dtype), np.random.default_rng(5)
        self.calls = 0

    def state(self, o, T, **more):
        return dict(T, tree=o["tree"].astype(np.float64).reshape(15, self.case.C, self.case.D), ist=o["ist"], **more)

    def begin(self, st):
        cs = self.case
        C, D = cs.C, cs.D
        tree0, dst0 = self.r(self.g.standard_normal((15, C, D))), self.g.standard_normal((C, 8))
        ist0 = self.g.integers(-9, 9, (C, 8)).astype(np.int32)
        o = three_ways(lambda lay: run_begin(lay, cs.dtype, st, tree0, dst0, ist0), self.layout, cs.dtype)
        w = R.nuts_begin(st["z"], st["p"], st["g"], st["U"], st["U0"], st["ke0"], tree0, dst0, ist0)
        check("tree", o["tree"].reshape(15, C, D), w["tree"], tree0)
        tol = np.zeros((C, 8))
        tol[:, R.H0] = 2 * U64 * (np.abs(st["U0"]) + np.abs(st["ke0"]))          # H0 = U0 + ke0: one rounding
        check("dst", o["dst"], w["dst"], dst0, tol)
        check("ist", o["ist"], w["ist"])
        return self.state(o, w, dst=o["dst"], ckpt_rows=self.r(self.g.standard_normal((C, cs.max_depth, 2, D))))

    def compact(self, T):
        cs = self.case
        f = Frame((1, 1, 0), np.float64)
        cap.nuts_compact(cs.C, f.flat("ist", T["ist"], np.int32), f.flat("rank", np.full(cs.C, 99), np.int32), f.flat("count", np.full(1, 99), np.int32))
        o = f.read("rank", "count")
        rank, count = R.nuts_compact(T["ist"])
        assert np.array_equal(o["rank"], rank) and int(o["count"][0]) == count
        return o["rank"], int(o["count"][0])

    def pre(self, T, eps, rank):
        cs, u = self.case, self.u
        C, D = cs.C, cs.D
        nn0, ode0 = self.r(self.g.standard_normal((C, max(cs.P, 1)))), self.r(self.g.standard_normal((C, 17)))
        o = three_ways(lambda lay: run_pre(lay, cs.dtype, cs, T, eps, rank, nn0, ode0), self.layout, cs.dtype)
        w, _, _, dec = R.nuts_pre(T, cs.seed, cs.it, eps, cs.minv, rank, cs.cmap, cs.mu, cs.sd, nn0, ode0)
        self.decisions += dec
        got = o["tree"].astype(np.float64).reshape(15, C, D)
        tol = np.zeros((15, C, D))
        want_nn, want_ode, tol_ode = nn0.copy(), ode0.copy(), np.zeros_like(ode0)
        for c in np.flatnonzero(T["ist"][:, R.ACTIVE]):
            v = int(w["ist"][c, R.DIRECTION])
            src = R.FZ if T["ist"][c, R.LEAF_I] else (R.RZ if v > 0 else R.LZ)
            sz, sp, sg = np.abs(T["tree"][src, c]), np.abs(T["tree"][src + 1, c]), np.abs(T["tree"][src + 2, c])
            e = abs(eps[c])
            # p -= eh g, eh = (R)(v eps / 2): the conversion, the product, the difference: 3
            tol[R.FP, c] = 4 * u * (sp + 0.5 * e * sg)
            # z += ed minv p, ed = (R)(v eps): the conversion, two products, the sum: 4, on top of p's 3
            tol[R.FZ, c] = 8 * u * (sz + e * cs.minv * (sp + 0.5 * e * sg))
            s, z = int(rank[c]), got[R.FZ, c]                # the parameters of slot rank[c] from the kernel's own stored z
            want_nn[s, :cs.P] = z[cs.n_ode:]
            want_ode[s, cs.idx] = cs.mu + cs.sd * z[:cs.n_ode]
            tol_ode[s, cs.idx] = (2 * u + 3 * U64) * (np.abs(cs.mu) + np.abs(cs.sd * z[:cs.n_ode]))
        check("tree", got, w["tree"], T["tree"], tol)
        check("ist", o["ist"], w["ist"])
        check("nn_p", o["nn_p"], want_nn)
        check("ode_p", o["ode_p"], want_ode, ode0, tol_ode)
        self.calls += 1
        return self.state(o, T), o["nn_p"].astype(np.float64), o["ode_p"].astype(np.float64)

    def post(self, T, eps, rank, gnn, gode, loss, status=None):
        cs, u = self.case, self.u
        C, D = cs.C, cs.D
        o = three_ways(lambda lay: run_post(lay, cs.dtype, cs, T, eps, rank, gnn, gode, loss, status), self.layout, cs.dtype)
        got = o["tree"].astype(np.float64).reshape(15, C, D)
        Tin = dict(T, ckpt=self.ckpt_dict(T["ckpt_rows"]))
        w, dec = R.nuts_post(Tin, cs.seed, cs.it, eps, cs.minv, rank, cs.cmap, cs.max_depth, cs.sd, gnn, gode, loss, K.LIK_SCALE, status,
                             fp_stored=got[R.FP])
        self.decisions += dec
        tol, tol_dst = np.zeros((15, C, D)), np.zeros((C, 8))
        want_ck, tol_ck = T["ckpt_rows"].copy(), np.zeros_like(T["ckpt_rows"])
        for c, i in w["info"].items():
            for r in (R.FG, R.SG, R.LG, R.RG):
                tol[r, c] = i["b_g"] * u                     # g = lik + z, and its copies to the subtree proposal and the edge
            if not np.array_equal(w["tree"][R.SG, c], T["tree"][R.SG, c]):
                tol[R.PG, c] = i["b_g"] * u                  # the proposal takes a subtree proposal written in this very call
            for r in (R.FP, R.LP, R.RP):
                tol[r, c] = i["b_p"] * u                     # p' = p - eh g, and its copy to the edge
            # rho_sub' = rho_sub + p': one rounding on top of p'; rho' = rho + rho_sub': one more
            tol[R.RHO_SUB, c] = (i["b_p"] + i["rho_sub_in"] + np.abs(w["tree"][R.FP, c])) * u
            tol[R.RHO, c] = tol[R.RHO_SUB, c] + (i["rho_in"] + np.abs(w["tree"][R.RHO_SUB, c])) * u
            # the sums over the kernel's own rows: (2 D + 4) u64 of their magnitude; then exp / log1p / the slots' own sums: 6
            w_d, b_d = np.nan_to_num(np.abs(w["dst"][c]), posinf=0.0), np.nan_to_num(np.abs(T["dst"][c]), posinf=0.0)
            tol_dst[c] = i["b_H"][U64] + 6 * U64 * (1 + i["mag"] + w_d + b_d)
        for (c, k) in w["written"]:
            ps, rb = w["ckpt"][(c, k)]
            want_ck[c, k - 1, 0], want_ck[c, k - 1, 1] = ps, rb
            tol_ck[c, k - 1, 0] = (w["info"][c]["minv_b_p"] + 2 * np.abs(ps)) * u   # p# = minv p': one product on top of p'
        check("tree", got, w["tree"], T["tree"], tol)
        check("ckpt", o["ckpt"].reshape(want_ck.shape), want_ck, T["ckpt_rows"], tol_ck)
        check("ist", o["ist"], w["ist"])
        check("dst", o["dst"], w["dst"], T["dst"], tol_dst)
        return self.state(o, T, dst=o["dst"], ckpt_rows=o["ckpt"].astype(np.float64).reshape(want_ck.shape))

    def finish(self, T, st):
        cs, u = self.case, self.u
        C, D = cs.C, cs.D
        last = None
        for adapt, slot, with_draws in ((0, 1, True), (1, -1, True), (1, 0, False)):
            draws = self.r(self.g.standard_normal((C, 2, D))) if with_draws else None
            stats, da = self.g.standard_normal((C, 2, 6)), self.g.uniform(0.1, 1, (C, 4)) * [1, 1, 1, 0] + [0, 0, 0, 4]
            o = three_ways(lambda lay: run_finish(lay, cs.dtype, cs, T, st, adapt, cs.log_eps, da, draws, stats, 2, slot), self.layout, cs.dtype)
            w = R.nuts_finish(T, adapt, 0.8, st["z"], st["g"], st["U"], cs.log_eps, da, cs.n_ode, cs.mu, cs.sd, draws, stats, slot)
            check("z", o["z"], w["z"])
            check("g", o["g"], w["g"])
            check("U", o["U"], w["U"])
            n_leaf = np.maximum(T["ist"][:, R.N_LEAF], 1)
            acc = T["dst"][:, R.SUM_ACC] / n_leaf
            t_acc = 2 * U64 * np.abs(acc)                    # one quotient
            if adapt:
                t_da, t_le = da_tolerance(da, acc, t_acc)
                check("da", o["da"], w["da"], da, t_da)
                check("log_eps", o["log_eps"], w["log_eps"], cs.log_eps, t_le)
            else:
                check("da", o["da"], da)
                check("log_eps", o["log_eps"], cs.log_eps)
            t_st = np.zeros_like(stats)
            if slot >= 0:
                t_st[:, slot, 0] = t_acc
            check("stats", o["stats"], w["stats"], stats, t_st)
            if with_draws:
                t_dr = np.zeros_like(draws)
                if slot >= 0:
                    t_dr[:, slot, :cs.n_ode] = (2 * u + 3 * U64) * (np.abs(cs.mu) + np.abs(cs.sd * w["z"][:, :cs.n_ode]))
                check("draws", o["draws"], w["draws"], draws, t_dr)
            last = last or w
        return last


@pytest.mark.parametrize("layout", K.TREE_LAYOUTS, ids=str)
@DT
@pytest.mark.parametrize("max_depth", [4, 1])
def test_nuts_tree_call_by_call(layout, dtype, max_depth):
    cs = K.TreeCase(layout, dtype, max_depth=max_depth)
    ops = KernelOps(cs, layout)
    out, T, alive = K.drive_tree(cs, ops)
    # the kernel's tree took the exits the CPU walk of the same case took
    ref_ops = K.RefOps(cs)
    _, T_ref, alive_ref = K.drive_tree(cs, ref_ops)
    assert np.array_equal(T["ist"], T_ref["ist"]) and np.array_equal(alive, alive_ref)
    assert [(d.kind, d.chain) for d in ops.decisions] == [(d.kind, d.chain) for d in ref_ops.decisions]
    if max_depth == 4:
        assert ops.calls == 15 and T["ist"][:, R.DIVERGENT].sum() == 1


@DT
def test_nuts_post_reads_the_status_of_the_chains_slot(dtype):
    """Chains 1 and 3 are inactive, so chain 4 sits in slot 2: a failing status in slot 2 (its last trajectory) must fail chain
    4 and nobody else, and a failing status in slot 4 nobody."""
    cs = K.status_case(dtype)
    ops = KernelOps(cs, cs.layout)
    for n_traj, slot, rank, T2 in K.walk_status_slots(cs, ops):
        assert rank.tolist() == [0, -1, 1, -1, 2]
        failed = np.flatnonzero(T2["ist"][:, R.FAILED])
        assert failed.tolist() == ([4] if slot == 2 else []), (n_traj, slot, failed)
        assert T2["ist"][[1, 3], R.N_LEAF].tolist() == [0, 0]
