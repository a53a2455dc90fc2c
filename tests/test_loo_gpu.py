"""The LOO kernels of csrc/hode_loo.hip (include/hode.h, "Model comparison") against their NumPy restatement
(tests/_loo_reference.py), in fp32 and fp64, at N = 18 (under one wave), 390 (a ragged wave) and 3 348 (fourteen workgroups, the
last ragged).  S = 1, 2, 7, 19 draws exercise the NaN of n < 2 and plain importance sampling (t <= 4: k = +inf); S = 40 (M = 8,
m = 32) and S = 300 (M = 52, m = 37) reach the Pareto fit, its weight pruning and a heap six levels deep that overflows hundreds
of times.  K = loo_tail_size(S), K = S + 3 and a K that is too small (NaN, left out of the table).  `-m gpu`.

TOLERANCES, none of them taken from the kernels' output:
* the pointwise log likelihood l: every operation but log(sigma) is an IEEE operation that NumPy repeats bit for bit; the bound
  of `_loo_reference.l_tolerance` (two ulp of log sigma through two re-rounding subtractions) is tol_l = 4 * 2^-52 *
  max(1, |log sigma|, |l|).  An order statistic moves by no more than its inputs, so the sorted `top`, `pmax` and `rmax` are held
  to tol_l; the Welford mean to tol_l + 2 n 2^-52 max|l|; lm2 = sum (l - mean)^2 to 4 n max|l - mean| tol_l + 4 n 2^-52 lm2;
  psum and rsum (sums of exp of differences of two perturbed values, rescaled at most n times) relatively to 4 tol_l + 8 n 2^-52.
* elpd_loo and pareto_k: ten times the fp64-against-longdouble difference of the restatement on exactly these inputs
  (test_loo_host.py): 1.4e-12 and 1.6e-12 absolute.  lppd, p_waic and elpd_waic follow from the state's bounds above.  An fp32
  output carries one rounding more, 2^-24 relative.  A table sum is allowed the sum of its entries' bounds plus
  count * 2^-52 * sum |term| for the order of the additions; the counts are exact (the restatement's k and p_waic are at least
  1e-6 from every threshold and no tail value ties its cut, asserted in test_loo_host.py and again here)."""
import os

import numpy as np
import pytest

import _loo_reference as LR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402

DTYPES = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
DEV = "cuda"
SENTINEL = -7.0
EPS = LR.EPS
SUMS = ("lmean", "lm2", "pmax", "psum", "rmax", "rsum")


def bits(t):
    if not t.is_floating_point():
        return t
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)       # (NaN == NaN)


def run(c, dt, K, splits=None, perm=None, offset=False, finish_after=None, use_mask=True, r_eff=1.0):
    """Fold c's draws in the given consecutive pieces (default: one call); returns the raw state as folded (clones), the outputs
    and the table of pred_loo_finish, the sorted top and the state itself."""
    tdt = DTYPES[dt][0]
    S, N = c["y"].shape
    y = torch.tensor(c["y"], dtype=tdt, device=DEV)
    status, sigma = torch.tensor(c["status"], device=DEV), torch.tensor(c["sigma"], device=DEV)
    obs = torch.tensor(c["obs"], dtype=tdt, device=DEV)
    mask = torch.tensor(c["mask"], device=DEV) if use_mask else None
    if perm is not None:
        y, status, sigma = y[perm].contiguous(), status[perm].contiguous(), sigma[perm].contiguous()
    if offset:                                                  # the same values one element off the allocation's alignment
        buf = torch.empty(S * N + 1, dtype=tdt, device=DEV)
        buf[1:].copy_(y.reshape(-1))
        y = buf[1:].view(S, N)
        assert y.data_ptr() % 16 != 0
    ls = hode.capi.pred_loo_state(N, K, DEV)
    ls["top"].fill_(SENTINEL)
    for n, (lo, hi) in enumerate(splits or [(0, S)]):
        hode.capi.pred_loo_fold(y[lo:hi], ls, obs, mask, sigma[lo:hi], status[lo:hi])
        if finish_after is not None and n == finish_after:
            hode.capi.pred_loo_finish(ls, tdt, r_eff)
    raw = {k: v.clone() for k, v in ls.items()}
    out, table = hode.capi.pred_loo_finish(ls, tdt, r_eff)
    return raw, out, table, hode.capi.pred_loo_top_values(ls), ls


def state_bounds(c, l, ref):
    """Per-entry absolute bounds of the state's running sums (module docstring)."""
    tol_l = LR.l_tolerance(c, l)
    n = ref["cnt"].astype(np.float64)
    lf = np.asarray(l, dtype=np.float64)
    lmax = np.where(np.isnan(lf), 0.0, np.abs(lf)).max(0)
    dmax = np.where(np.isnan(lf), 0.0, np.abs(lf - ref["lmean"][None])).max(0)
    rel = 4.0 * tol_l + 8.0 * n * EPS
    return {"tol_l": tol_l, "lmean": tol_l + 2.0 * n * EPS * lmax, "lm2": 4.0 * n * dmax * tol_l + 4.0 * n * EPS * ref["lm2"],
            "pmax": tol_l, "rmax": tol_l, "psum": rel * ref["psum"], "rsum": rel * ref["rsum"]}


def output_bounds(c, l, ref, out):
    b = state_bounds(c, l, ref)
    n = np.maximum(ref["cnt"].astype(np.float64), 2.0)
    with np.errstate(all="ignore"):
        lppd = b["pmax"] + b["psum"] / np.where(ref["psum"] > 0, ref["psum"], 1.0) + 4.0 * EPS * np.abs(np.nan_to_num(out["lppd"]))
        pw = b["lm2"] / (n - 1.0) + 2.0 * EPS * np.abs(np.nan_to_num(out["p_waic"]))
    N = lppd.size
    return {"elpd_loo": np.full(N, LR.TOL_ELPD), "pareto_k": np.full(N, LR.TOL_K), "lppd": lppd, "p_waic": pw,
            "elpd_waic": lppd + pw + EPS * np.abs(np.nan_to_num(out["elpd_waic"]))}


def table_bounds(ref_out, ob):
    """[6, 8]: the bound of every fp64 sum of the table (columns 1..7; column 0 unused)."""
    N = ref_out["lppd"].size
    use = ~np.isnan(ref_out["lppd"])
    tb = np.zeros((6, 8))
    v = {k: np.nan_to_num(np.asarray(ref_out[k], dtype=np.float64)) for k in LR.OUTPUTS}
    for s in range(6):
        u = use & (np.arange(N) % 6 == s)
        cnt = u.sum()
        terms = ((1, v["elpd_loo"], ob["elpd_loo"]), (2, v["elpd_loo"] ** 2, 2.0 * np.abs(v["elpd_loo"]) * ob["elpd_loo"] + ob["elpd_loo"] ** 2),
                 (3, v["lppd"] - v["elpd_loo"], ob["lppd"] + ob["elpd_loo"]), (4, v["elpd_waic"], ob["elpd_waic"]),
                 (5, v["elpd_waic"] ** 2, 2.0 * np.abs(v["elpd_waic"]) * ob["elpd_waic"] + ob["elpd_waic"] ** 2), (6, v["p_waic"], ob["p_waic"]),
                 (7, v["lppd"], ob["lppd"]))
        for col, term, bound in terms:
            tb[s, col] = bound[u].sum() + (cnt + 2) * EPS * (np.abs(term[u]).sum() + np.abs(v["lppd"][u]).sum() + np.abs(v["elpd_loo"][u]).sum())
    return tb


def check(got, c, dt, K, refs):
    """The kernels' state, outputs and table against the restatement's (refs = LR.reference(...))."""
    raw, out, table, top, _ = got
    l, ref, rout = refs
    npdt = DTYPES[dt][1]
    N = c["N"]
    cnt = ref["cnt"]
    assert np.array_equal(raw["cnt"].cpu().numpy(), cnt)
    m = np.minimum(cnt, K)
    untouched = np.arange(K)[:, None] >= m[None]
    assert bool((raw["top"].cpu().numpy()[untouched] == SENTINEL).all())              # slots past min(cnt, K) were never written
    b = state_bounds(c, l, ref)
    gtop, rtop = top.cpu().numpy(), LR.sorted_top(ref)
    assert np.array_equal(np.isnan(gtop), np.isnan(rtop)) and np.array_equal(np.isnan(rtop), untouched)
    worst = np.where(untouched, 0.0, np.abs(gtop - rtop) / b["tol_l"][None]).max()
    print(f"N={N} S={c['y'].shape[0]} K={K} {dt}: top, worst difference / bound = {worst:.3f}")
    assert worst <= 1.0
    for k in SUMS:
        g, r = raw[k].cpu().numpy(), ref[k]
        inf = np.isinf(r)
        assert np.array_equal(g[inf], r[inf]), k
        ratio = np.abs(g[~inf] - r[~inf]) / np.maximum(b[k][~inf], 1e-300)
        ratio = np.where(g[~inf] == r[~inf], 0.0, ratio)
        print(f"    {k}: worst difference / bound = {ratio.max() if ratio.size else 0.0:.3f}")
        assert (ratio <= 1.0).all(), k
    ob = output_bounds(c, l, ref, rout)
    scored = ~np.isnan(rout["lppd"])
    for k in LR.OUTPUTS:
        g, r = out[k].cpu().numpy().astype(np.float64), np.asarray(rout[k], dtype=np.float64)
        assert out[k].dtype == DTYPES[dt][0]
        assert np.array_equal(np.isnan(g), np.isnan(r)), k                                  # the NaN pattern, exactly
        assert np.array_equal(np.isinf(g), np.isinf(r)) and np.array_equal(g[np.isinf(r)], r[np.isinf(r)]), k
        fin = np.isfinite(r)
        bound = ob[k][fin] + (2.0 ** -24 * np.abs(r[fin]) if npdt == np.float32 else 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(g[fin] == r[fin], 0.0, np.abs(g[fin] - r[fin]) / bound)
        print(f"    {k}: worst difference / bound = {ratio.max() if ratio.size else 0.0:.3f}")
        assert (ratio <= 1.0).all(), k
        assert np.isnan(g[~scored]).all()
    want, tb = LR.table(rout), table_bounds(rout, ob)
    tab = table.cpu().numpy()
    print("    table\n", tab, "\n    restatement\n", want)
    assert np.array_equal(tab[:, [0, 8, 9, 10, 11, 12]], want[:, [0, 8, 9, 10, 11, 12]])
    assert (np.abs(tab[:, 1:8] - want[:, 1:8]) <= tb[:, 1:8]).all(), np.abs(tab[:, 1:8] - want[:, 1:8]) / np.maximum(tb[:, 1:8], 1e-300)
    assert (tab[LR.UNSEEN_STATE] == 0).all()
    return rout


def k_variants(shape, S):
    ks = {LR.loo_tail_size(S), 2}
    if S < 300 or shape != LR.SHAPES[2]:
        ks.add(S + 3)
    return sorted(ks)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape,S", LR.GPU_CASES)
def test_fold_and_finish_against_restatement(shape, S, dt):
    c = LR.case(*shape, S, dt)
    for K in k_variants(shape, S):
        refs = LR.reference(*shape, S, dt, K)
        rout = check(run(c, dt, K), c, dt, K, refs)
        assert LR.clear_of_thresholds(rout) and list(np.where(rout["tie"])[0]) in ([], [LR.CONST_ENTRY])
        cnt, scored = refs[1]["cnt"], ~np.isnan(rout["lppd"])
        # the contract's NaN, independently of the restatement
        assert cnt[1] == 0 and not scored[1] and not scored[np.arange(c["N"]) % 6 == LR.UNSEEN_STATE].any()
        if S < 2 or LR.loo_tail_size(S) > K:
            assert not scored.any()                                                          # one draw, or a buffer sized for fewer
        else:
            assert np.array_equal(scored, cnt >= 2)                                          # fewer draws need no more ratios
            assert scored[LR.CONST_ENTRY] and np.isinf(rout["pareto_k"][LR.CONST_ENTRY])
            if S <= 19:
                assert np.isinf(rout["pareto_k"][scored]).all()                              # t <= 4: plain importance sampling
            elif c["N"] >= 390:
                assert (LR.table(rout)[:, 8:12].sum(0) > 0).all()                            # all four k bins are populated
    # the skips reached the counts
    cnt = LR.reference(*shape, S, dt, LR.loo_tail_size(S))[1]["cnt"].reshape(shape[0], shape[1], 6)
    assert cnt[0, 0, 0] == (S - 1 if S >= 2 else S) and cnt[0, 0, 2] == S


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_special_cases(dt):
    """sigma_k = 0 for state 3 in every draw (no likelihood: NaN and a zero row); no mask (finiteness of obs alone decides);
    r_eff = 0.5 with a buffer sized for it and with one sized for r_eff = 1."""
    shape, S = LR.SHAPES[1], 40
    c = LR.case(*shape, S, dt, 3)
    K = LR.loo_tail_size(S)
    refs = LR.reference(*shape, S, dt, K, False, 3)
    rout = check(run(c, dt, K), c, dt, K, refs)
    st3 = np.arange(c["N"]) % 6 == 3
    assert (refs[1]["cnt"][st3] == 0).all() and np.isnan(rout["elpd_loo"][st3]).all() and (LR.table(rout)[3] == 0).all()
    # no mask
    c0 = LR.case(*shape, S, dt)
    l = LR.log_lik(c0["y"], c0["obs"], None, c0["sigma"], c0["status"])
    st, ro = LR.loo_of(l, K)
    got = run(c0, dt, K, use_mask=False)
    assert np.array_equal(got[0]["cnt"].cpu().numpy(), st["cnt"]) and (st["cnt"][np.arange(c0["N"]) % 6 == LR.UNSEEN_STATE] > 0).any()
    assert np.array_equal(got[2].cpu().numpy()[:, [0, 8, 9, 10, 11, 12]], LR.table(ro)[:, [0, 8, 9, 10, 11, 12]])
    # r_eff = 0.5: M = ceil(min(8, 3 sqrt(80))) = 8 still; at S = 300, M = 60 instead of 52
    c3 = LR.case(*LR.SHAPES[0], 300, dt)
    l3 = LR.log_lik(c3["y"], c3["obs"], c3["mask"], c3["sigma"], c3["status"])
    K5 = LR.loo_tail_size(300, 0.5)
    assert K5 == 61
    st5 = LR.fold(LR.fresh_state(c3["N"], K5), l3)
    ro5 = LR.finish(st5, 0.5)
    g5 = run(c3, dt, K5, r_eff=0.5)
    assert (ro5["t"][ro5["t"] > 4] == 60).all()
    for k in ("elpd_loo", "pareto_k"):
        g, r = g5[1][k].cpu().numpy().astype(np.float64), ro5[k]
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r))
        tol = (LR.TOL_ELPD if k == "elpd_loo" else LR.TOL_K) + (2.0 ** -24 * np.abs(r[fin]) if dt == "f32" else 0.0)
        assert (np.abs(g[fin] - r[fin]) <= tol).all(), k
    small = run(c3, dt, LR.loo_tail_size(300), r_eff=0.5)                                    # sized for r_eff = 1: 53 < 61
    assert all(bool(torch.isnan(small[1][k]).all()) for k in LR.OUTPUTS) and bool((small[2] == 0).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", LR.SHAPES)
def test_splits_permutation_and_further_folds(shape, dt):
    """7 = 3 + 3 + 1 = 4 + 3 (from a misaligned view) = 1 x 7 = the same call again, and 300 in 16 pieces: every state array, every
    output and the table are torch.equal.  A permutation of the draws: cnt, the sorted top and pareto_k bit-equal, the rest to
    the bounds of the module docstring.  Folding on after a finish (which sorts top in place): the same multiset is held and the
    same values are evicted in the same order, so everything is bit-equal again."""
    for S, K, runs in ((7, 3, {"3+3+1": [(0, 3), (3, 6), (6, 7)], "4+3": [(0, 4), (4, 7)], "one by one": [(s, s + 1) for s in range(7)],
                               "again": [(0, 7)]}),
                       (7, 10, {"3+3+1": [(0, 3), (3, 6), (6, 7)]}),
                       (300, 53, {"16 pieces": [(lo, min(lo + 19, 300)) for lo in range(0, 300, 19)]})):
        c = LR.case(*shape, S, dt)
        whole = run(c, dt, K)
        for name, splits in runs.items():
            other = run(c, dt, K, splits, offset=(name == "4+3"))
            assert len(splits) == 16 or S == 7
            for k in hode.capi.PRED_LOO_STATE:
                assert torch.equal(bits(whole[0][k]), bits(other[0][k])), (name, k)
            for k in LR.OUTPUTS:
                assert torch.equal(bits(whole[1][k]), bits(other[1][k])), (name, k)
            assert torch.equal(bits(whole[2]), bits(other[2])), name
        later = run(c, dt, K, [(0, 3), (3, S)], finish_after=0)
        assert torch.equal(whole[0]["cnt"], later[0]["cnt"]) and torch.equal(bits(whole[3]), bits(later[3]))
        for k in SUMS:
            assert torch.equal(bits(whole[0][k]), bits(later[0][k])), k
        for k in LR.OUTPUTS:
            assert torch.equal(bits(whole[1][k]), bits(later[1][k])), k
        assert torch.equal(bits(whole[2]), bits(later[2]))
        perm = torch.tensor(np.random.default_rng(S + K).permutation(S), device=DEV)
        shuffled = run(c, dt, K, perm=perm)
        assert torch.equal(whole[0]["cnt"], shuffled[0]["cnt"]) and torch.equal(bits(whole[3]), bits(shuffled[3]))
        assert torch.equal(bits(whole[1]["pareto_k"]), bits(shuffled[1]["pareto_k"]))
        pc = {k: (v[perm.cpu().numpy()] if k in ("y", "sigma", "status") else v) for k, v in c.items()}
        l = LR.log_lik(pc["y"], pc["obs"], pc["mask"], pc["sigma"], pc["status"])
        st, ro = LR.loo_of(l, K)
        check(shuffled, pc, dt, K, (l, st, ro))


# ------------------------------------------------------------------------------------------------ the entry points
B, T = 3, 13
SIGMA6 = [6.0, 0.8, 3.0, 0.4, 0.03, 0.02]


def _model(golden_dir, variational=False):
    import models
    w = np.load(os.path.join(golden_dir, "g0_weights_h32_l2.npz"))
    ode8 = {"a_GI": 0.0104, "k_I": 0.025, "rho": 0.003, "E_max": 0.1, "EC_50": 50.0, "V_max": 9.0, "K_m": 7.0, "k_L": 0.02}
    prior = {f"ode_{n}": {"mean": v, "std": 0.05 * v} for n, v in ode8.items()}
    m = models.HybridODENN(nn_hidden=32, nn_layers=2, use_variational=variational, prior_params=prior if variational else None,
                           device="cuda")
    flat, off = torch.tensor(w["nn_flat"]), 0
    with torch.no_grad():
        for name, p in m.nn_residual.named_parameters():
            p.copy_(flat[off:off + p.numel()].reshape(p.shape))
            if variational:                                  # a posterior centred on the golden weights, 2 % wide
                key = f"nn_{name.replace('.', '_')}"
                m.variational_params.means[key].copy_(p)
                m.variational_params.log_stds[key].fill_(float(np.log(0.02)))
            off += p.numel()
    return m


@pytest.fixture(scope="module")
def batch(golden_dir):
    g = np.load(os.path.join(golden_dir, "g4_t61_pulses.npz"))
    rng = np.random.default_rng(5)
    obs = g["y_rk45_tight"][:B, :T].astype(np.float64) * (1.0 + 0.05 * rng.standard_normal((B, T, 6)))
    obs[rng.random((B, T, 6)) < 0.05] = np.nan
    return {"initial_state": torch.tensor(g["x0"][:B]), "observations": torch.tensor(obs, dtype=torch.float32),
            "time_points": torch.tensor(g["t"][:T]),
            "external_inputs": {"meal": torch.tensor(g["meal"][:B, :T]), "tVNS": torch.tensor(g["tvns"][:B, :T])}}


def _check_loo_against_block(summ, y, sigma, batch):
    """summ.loo against the restatement applied to the held block y [S, B, T, 6] with the noise sigma [S, 6]."""
    y = y.detach().cpu().numpy().astype(np.float64)
    S = y.shape[0]
    obs = batch["observations"].numpy().astype(np.float64).reshape(-1)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(-1, 6), (S, 6))
    c = {"y": y.reshape(S, -1), "sigma": sigma, "N": obs.size}
    l = LR.log_lik(c["y"], obs, None, sigma)
    st, ro = LR.loo_of(l, LR.loo_tail_size(S))
    ob = output_bounds(c, l, st, ro)
    loo = summ.loo
    for k in LR.OUTPUTS:
        g, r = getattr(loo, k).cpu().numpy().astype(np.float64).reshape(-1), ro[k]
        assert tuple(getattr(loo, k).shape) == (B, T, 6) and np.array_equal(np.isnan(g), np.isnan(r)), k
        fin = np.isfinite(r)
        assert np.array_equal(g[np.isinf(r)], r[np.isinf(r)])
        assert (np.abs(g[fin] - r[fin]) <= ob[k][fin] + 2.0 ** -24 * np.abs(r[fin])).all(), k
    want, tb = LR.table(ro), table_bounds(ro, ob)
    assert np.array_equal(loo.table[:, [0, 8, 9, 10, 11, 12]], want[:, [0, 8, 9, 10, 11, 12]])
    assert (np.abs(loo.table[:, 1:8] - want[:, 1:8]) <= tb[:, 1:8]).all()
    est = loo.estimates()
    assert est["count"] == np.isfinite(obs).sum() == want[:, 0].sum() and abs(est["elpd_loo"] - want[:, 1].sum()) <= tb[:, 1].sum()
    assert abs(est["p_loo"] - (est["lppd"] - est["elpd_loo"])) <= 1e-9 * abs(est["lppd"]) and est["looic"] == -2.0 * est["elpd_loo"]
    return loo


def _same_fields(a, b):
    for name in ("mean", "std", "pit", "n"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert np.array_equal(a.table, b.table)
    assert (a.quantiles is None) == (b.quantiles is None)
    if a.quantiles is not None:
        assert torch.equal(bits(a.quantiles), bits(b.quantiles)) and np.array_equal(a.band_table, b.band_table)
    ma, mb = a.metrics(), b.metrics()
    assert set(ma) == set(mb) and all(np.array_equal(ma[k], mb[k], equal_nan=True) for k in ma)


def test_predictive_summary_and_vi_loo_in_pieces(golden_dir, batch):
    from inference import VariationalInference, compare, predictive_summary
    m = _model(golden_dir, variational=True)
    torch.manual_seed(3)
    with torch.no_grad():
        draws = [m.variational_params.sample(1)[0] for _ in range(7)]
        y = m.forward_param_sets(draws, batch["initial_state"], batch["time_points"], batch["external_inputs"])
    assert m.solve_failures() == 0
    piece = B * T * 6 * 4
    summ = predictive_summary(m, draws, batch, sigma=SIGMA6, max_bytes=3 * piece, loo=True)               # cut 3 + 3 + 1
    loo = _check_loo_against_block(summ, y, SIGMA6, batch)
    other = predictive_summary(m, draws, batch, sigma=SIGMA6, max_bytes=2 * piece, loo=True, quantiles=(0.025, 0.975))     # 2 + 2 + 2 + 1
    for k in LR.OUTPUTS:
        assert torch.equal(bits(getattr(loo, k)), bits(getattr(other.loo, k))), k
    assert np.array_equal(loo.table, other.loo.table)
    # with loo off (by default and explicitly) every earlier field is what it was, and loo on changes none of them
    plain = predictive_summary(m, draws, batch, sigma=SIGMA6, max_bytes=3 * piece)
    off = predictive_summary(m, draws, batch, sigma=SIGMA6, max_bytes=3 * piece, loo=False)
    assert plain.loo is None and off.loo is None
    _same_fields(plain, off)
    _same_fields(plain, summ)
    _same_fields(predictive_summary(m, draws, batch, sigma=SIGMA6, max_bytes=2 * piece, quantiles=(0.025, 0.975)), other)
    # a model against itself, and against one with another noise model
    rows = compare({"a": summ, "b": other.loo})
    assert [r["elpd_diff"] for r in rows] == [0.0, 0.0] and [r["dse"] for r in rows] == [0.0, 0.0]
    assert abs(rows[0]["weight"] - 0.5) <= 1e-12 and rows[0]["elpd"] == loo.estimates()["elpd_loo"]
    wide = predictive_summary(m, draws, batch, sigma=[10.0 * s for s in SIGMA6], loo=True)
    for ic in ("loo", "waic"):
        rows = compare({"wide": wide, "fitted": summ}, ic=ic)
        assert sorted(r["name"] for r in rows) == ["fitted", "wide"] and rows[0]["elpd"] > rows[1]["elpd"]
        assert rows[0]["elpd_diff"] == 0.0 and rows[1]["elpd_diff"] == rows[1]["elpd"] - rows[0]["elpd"] and rows[1]["dse"] > 0
        assert rows[0]["weight"] > rows[1]["weight"] and abs(rows[0]["weight"] + rows[1]["weight"] - 1.0) <= 1e-12
    with pytest.raises(ValueError, match="sigma"):
        predictive_summary(m, draws, batch, loo=True)
    torch.manual_seed(3)
    vs = VariationalInference(m, device=torch.device("cuda")).predictive_summary(batch, n_samples=7, noise_sigma=SIGMA6, max_bytes=2 * piece,
                                                                                 loo=True)
    _check_loo_against_block(vs, y, SIGMA6, batch)


def test_hmc_result_loo(golden_dir, batch):
    from inference.hmc import HMCResult
    from inference.observation import ObservationModel
    m = _model(golden_dir)
    nn_base, ode_base = m._params_on(torch.device("cuda"))
    rng = np.random.default_rng(9)
    mu = np.array([0.025, 7.0])
    draws = torch.tensor(mu * (1.0 + 0.05 * rng.standard_normal((2, 4, 2))), dtype=torch.float32, device="cuda")
    res = HMCResult(draws, ["k_I", "K_m"], [], {}, m, ode_base.detach(), nn_base.detach(), ObservationModel(SIGMA6), batch)
    summ = res.predictive_summary(max_bytes=3 * B * T * 6 * 4, loo=True)
    y = res.predict(batch["initial_state"], batch["time_points"], batch["external_inputs"], observation_noise=False)
    assert tuple(y.shape) == (8, B, T, 6)
    sigma = res.noise_sigma(batch, 1, 0, "dopri5", 1e-6, 1e-8).cpu().numpy()
    _check_loo_against_block(summ, y, sigma, batch)
    plain = res.predictive_summary(max_bytes=3 * B * T * 6 * 4)
    assert plain.loo is None
    _same_fields(plain, summ)
    with pytest.raises(ValueError, match="observation_noise"):
        res.predictive_summary(observation_noise=False, loo=True)
