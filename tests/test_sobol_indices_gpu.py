"""The Sobol-index kernel (csrc/hode_sobol.hip) and its Python surface (inference/sobol.py) on the GPU, held to the numpy
restatement of tests/_sobol_reference.py.  `-m gpu`.

Tolerance against the restatement: absolute 1e-9 on every index and conf.  Both sides sum fp64 in some order, at most ~1e5 terms
of magnitude <= ~1e2 after normalisation: 1e5 * 2^-53 * 1e2 ~ 1e-9; fp32 input is exact in fp64.  NaN positions must match
exactly (assert_allclose with equal_nan demands NaN on both sides or neither)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import hode  # noqa: E402
from inference import saltelli_design, sobol_indices, sobol_study  # noqa: E402
from inference.sobol import default_outputs  # noqa: E402

import _sobol_reference as SR  # noqa: E402

ATOL = 1e-9
KEYS = ("S1", "ST", "S2", "S1_conf", "ST_conf", "S2_conf")
Z95 = 1.959963984540054


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _close(got, want, second=True, what=""):
    """`got`: the binding's dict of device tensors, `want`: the restatement's dict of arrays (leading M)."""
    for k in KEYS:
        if k.startswith("S2") and not second:
            assert got[k] is None
            continue
        g, w = got[k].cpu().numpy(), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        print(what, k, "max |diff|", np.nanmax(np.abs(g - w)) if np.isfinite(g - w).any() else "all NaN")
        np.testing.assert_allclose(g, w, rtol=0.0, atol=ATOL, equal_nan=True, err_msg=f"{what} {k}")
    np.testing.assert_allclose(got["variance"].cpu().numpy(), want["variance"], rtol=1e-12, atol=0.0, equal_nan=True, err_msg=what)


def _equal(a, b):
    """Bit for bit, NaN included."""
    for k in KEYS + ("variance",):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None
        else:
            assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


def _columns(got, cols):
    return {k: (None if v is None else v[cols]) for k, v in got.items()}


def _ishigami(n, second=True, seed=0):
    return SR.ishigami(saltelli_design([(-np.pi, np.pi)] * 3, n=n, calc_second_order=second, seed=seed))


@pytest.mark.parametrize("second", [True, False])
def test_case1_ishigami_small_fp64(second):
    y = _ishigami(64, second)
    got = hode.capi.sobol_indices(_dev(y[:, None]), 3, second, 16, 11, Z95)
    _close(got, SR.analyze(y[:, None], 3, second, 16, 11, Z95), second, "case1")


def test_case2_odd_sizes_padded_rows_unaligned_base_fp32():
    """D = 7, N = 5, M = 7 columns inside rows of ldy = 9, the first element one off the allocation's start."""
    rows = 5 * 16
    buf = torch.as_tensor(np.random.default_rng(2).standard_normal(1 + rows * 9), dtype=torch.float32, device="cuda")
    Y = buf[1:].view(rows, 9)[:, :7]
    assert Y.data_ptr() % 8 == 4 and Y.stride(0) == 9
    got = hode.capi.sobol_indices(Y, 7, True, 3, 1 << 40 | 5, Z95)
    _close(got, SR.analyze(Y.cpu().numpy(), 7, True, 3, 1 << 40 | 5, Z95), True, "case2")
    # the padding was not read as data, and the strided view equals its packed copy
    _equal(got, hode.capi.sobol_indices(Y.contiguous(), 7, True, 3, 1 << 40 | 5, Z95))


@pytest.mark.parametrize("R", [0, 1])
def test_case3_one_base_sample_gives_nan_conf(R):
    y = np.random.default_rng(3).standard_normal((8, 2))
    got = hode.capi.sobol_indices(_dev(y), 3, True, R, 0, Z95)
    torch.cuda.synchronize()
    for k in ("S1_conf", "ST_conf", "S2_conf"):
        assert torch.isnan(got[k]).all(), k
    _close(got, SR.analyze(y, 3, True, R, 0, Z95), True, f"case3 R={R}")


def test_case4_degenerate_columns_do_not_disturb_their_neighbours():
    rng = np.random.default_rng(4)
    y = rng.standard_normal((12 * 8, 4)).astype(np.float32)
    y[:, 1] = 3.25
    y[17, 2] = np.nan
    Y = _dev(y, torch.float32)
    got = hode.capi.sobol_indices(Y, 3, True, 5, 7, Z95)
    for k in KEYS:
        assert torch.isnan(got[k][1:3]).all(), k
        live = got[k][[0, 3]]
        assert torch.isfinite(live[:, 0, 1] if k.startswith("S2") else live).all(), k
    assert float(got["variance"][1]) == 0.0 and bool(torch.isnan(got["variance"][2]))
    _close(got, SR.analyze(y, 3, True, 5, 7, Z95), True, "case4")
    for c in (0, 3):
        _equal(_columns(got, slice(c, c + 1)), hode.capi.sobol_indices(Y[:, c:c + 1], 3, True, 5, 7, Z95))
    # an infinite value is non-finite too
    y[17, 2] = np.inf
    inf = hode.capi.sobol_indices(_dev(y, torch.float32), 3, True, 5, 7, Z95)
    assert torch.isnan(inf["S1"][2]).all() and bool(torch.isnan(inf["variance"][2]))


def test_case5_column_too_large_for_lds_matches_and_lds_pair():
    """N = 2048, D = 7 in fp64 is 256 KiB per column: gathered from global memory.  N = 512 of the same data (64 KiB) is staged."""
    y = np.random.default_rng(5).standard_normal((2048 * 16, 2))
    y[:, 1] = y[:, 1] * 3.0 + np.repeat(np.random.default_rng(6).standard_normal(2048), 16) * 2.0 + 40.0      # correlated blocks
    for n in (2048, 512):
        part = y[:n * 16]
        got = hode.capi.sobol_indices(_dev(part), 7, True, 4, 21, Z95)
        _close(got, SR.analyze(part, 7, True, 4, 21, Z95), True, f"case5 N={n}")


def test_case5b_both_routes_give_the_same_bits():
    """The same values as fp32 (128 KiB: staged) and as fp64 (256 KiB: gathered from global memory): fp32 converts to fp64 exactly,
    so the two calls feed the same operands to the same sums.  Likewise with the resample indices kept in LDS (fp64, D = 3,
    N = 2000: 128 000 B + 8 000 B) or recomputed (N = 2500: 160 000 B leave no room for them) against the restatement, and with
    neither the column nor the indices in LDS (D = 1, first order, N = 41 000)."""
    y32 = np.random.default_rng(8).standard_normal((2048 * 16, 1)).astype(np.float32)
    a = hode.capi.sobol_indices(_dev(y32, torch.float32), 7, True, 3, 2, Z95)
    b = hode.capi.sobol_indices(_dev(y32, torch.float64), 7, True, 3, 2, Z95)
    _equal(a, b)
    y = np.random.default_rng(9).standard_normal((2500 * 8, 1))
    for n in (2000, 2500):
        got = hode.capi.sobol_indices(_dev(y[:n * 8]), 3, True, 2, 4, Z95)
        _close(got, SR.analyze(y[:n * 8], 3, True, 2, 4, Z95), True, f"case5b N={n}")
    y1 = np.random.default_rng(10).standard_normal((41000 * 3, 1))
    got = hode.capi.sobol_indices(_dev(y1), 1, False, 2, 4, Z95)
    _close(got, SR.analyze(y1, 1, False, 2, 4, Z95), False, "case5b D=1")


def test_case6_same_bits_every_time_and_per_column():
    y = np.random.default_rng(6).standard_normal((32 * 12, 12)).astype(np.float32)
    y[:, 5] += y[:, 4]
    Y = _dev(y, torch.float32)
    a = hode.capi.sobol_indices(Y, 5, True, 6, 99, Z95)
    b = hode.capi.sobol_indices(Y, 5, True, 6, 99, Z95)
    _equal(a, b)
    for c in range(12):
        _equal(_columns(a, slice(c, c + 1)), hode.capi.sobol_indices(Y[:, c:c + 1].contiguous(), 5, True, 6, 99, Z95))
    # conf of a column does not change when unrelated columns are added: all columns share the resample indices
    few = hode.capi.sobol_indices(Y[:, 3:5], 5, True, 6, 99, Z95)
    _equal(_columns(a, slice(3, 5)), few)
    # ... and it does depend on the seed
    assert not torch.equal(a["S1_conf"], hode.capi.sobol_indices(Y, 5, True, 6, 100, Z95)["S1_conf"])
    _close(a, SR.analyze(y, 5, True, 6, 99, Z95), True, "case6")


def test_case7_class_surface_time_resolved_study():
    """256 sets x 61 points through sobol_study.  Row 0 of every trajectory is x0: constant over the design, NaN indices.  The
    GE state is constant only where nothing but ODECore moves it (dGE = 0 there): the benchmark's network adds a residual to all
    six states (measured here: GE gets finite indices from point 1 on), so the all-NaN GE column is checked on the same model
    with the GE row of the network's output layer zeroed, and on the benchmark's model the NaN positions are the restatement's."""
    import bench
    dev = torch.device("cuda")
    m = bench.class_model(dev)
    x0, t, meal, tvns = (v.to(dev) for v in bench.sobol_inputs())
    bounds = dict(zip(bench.SOBOL_NAMES, map(tuple, bench.SOBOL_BOUNDS)))
    Si = sobol_study(m, bounds, x0, t, {"meal": meal, "tVNS": tvns}, n=16, time_resolved=True, num_resamples=8, seed=3)
    assert Si.n_dropped == 0 and Si.names == bench.SOBOL_NAMES and Si.outputs == ["glucose_auc", "insulin_peak", "glp1_response"]
    assert tuple(Si["S1"].shape) == (3, 7) and tuple(Si["S2"].shape) == (3, 7, 7) and Si["S1"] is Si.S1
    Rt = Si.resolved
    assert tuple(Rt["S1"].shape) == (61, 6, 7) and tuple(Rt["S2"].shape) == (61, 6, 7, 7) and tuple(Rt.variance.shape) == (61, 6)
    for k in KEYS:
        assert torch.isnan(Rt[k][0]).all(), k                                                # x0 does not move
    assert torch.isfinite(Rt["S1"][7:, 0]).all() and torch.isfinite(Si["S1"]).all()          # glucose after the meal, the three outputs
    # against the restatement fed the same downloaded trajectories
    sets = saltelli_design(bounds, n=16, seed=3)
    y = m.forward_ode_sets({k: torch.as_tensor(sets[:, i], dtype=torch.float32) for i, k in enumerate(bench.SOBOL_NAMES)},
                           x0, t, {"meal": meal, "tVNS": tvns})
    assert tuple(y.shape) == (256, 61, 6)
    yh = y.cpu().numpy()
    want = SR.analyze(yh.reshape(256, -1), 7, True, 8, 3, Z95)
    got = {k: Rt[k].reshape(366, *Rt[k].shape[2:]) for k in KEYS}
    got["variance"] = Rt.variance.reshape(366)
    _close(got, want, True, "case7 resolved")
    # the three outputs of plot_all.py:194-196, restated in fp64 on the downloaded trajectories
    y64, t64 = yh.astype(np.float64), t.cpu().numpy().astype(np.float64)
    auc = np.sum((y64[:, 1:, 0] + y64[:, :-1, 0]) * 0.5 * np.diff(t64), axis=1)
    out3 = np.stack([auc, y64[:, :, 1].max(1), y64[:, 6:, 3].mean(1)], 1)
    np.testing.assert_allclose(out3, bench.sobol_outputs(y).cpu().numpy(), rtol=1e-5)             # (the benchmark's fp32 statement)
    got3 = {k: Si[k] for k in KEYS}
    got3["variance"] = Si.variance
    _close(got3, SR.analyze(out3, 7, True, 8, 3, Z95), True, "case7 outputs")
    num = Si.numpy()
    assert isinstance(num["S1"], np.ndarray) and num["names"] == bench.SOBOL_NAMES
    # a GE state that never moves: no residual on it, dGE = 0 in ODECore
    with torch.no_grad():
        last = [p for p in m.nn_residual.parameters()][-2:]
        assert tuple(last[0].shape) == (6, 64) and tuple(last[1].shape) == (6,)
        last[0][4].zero_()
        last[1][4].zero_()
    R0 = sobol_study(m, bounds, x0, t, {"meal": meal, "tVNS": tvns}, n=16, time_resolved=True, num_resamples=8, seed=3).resolved
    for k in KEYS:
        assert torch.isnan(R0[k][0]).all() and torch.isnan(R0[k][:, 4]).all(), k
    assert bool((R0.variance[:, 4] == 0).all()) and torch.isfinite(R0["S1"][7:, 0]).all()


def test_case7b_failed_solves_are_dropped_whole():
    """A box that reaches outside the model's range: base samples with a failed block leave the analysis, too many raise."""
    import bench
    dev = torch.device("cuda")
    m = bench.class_model(dev)
    x0, t, meal, tvns = (v.to(dev) for v in bench.sobol_inputs())

    class Failing:
        """The model with chosen solves marked failed after the launch."""
        def __init__(self, bad):
            self.bad = bad

        def forward_ode_sets(self, *a, **k):
            y = m.forward_ode_sets(*a, **k)
            self.last_solve_info = dict(m.last_solve_info)
            st = self.last_solve_info["status"].clone()
            st[self.bad] = 1
            self.last_solve_info["status"] = st
            return y

    bounds = dict(zip(bench.SOBOL_NAMES[:2], map(tuple, bench.SOBOL_BOUNDS[:2])))
    ext = {"meal": meal, "tVNS": tvns}
    full = sobol_study(m, bounds, x0, t, ext, n=16, num_resamples=0)
    one = sobol_study(Failing([6 * 3 + 1, 6 * 3 + 4]), bounds, x0, t, ext, n=16, num_resamples=0)      # two blocks of base sample 3
    assert full.n_dropped == 0 and one.n_dropped == 1
    sets = saltelli_design(bounds, n=16)
    y = m.forward_ode_sets({k: torch.as_tensor(sets[:, i], dtype=torch.float32) for i, k in enumerate(bounds)}, x0, t, ext)
    keep = np.r_[0:18, 24:96]
    want = SR.analyze(default_outputs(y, t, meal).cpu().numpy()[keep], 2, True, 0, 0, Z95)
    np.testing.assert_allclose(one.S1.cpu().numpy(), want["S1"], rtol=0, atol=ATOL)
    with pytest.raises(RuntimeError):
        sobol_study(Failing([0, 7, 13]), bounds, x0, t, ext, n=16, num_resamples=0)                       # 3 of 16 base samples


def test_case8_ishigami_within_its_own_confidence_of_the_exact_indices():
    Si = sobol_indices(_dev(_ishigami(1024)), 3, num_resamples=100, seed=0)
    s1, st, s2 = Si.S1.cpu().numpy(), Si.ST.cpu().numpy(), Si.S2.cpu().numpy()
    c1, ct, c2 = Si.S1_conf.cpu().numpy(), Si.ST_conf.cpu().numpy(), Si.S2_conf.cpu().numpy()
    print("S1", s1, c1, "ST", st, ct, "S2_13", s2[0, 2], c2[0, 2])
    assert s1.shape == (3,) and s2.shape == (3, 3)
    assert np.all(np.abs(s1 - SR.ISHIGAMI_S1) < c1) and np.all(np.abs(st - SR.ISHIGAMI_ST) < ct)
    assert abs(s2[0, 2] - SR.ISHIGAMI_S2_13) < c2[0, 2]
    # the same numbers as the restatement the host test holds to the same condition
    want = SR.analyze_column(_ishigami(1024), 3, True, 100, 0, Z95)
    np.testing.assert_allclose(s1, want["S1"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(c1, want["S1_conf"], rtol=0, atol=ATOL)
