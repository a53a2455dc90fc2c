"""The Sobol indices without a GPU (inference/sobol.py, csrc/hode_sobol.hip): the C ABI's entry pair and its host-side argument
checks, the Saltelli design against the benchmark's, and the numpy restatement of the estimators (tests/_sobol_reference.py,
which the GPU tests hold the kernel to) on the Ishigami function, whose indices are known in closed form."""
import ctypes
import os
import re

import numpy as np
import pytest

import hode
from inference import SobolIndices, saltelli_design, sobol_indices, sobol_study  # noqa: F401  (the package exports the surface)

import _sobol_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


def test_header_declares_the_entry_pair_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "hode.h")).read()
    lib = ctypes.CDLL(hode.lib_path())
    for name in ("hode_sobol_indices_f32", "hode_sobol_indices_f64"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in hode.capi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+HODE_SOBOL_MAX_D\s+32\b", hdr) and hode.capi.SOBOL_MAX_D == 32


def _call(fn, N=4, D=3, M=2, Y=16, ldy=2, second=1, R=2, S1=16, ST=16, S2=16, S1c=16, STc=16, S2c=16, var=0):
    p = ctypes.c_void_p
    return fn(p(0), ctypes.c_int(N), ctypes.c_int(D), ctypes.c_int(M), p(Y), ctypes.c_int64(ldy), ctypes.c_int(second), ctypes.c_int(R),
              ctypes.c_uint64(0), ctypes.c_double(1.96), p(S1), p(ST), p(S2), p(S1c), p(STc), p(S2c), p(var))


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_arguments_are_rejected_on_the_host_before_any_launch(sfx):
    """Every case returns before a device is touched (there is none here): pointers are non-NULL but never dereferenced."""
    fn = getattr(hode.load(), f"hode_sobol_indices_{sfx}")
    for bad in (dict(N=0), dict(D=0), dict(M=0), dict(ldy=1), dict(R=-1), dict(Y=0), dict(S1=0), dict(ST=0), dict(S2=0),
                dict(S1c=0), dict(STc=0), dict(S2c=0), dict(N=-3), dict(D=-1)):
        assert _call(fn, **bad) == EINVAL, bad
    assert _call(fn, D=33) == EUNSUPPORTED
    assert _call(fn, D=33, second=0, S2=0, S2c=0) == EUNSUPPORTED
    assert _call(fn, D=33, Y=0) == EINVAL                  # a bad argument outranks an unsupported size


def test_saltelli_design_is_the_benchmarks_design_bit_for_bit():
    import bench
    for seed in (0, 3):
        ours = saltelli_design(dict(zip(bench.SOBOL_NAMES, bench.SOBOL_BOUNDS)), n=1024, seed=seed)
        assert ours.shape == (1024 * 16, 7) and np.array_equal(ours, bench.saltelli_sets(1024, seed=seed))


def test_saltelli_design_blocks_for_any_dimension_and_without_second_order():
    box = [(-1.0, 2.0), (0.0, 1.0), (3.0, 5.0), (-4.0, -2.0), (10.0, 20.0)]
    full = saltelli_design(box, n=8, seed=1).reshape(8, 12, 5)
    first = saltelli_design(box, n=8, calc_second_order=False, seed=1).reshape(8, 7, 5)
    A, B = full[:, 0], full[:, -1]
    lo, hi = np.array(box).T
    assert np.all(full >= lo) and np.all(full <= hi) and not np.array_equal(A, B)
    for j in range(5):
        other = [c for c in range(5) if c != j]
        assert np.array_equal(full[:, 1 + j, j], B[:, j]) and np.array_equal(full[:, 1 + j][:, other], A[:, other])       # AB_j
        assert np.array_equal(full[:, 6 + j, j], A[:, j]) and np.array_equal(full[:, 6 + j][:, other], B[:, other])       # BA_j
    assert np.array_equal(first[:, :6], full[:, :6]) and np.array_equal(first[:, 6], B)                                   # A, AB, B


def test_restatement_on_ishigami_lies_within_its_own_confidence_of_the_exact_indices():
    X = saltelli_design([(-np.pi, np.pi)] * 3, n=1024, seed=0)
    si = SR.analyze_column(SR.ishigami(X), 3, second=True, R=100, seed=0)
    print("S1", si["S1"], si["S1_conf"], "ST", si["ST"], si["ST_conf"], "S2_13", si["S2"][0, 2], si["S2_conf"][0, 2])
    assert np.all(np.abs(si["S1"] - SR.ISHIGAMI_S1) < si["S1_conf"])
    assert np.all(np.abs(si["ST"] - SR.ISHIGAMI_ST) < si["ST_conf"])
    assert abs(si["S2"][0, 2] - SR.ISHIGAMI_S2_13) < si["S2_conf"][0, 2]
    assert np.all(np.isnan(si["S2"][np.tril_indices(3)])) and np.all(np.isfinite(si["S2"][np.triu_indices(3, 1)]))
    # first-order design: the same S1 / ST estimators on the A, AB, B blocks alone
    keep = np.r_[0:4, 7]
    s1 = SR.analyze_column(SR.ishigami(X).reshape(1024, 8)[:, keep].reshape(-1), 3, second=False, R=0)
    assert np.all(np.abs(s1["S1"] - SR.ISHIGAMI_S1) < 0.02) and np.all(np.isnan(s1["S1_conf"])) and np.all(np.isnan(s1["S2"]))


def test_restatement_resampling_and_degenerate_columns():
    rho = SR.resample_indices(5 << 33 | 9, 2, 1000)
    assert rho.min() >= 0 and rho.max() < 1000 and len(set(rho.tolist())) > 500
    assert np.array_equal(rho[:10], SR.resample_indices(5 << 33 | 9, 2, 10 ** 3)[:10])
    assert not np.array_equal(rho, SR.resample_indices(5 << 33 | 9, 3, 1000))
    assert np.all(SR.resample_indices(1, 0, 1) == 0)
    y = np.random.default_rng(0).standard_normal(40)
    const = SR.analyze_column(np.full(40, 2.5), 3, R=4)
    assert np.all(np.isnan(const["S1"])) and np.all(np.isnan(const["ST_conf"])) and const["variance"] == 0.0
    y[7] = np.nan
    assert np.isnan(SR.analyze_column(y, 3, R=4)["variance"])


def test_sobol_indices_needs_the_device():
    """No CPU fallback: a host tensor raises."""
    torch = pytest.importorskip("torch")
    with pytest.raises(hode.HodeError):
        sobol_indices(torch.zeros(16, 2), 3)
