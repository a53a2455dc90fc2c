"""Host-side tests of the HMC sampler (no GPU): the C ABI of the MCMC section (declared, exported, listed; argument
validation before any launch), the Philox stream against rocRAND's host-callable engine, the static checks of the kernel
source (DPP / LDS hazards, 0 bytes of scratch), and the host half of HMCResult (sample naming, R-hat, ESS)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import hode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW = [f"hode_{n}_{s}" for n in ("mse_sets", "hmc_refresh", "hmc_leapfrog", "hmc_accept", "hmc_welford") for s in ("f32", "f64")]
EINVAL = -1
P_, I_ = ctypes.c_void_p, ctypes.c_int


def test_mcmc_entry_points_are_declared_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "hode.h")).read()
    declared = set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(hode.lib_path())
    for name in NEW:
        assert name in declared and name in hode.capi.SYMBOLS and hasattr(lib, name), name


def test_bad_sizes_and_null_pointers_are_rejected_before_any_launch():
    """Fake device pointers: every call below must fail on the host, before anything is dereferenced or launched."""
    lib = ctypes.CDLL(hode.lib_path())
    f = P_(256)
    N = P_(0)
    d, u64, u32 = ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32
    for sfx, real in (("f32", ctypes.c_float), ("f64", ctypes.c_double)):
        mse = getattr(lib, f"hode_mse_sets_{sfx}")
        assert mse(N, I_(-1), ctypes.c_int64(8), f, f, real(1.0), f, f) == EINVAL
        assert mse(N, I_(2), ctypes.c_int64(-8), f, f, real(1.0), f, f) == EINVAL
        assert mse(N, I_(2), ctypes.c_int64(8), N, f, real(1.0), f, f) == EINVAL
        assert mse(N, I_(2), ctypes.c_int64(8), f, f, real(1.0), N, f) == EINVAL
        ref = getattr(lib, f"hode_hmc_refresh_{sfx}")
        ok = [f] * 12
        for C, D, ld in ((0, 4, 4), (2, 0, 4), (2, 8, 4)):
            assert ref(N, I_(C), I_(D), I_(ld), u64(0), u32(0), d(0.1), *ok) == EINVAL
        assert ref(N, I_(2), I_(4), I_(4), u64(0), u32(0), d(1.5), *ok) == EINVAL           # jitter outside [0, 1)
        for k in range(12):
            args = list(ok)
            args[k] = N
            assert ref(N, I_(2), I_(4), I_(4), u64(0), u32(0), d(0.1), *args) == EINVAL, k
        lf = getattr(lib, f"hode_hmc_leapfrog_{sfx}")

        def leap(C=2, D=7 + 13510, ld=13520, flags=15, P=13510, n_traj=4, mask=0b11100100100111, sample_nn=1, nulls=()):
            a = dict(eps=f, minv=f, z=f, p=f, g=f, gnn=f, gode=f, loss=f, status=f, U=f, ke=f, failed=f, mu=f, sd=f, nn_p=f, ode_p=f)
            for k in nulls:
                a[k] = N
            return lf(N, I_(C), I_(D), I_(ld), I_(flags), d(0.5), a["eps"], a["minv"], a["z"], a["p"], a["g"], a["gnn"], a["gode"], I_(P),
                      a["loss"], d(0.5), a["status"], I_(n_traj), a["U"], a["ke"], a["failed"], u32(mask), a["mu"], a["sd"], I_(sample_nn),
                      a["nn_p"], a["ode_p"])
        assert leap(D=7 + 13509) == EINVAL                     # D != popcount(mask) + P
        assert leap(mask=1 << 17) == EINVAL                    # only 17 constants
        assert leap(flags=64) == EINVAL
        assert leap(n_traj=0) == EINVAL
        for k in ("eps", "minv", "z", "p", "g", "U", "failed", "ke", "mu", "nn_p", "ode_p"):
            assert leap(nulls=(k,)) == EINVAL, k
        acc = getattr(lib, f"hode_hmc_accept_{sfx}")

        def accept(C=2, mode=0, delta=0.8, n_ode=7, slot=0, n_slots=4, nulls=()):
            a = [f] * 13
            for k in nulls:
                a[k] = N
            return acc(N, I_(C), I_(20), I_(20), I_(mode), u64(0), u32(0), d(delta), *a[:12], I_(n_ode), a[12], f, f, f, I_(n_slots),
                       I_(slot))
        assert accept(C=0) == EINVAL and accept(mode=7) == EINVAL and accept(delta=1.0) == EINVAL and accept(n_ode=18) == EINVAL
        assert accept(slot=4) == EINVAL
        for k in range(13):
            assert accept(nulls=(k,)) == EINVAL, k
        wf = getattr(lib, f"hode_hmc_welford_{sfx}")
        assert wf(N, I_(2), I_(8), I_(8), I_(0), f, f, f) == EINVAL
        assert wf(N, I_(2), I_(8), I_(8), I_(1), N, f, f) == EINVAL
        assert wf(N, I_(2), I_(8), I_(8), I_(2), f, f, N) == EINVAL
        assert wf(N, I_(2), I_(8), I_(4), I_(1), f, f, f) == EINVAL


PHILOX_CHECK = r'''
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_philox4x32_10.h>
#include <cstdio>
#include "hode_philox.h"
int main() {
    const unsigned long long seeds[3] = {0ull, 12345ull, 0xDEADBEEF12345678ull};
    int bad = 0, n = 0;
    for (auto seed : seeds) for (uint32_t chain : {0u, 1u, 1023u}) for (uint32_t it : {0u, 7u, 0x80000003u})
    for (uint32_t tag : {0u, 1u, 2u, 3u}) for (uint32_t grp : {0u, 5u, 3379u}) {
        // key (seed lo, chain), counter (group, tag, iteration, seed hi)
        rocrand_device::philox4x32_10_engine e((seed & 0xffffffffull) | ((unsigned long long)chain << 32),
                                              (unsigned long long)it | ((seed >> 32) << 32),
                                              4ull * ((unsigned long long)grp | ((unsigned long long)tag << 32)));
        const uint4 r = e.next4();
        const hode::Philox4 m = hode::hmc_rng(seed, chain, it, tag, grp);
        bad += !(r.x == m.x && r.y == m.y && r.z == m.z && r.w == m.w);
        ++n;
    }
    printf("%d of %d differ\n", bad, n);
    return bad != 0;
}
'''


def test_philox_matches_rocrand_host_engine():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "philox_check.cpp"), os.path.join(tmp, "philox_check")
        open(src, "w").write(PHILOX_CHECK)
        subprocess.run([HIPCC, "-O1", "-std=c++17", f"-I{CSRC}", src, "-o", exe], check=True, capture_output=True, timeout=600)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 of 324 differ" in r.stdout, r.stdout + r.stderr


def test_no_dpp_or_lds_hazard_in_the_sampler_source():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dpp_hazard_check.py"), os.path.join(CSRC, "hode_hmc.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "0 hazard(s)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_sampler_kernels_use_no_scratch():
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "--cuda-device-only", "-c",
                            os.path.join(CSRC, "hode_hmc.hip"), "-o", os.path.join(tmp, "hmc.o"), "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {"mse_sets_kernel", "refresh_kernel", "leapfrog_kernel", "accept_kernel", "welford_kernel"}
    assert {k for k in kernels if any(k in n for n in names)} == kernels
    assert len(names) == len(scratch) >= 10 and all(s == 0 for s in scratch), list(zip(names, scratch))


# ------------------------------------------------------------------ HMCResult on the host
def _nn_shapes(H, L):
    from models.nn_residual import NNResidual
    return [(n, tuple(p.shape)) for n, p in NNResidual(9, H, 6, n_layers=L).named_parameters()]


@pytest.mark.parametrize("H,L", [(64, 4), (32, 2)])
def test_sample_keys_and_shapes_follow_run_nuts(H, L):
    from inference.hmc import REFERENCE_PRIORS, HMCResult
    from models.ode_core import ODE_PARAM_NAMES
    names = [n for n in ODE_PARAM_NAMES if n in REFERENCE_PRIORS]
    nn = _nn_shapes(H, L)
    P = hode.n_params(H, L)
    C, n = 3, 5
    draws = torch.randn(C, n, len(names) + P, dtype=torch.float64)
    res = HMCResult(draws, names, nn, {})
    s = res.samples
    # reference mcmc.py:109-113: 'ode.<name>' for the seven constants, 'nn.<parameter name>' for every MLP tensor
    assert list(s) == [f"ode.{k}" for k in names] + [f"nn.{k}" for k, _ in nn]
    assert names == ["a_GI", "k_I", "rho", "E_max", "V_max", "K_m", "k_L"]
    for k, shape in nn:
        assert s[f"nn.{k}"].shape == (C, n) + shape
    assert s["ode.k_L"].shape == (C, n)
    np.testing.assert_array_equal(s["ode.rho"], draws[:, :, 2].numpy())
    np.testing.assert_array_equal(s[f"nn.{nn[-1][0]}"], draws[:, :, -6:].numpy())
    f = res.flat()
    assert f["ode.a_GI"].shape == (C * n,) and f[f"nn.{nn[0][0]}"].shape == (C * n,) + nn[0][1]
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "mcmc_samples.npz"), **s)          # what the reference trainer does (train_hybrid.py:516)
        back = np.load(os.path.join(tmp, "mcmc_samples.npz"))
        assert set(back.files) == set(s)


def _ar1(M, N, K, phi, g):
    x = torch.empty(M, N, K, dtype=torch.float64)
    e = torch.randn(M, N, K, dtype=torch.float64, generator=g)
    x[:, 0] = e[:, 0] / np.sqrt(1 - phi * phi)
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return x


def test_ess_of_ar1_chains():
    from inference.hmc import HMCResult
    g = torch.Generator().manual_seed(3)
    M, N, K, phi = 8, 4000, 6, 0.5
    res = HMCResult(_ar1(M, N, K, phi, g), [], [], {})
    ess = res.ess()
    want = M * N * (1 - phi) / (1 + phi)
    assert ess.shape == (K,)
    assert float((ess / want - 1).abs().max()) < 0.10, (ess / want).tolist()


def test_rhat_separates_mixed_from_shifted_chains():
    from inference.hmc import HMCResult
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 1000, 5, dtype=torch.float64, generator=g)
    assert float(HMCResult(x, [], [], {}).rhat().max()) < 1.01
    y = x.clone()
    y[3] += 2.0                                                      # one chain somewhere else
    assert float(HMCResult(y, [], [], {}).rhat().min()) > 1.1


def test_import_without_arviz():
    r = subprocess.run([sys.executable, "-c", "import sys; sys.modules['arviz'] = None; from inference.hmc import run_hmc; print('ok')"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")])))
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
