"""Host-side pieces of bench.py that need no GPU: the kernel-source hash that stamps profiles/pmc_traffic.json."""
import os
import shutil

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_comment_stripper_keeps_code_and_string_literals():
    src = 'int a = 1; // trailing\n/* block\n comment */ const char *s = "// not a comment"; char c = \'"\';\n'
    out = bench._strip_c_comments(src)
    assert "trailing" not in out and "block" not in out
    assert '"// not a comment"' in out and "int a = 1;" in out and "'\"'" in out


def test_kernel_source_hash_ignores_comments_but_not_code(tmp_path):
    pkg = os.path.join("hybrid-ode-for-glp-1-and-glucose_amd", "csrc")
    dst = tmp_path / pkg
    shutil.copytree(os.path.join(ROOT, pkg), dst, ignore=shutil.ignore_patterns("_obj", "*.o", ".build.lock"))
    base = bench.kernel_source_sha(str(tmp_path))
    assert base == bench.kernel_source_sha()                      # same sources, other root
    f = dst / "hode_solve_fwd.hip"
    text = f.read_text()
    f.write_text("// a new comment line\n" + text.replace("namespace hode {", "namespace hode {   /* remark */", 1))
    assert bench.kernel_source_sha(str(tmp_path)) == base         # comments and white space do not count
    f.write_text(text.replace("dim3(64)", "dim3(64 )", 1).replace("return HODE_EUNSUPPORTED;", "return HODE_EUNSUPPORTED + 0;", 1))
    assert bench.kernel_source_sha(str(tmp_path)) != base         # code does


def test_committed_pmc_stamp_matches_the_committed_kernels():
    """profiles/pmc_traffic.json must have been taken on the kernels of this tree (bench.py drops the reading otherwise)."""
    import json

    import pytest
    stamp = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["kernel_source_sha"]
    if stamp != bench.kernel_source_sha():      # a reminder, not a gate: kernels may change in a container without a GPU
        pytest.skip("profiles/pmc_traffic.json is stale: re-run tools/profile_gpu.sh + tools/summarize_profile.py on the GPU box")


def test_binary_stamp_follows_the_sources(tmp_path, monkeypatch):
    """csrc/Makefile stamps libhode.so with a hash of its sources; hode/_build.py recomputes it from the tree.  The committed
    tree's binary is current; any change to a kernel source, a header, the C ABI header or the Makefile makes it stale, and a
    caller that may not build (bench.py --no-build: everything under rocprofv3) gets an error instead of a stale benchmark."""
    import pytest
    from hode import _build
    assert _build.is_current() and _build.source_stamp() == _build.binary_stamp()
    pkg = tmp_path / "pkg"
    shutil.copytree(os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd", "csrc"), pkg / "csrc",
                    ignore=shutil.ignore_patterns("_obj", "*.o", ".build.lock"))
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "include", "hode.h"), tmp_path / "include" / "hode.h")
    os.makedirs(pkg / "hode")
    shutil.copy(_build.SO, pkg / "hode" / "libhode.so")
    shutil.copy(_build.SO + ".srcsha", pkg / "hode" / "libhode.so.srcsha")
    monkeypatch.setattr(_build, "CSRC", str(pkg / "csrc"))
    monkeypatch.setattr(_build, "SO", str(pkg / "hode" / "libhode.so"))
    assert _build.is_current()                                        # same sources, other place
    f = pkg / "csrc" / "hode_optim.hip"
    f.write_text(f.read_text() + "\n// touched\n")
    assert not _build.is_current()
    with pytest.raises(RuntimeError, match="may not start a build"):
        _build.ensure(may_build=False)


def test_saltelli_design_of_the_sobol_leg():
    """bench.py's stand-in for SALib's saltelli.sample(problem, 1024) (reference plots/plot_all.py:139-158): N (2 D + 2) rows in the
    block layout A, AB_1..AB_D, BA_1..BA_D, B, inside the bounds of :140-148; the three outputs follow :191-193."""
    import numpy as np
    import bench
    s = bench.saltelli_sets(1024)
    D = len(bench.SOBOL_NAMES)
    assert s.shape == (1024 * (2 * D + 2), D) == (16384, 7)
    lo, hi = np.array(bench.SOBOL_BOUNDS).T
    assert (s >= lo).all() and (s <= hi).all()
    blk = s.reshape(1024, 2 * D + 2, D)
    A, B = blk[:, 0], blk[:, -1]
    for i in range(D):
        other = [j for j in range(D) if j != i]
        assert np.array_equal(blk[:, 1 + i][:, other], A[:, other]) and np.array_equal(blk[:, 1 + i][:, i], B[:, i])
        assert np.array_equal(blk[:, 1 + D + i][:, other], B[:, other]) and np.array_equal(blk[:, 1 + D + i][:, i], A[:, i])
    assert np.array_equal(bench.saltelli_sets(1024), s)           # seeded
    y = np.random.default_rng(0).random((5, 61, 6))
    want = np.stack([np.trapz(y[:, :, 0], dx=5 / 60, axis=1), y[:, :, 1].max(1), y[:, 6:, 3].mean(1)], 1)
    assert np.allclose(bench.sobol_outputs(y), want, rtol=1e-13)
    x0, t, meal, tvns = bench.sobol_inputs()
    assert x0.tolist() == [5.0, 60.0, 80.0, 0.0, 0.0, 1.0] and t.shape == (61,) and float(meal[0, 6]) == 75.0 and float(meal.sum()) == 75.0


def test_dump_outputs_writes_the_solution_and_samples_fixed_rows_when_too_large(tmp_path):
    """bench.py --dump-outputs: y (fp32) and status / nsteps / nfev (fp64) as <name>.npy; above the byte cap a seeded sample of
    trajectories (the same rows every run) is written, with their indices in rows.npy."""
    import types

    import numpy as np
    import torch
    B, T = 50, 7
    g = torch.Generator().manual_seed(0)
    sol = types.SimpleNamespace(y=torch.randn(B, T, 6, generator=g), status=torch.arange(B, dtype=torch.int32) % 3,
                                nsteps=torch.arange(B, dtype=torch.int32) + 100, nfev=torch.arange(B, dtype=torch.int32) * 6 + 2)
    full = tmp_path / "full"
    bench.dump_outputs(str(full), sol)
    assert sorted(os.listdir(full)) == ["nfev.npy", "nsteps.npy", "status.npy", "y.npy"]
    y = np.load(full / "y.npy")
    assert y.dtype == np.float32 and np.array_equal(y, sol.y.numpy())
    for k in ("status", "nsteps", "nfev"):
        v = np.load(full / f"{k}.npy")
        assert v.dtype == np.float64 and np.array_equal(v, getattr(sol, k).numpy())
    cap = 10 * (T * 6 * 4 + 32) + 1024                                # room for 10 trajectories + the .npy headers
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), sol, max_bytes=cap)
    bench.dump_outputs(str(b), sol, max_bytes=cap)
    rows = np.load(a / "rows.npy").astype(np.int64)
    assert len(rows) == 10 and np.all(np.diff(rows) > 0) and np.array_equal(rows, np.load(b / "rows.npy"))
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= cap
    assert np.array_equal(np.load(a / "y.npy"), sol.y.numpy()[rows])
    assert np.array_equal(np.load(a / "nfev.npy"), sol.nfev.numpy()[rows].astype(np.float64))


def test_plain_run_has_no_secondary_legs_and_full_has_them_all():
    """bench.py without --full times the headline and nothing else; --full adds every leg its --no-* options leave, the N = 1
    legs only when one process runs."""
    import bench
    base = ["--gpus", "1", "--steps", "5", "--warmup", "2"]
    assert bench.secondary_legs(bench.parse_args(base), 1) == set()
    assert bench.secondary_legs(bench.parse_args(base + ["--no-train", "--no-sobol"]), 1) == set()
    full = bench.secondary_legs(bench.parse_args(base + ["--full"]), 1)
    assert full == {"zscore", "train", "cpu_baseline", "vi", "generic", "data_side", "sobol", "class_path"}
    assert bench.secondary_legs(bench.parse_args(base + ["--full", "--no-train", "--no-sobol"]), 1) == full - {"train", "sobol"}
    assert bench.secondary_legs(bench.parse_args(["--gpus", "2", "--full"]), 2) == {"zscore", "train"}
    assert bench.secondary_legs(bench.parse_args(["--gpus", "2", "--full", "--no-zscore"]), 2) == {"train"}
