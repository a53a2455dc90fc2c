"""eval/evaluate.py and the predictive_summary entry points on the GPU against the NumPy restatement
(tests/_predictive_reference.py) applied to the trajectories the existing surface returns, and against the values captured from
the reference (tests/golden/eval/calibration.npz).  Model: the h32_l2 golden weights; B = 3, T = 13; the loader is a list of two
batches.  `-m gpu`.

Tolerance: the solves behind `evaluate_model` / `predictive_summary` run as batched parameter sets cut into pieces, the
restatement is fed `forward_param_sets` / `predict` of ALL draws; test_sobol_gpu.py
(test_shared_network_launch_equals_one_network_copy_per_set) holds batched sets and per-set solves to torch.equal, so the
trajectories carry no tolerance of their own and what is left is the kernels' FP64_TOL of test_predictive_gpu.py (fp32 outputs:
2e-7)."""
import os

import numpy as np
import pytest

import _predictive_reference as PR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FP64_TOL = 1.1e-11
FP32_TOL = 2e-7
B, T = 3, 13
STATES = ("glucose", "insulin", "glucagon", "glp1", "ge", "ffa")
POINT_KEYS = {"rmse", "mae", "nrmse"} | {f"{p}_{s}" for p in ("rmse", "mae", "nrmse") for s in STATES}
CAL_KEYS = {"ece", "msis", "sharpness", "coverage_95", "mean_normalized_error"}
THR = PR.thresholds(10)


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
def loader(golden_dir):
    g = np.load(os.path.join(golden_dir, "g4_t61_pulses.npz"))
    rng = np.random.default_rng(5)
    out = []
    for lo in (0, B):
        obs = g["y_rk45_tight"][lo:lo + B, :T].astype(np.float64) * (1.0 + 0.05 * rng.standard_normal((B, T, 6)))
        obs[rng.random((B, T, 6)) < 0.05] = np.nan
        out.append({"initial_state": torch.tensor(g["x0"][lo:lo + B]), "observations": torch.tensor(obs, dtype=torch.float32),
                    "time_points": torch.tensor(g["t"][:T]),
                    "external_inputs": {"meal": torch.tensor(g["meal"][lo:lo + B, :T]), "tVNS": torch.tensor(g["tvns"][lo:lo + B, :T])}})
    return out


def _restated_table(blocks, loader, sigma=None):
    """Sum over the batches of the restatement's table for draws blocks[i] [S, B, T, 6] of batch i."""
    table = 0
    outs = []
    for y, batch in zip(blocks, loader):
        y = y.detach().cpu().numpy().astype(np.float64)
        obs = batch["observations"].numpy().astype(np.float64).reshape(-1)
        S = y.shape[0]
        sig = None if sigma is None else np.tile(np.asarray(sigma, dtype=np.float64), (S, 1))
        st = PR.fold(PR.fresh_state(obs.size), y.reshape(S, -1), obs, None, sig)
        mean, sd, pit, t, edges = PR.score(st, obs, None, None if sig is None else (sig ** 2).mean(0), THR)
        assert PR.clear_of_edges(edges)
        table = table + t
        outs.append((mean, sd, pit))
    return table, outs


def _check_metrics(out, want, keys_cal=False):
    np.testing.assert_allclose(out["rmse"], want["rmse"], rtol=FP64_TOL)
    np.testing.assert_allclose(out["mae"], want["mae"], rtol=FP64_TOL)
    np.testing.assert_allclose(out["nrmse"], want["rmse"] / np.mean(want["target_std_per_state"]), rtol=FP64_TOL)
    for k, s in enumerate(STATES):
        np.testing.assert_allclose(out[f"rmse_{s}"], want["rmse_per_state"][k], rtol=FP64_TOL)
        np.testing.assert_allclose(out[f"mae_{s}"], want["mae_per_state"][k], rtol=FP64_TOL)
        np.testing.assert_allclose(out[f"nrmse_{s}"], want["rmse_per_state"][k] / want["target_std_per_state"][k], rtol=FP64_TOL)
    if keys_cal:
        for k in CAL_KEYS:
            np.testing.assert_allclose(out[k], want[k], rtol=FP64_TOL, err_msg=k)


def test_evaluate_model_point_path(golden_dir, loader, tmp_path):
    from eval.evaluate import evaluate_model, save_evaluation_results
    m = _model(golden_dir)
    out = evaluate_model(m, loader, torch.device("cuda"))
    assert set(out) == POINT_KEYS
    with torch.no_grad():
        blocks = [m.forward(b["initial_state"], b["time_points"], b["external_inputs"]).unsqueeze(0) for b in loader]
    table, _ = _restated_table(blocks, loader)
    assert (table[:, 5:] == 0).all()                              # one draw: no uncertainty columns
    _check_metrics(out, PR.metrics(table, 10))
    # with observation noise the predictive has a density: the extra keys appear, the reference's keys do not move
    noisy = evaluate_model(m, loader, torch.device("cuda"), noise_sigma=[6.0, 0.8, 3.0, 0.4, 0.03, 0.02])
    assert set(noisy) == POINT_KEYS | {"crps", "lppd", "pit_histogram"} and all(noisy[k] == out[k] for k in POINT_KEYS)
    assert np.isnan(noisy["crps"]) and np.isnan(noisy["lppd"])   # ... and one draw has no spread to score
    p = tmp_path / "ev.csv"
    save_evaluation_results(out, str(p))
    rows = p.read_text().splitlines()
    assert rows[0].split(",") == list(out) and len(rows) == 2 and "Per-State RMSE:" in (tmp_path / "ev.txt").read_text()


def test_evaluate_model_variational_path_in_pieces(golden_dir, loader):
    from eval.evaluate import evaluate_model
    m = _model(golden_dir, variational=True)
    torch.manual_seed(3)
    out = evaluate_model(m, loader, torch.device("cuda"), use_variational=True, n_posterior_samples=5, max_bytes=2 * B * T * 6 * 4)
    assert set(out) == POINT_KEYS | CAL_KEYS
    torch.manual_seed(3)
    blocks = []
    with torch.no_grad():
        for b in loader:
            draws = [m.variational_params.sample(1)[0] for _ in range(5)]          # one at a time, per batch
            blocks.append(m.forward_param_sets(draws, b["initial_state"], b["time_points"], b["external_inputs"]))
            assert m.solve_failures() == 0
    table, _ = _restated_table(blocks, loader)
    assert table[:, 5].sum() == table[:, 0].sum() > 0
    _check_metrics(out, PR.metrics(table, 10), keys_cal=True)
    # the cut changes memory and nothing else
    torch.manual_seed(3)
    whole = evaluate_model(m, loader, torch.device("cuda"), use_variational=True, n_posterior_samples=5)
    assert all(np.array_equal(whole[k], out[k]) for k in out)
    # VariationalInference.predictive_summary: the same draws of the first batch, per-entry outputs too
    from inference import VariationalInference
    torch.manual_seed(3)
    summ = VariationalInference(m, device=torch.device("cuda")).predictive_summary(loader[0], n_samples=5, max_bytes=2 * B * T * 6 * 4)
    _, outs = _restated_table(blocks[:1], loader[:1])
    for got, want in zip((summ.mean, summ.std, summ.pit), outs[0]):
        np.testing.assert_allclose(got.cpu().numpy().reshape(-1).astype(np.float64), want, rtol=FP32_TOL, equal_nan=True)


@pytest.mark.parametrize("noise", [False, True])
def test_hmc_result_predictive_summary_from_arrays(golden_dir, loader, noise):
    from inference.hmc import HMCResult
    from inference.observation import ObservationModel
    m = _model(golden_dir)
    batch = loader[1]
    nn_base, ode_base = m._params_on(torch.device("cuda"))
    rng = np.random.default_rng(9)
    mu = np.array([0.025, 7.0])
    draws = torch.tensor(mu * (1.0 + 0.05 * rng.standard_normal((2, 4, 2))), dtype=torch.float32, device="cuda")
    sigma = [6.0, 0.8, 3.0, 0.4, 0.03, 0.02]
    res = HMCResult(draws, ["k_I", "K_m"], [], {}, m, ode_base.detach(), nn_base.detach(), ObservationModel(sigma), batch)
    summ = res.predictive_summary(thin=2, observation_noise=noise, max_bytes=3 * B * T * 6 * 4)
    y = res.predict(batch["initial_state"], batch["time_points"], batch["external_inputs"], thin=2)
    assert tuple(y.shape) == (4, B, T, 6) and int((summ.n != 4).sum()) == 0
    table, outs = _restated_table([y], [batch], sigma if noise else None)
    for got, want in zip((summ.mean, summ.std, summ.pit), outs[0]):
        np.testing.assert_allclose(got.cpu().numpy().reshape(-1).astype(np.float64), want, rtol=FP32_TOL, equal_nan=True)
    cols = [0, 5, 9, 10, 11, 12, 15] + list(range(16, 36))
    assert np.array_equal(summ.table[:, cols], table[:, cols])
    np.testing.assert_allclose(summ.table, table, rtol=FP64_TOL, atol=0)
    assert (table[:, 15].sum() > 0) == noise
    m_ = summ.metrics()
    assert np.isfinite(m_["crps"]) and np.isfinite(m_["lppd"]) == noise


@pytest.mark.parametrize("tag", ["a", "b"])
def test_metric_functions_reproduce_the_reference_fixture(golden_dir, tag):
    """The rule of test_predictive_host.py: deterministic keys to 1e-12 relative, ece inside the reference's spread."""
    from eval.evaluate import compute_calibration_error, compute_mae, compute_rmse
    g = np.load(os.path.join(golden_dir, "eval", "calibration.npz"))
    p, u, t = (torch.tensor(g[f"{tag}_{k}"]) for k in ("predictions", "uncertainties", "targets"))
    cal = compute_calibration_error(p, u, t)
    assert set(cal) == CAL_KEYS and all(isinstance(v, float) for v in cal.values())
    for k in ("msis", "sharpness", "coverage_95", "mean_normalized_error"):
        assert abs(cal[k] - float(g[f"{tag}_{k}"])) <= 1e-12 * abs(float(g[f"{tag}_{k}"])), k
    assert float(g[f"{tag}_ece_min"]) <= cal["ece"] <= float(g[f"{tag}_ece_max"])
    assert cal["ece"] == PR.calibration(p.numpy(), u.numpy(), t.numpy())[0]["ece"]          # counts: exactly the restatement's
    for fn, k in ((compute_rmse, "rmse"), (compute_mae, "mae")):
        v, per = fn(p, t), fn(p, t, per_state=True)
        assert isinstance(v, float) and isinstance(per, np.ndarray) and per.shape == (6,)
        assert abs(v - float(g[f"{tag}_{k}"])) <= 1e-12 * float(g[f"{tag}_{k}"])
        np.testing.assert_allclose(per, g[f"{tag}_{k}_per_state"], rtol=1e-12, atol=0)
    assert isinstance(compute_rmse(p.float(), t.float()), float)                           # fp32 tensors take the fp32 kernel
