"""Host-side checks of the latent initial-state model (no GPU): the argument checks of InitialStatePrior and of the samplers'
entry points before any device is touched, from_batch against numpy, the numpy restatement (tests/_initial_state_restatement.py)
against its own transpose, a LatentStateResult built from arrays, the return codes of the two kernels' entry points without a
launch, and the declared / listed / exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import _initial_state_restatement as XR

torch = pytest.importorskip("torch")
import hode  # noqa: E402

MEAN = [8.0, 90.0, 80.0, 10.0, 0.5, 0.5]
SD = [1.0, 9.0, 8.0, 1.0, 0.1, 0.05]


def test_prior_argument_checks():
    from inference.initial_state import STATE_NAMES, InitialStatePrior
    assert STATE_NAMES == ("G", "I", "Glu", "GLP1", "GE", "FFA")
    p = InitialStatePrior(MEAN, SD)
    assert p.states == [0, 1, 2, 3, 4, 5] and p.n_lat == 6 and p.link == "identity"
    p = InitialStatePrior(MEAN, SD, states=("GE", "I"), link="log")
    assert p.states == [1, 4] and p.n_lat == 2 and p.state_names == ["I", "GE"] and p.lat_mask == 0b10010
    assert InitialStatePrior(MEAN, SD, states=(4, 1)).states == [1, 4]
    assert InitialStatePrior(np.tile(MEAN, (3, 1)), np.tile(SD, (3, 1)), states=("G",)).bind(3).m.shape == (3, 6)
    # only the latent entries are read: a zero sd or a non-positive mean elsewhere is fine
    InitialStatePrior([8.0, 90.0, 80.0, 10.0, 0.0, 0.5], [1.0, 9.0, 0.0, 1.0, 0.1, 0.05], states=("G", "I"), link="log")
    bad = [dict(states=("G", "no_such_state")), dict(states=(6,)), dict(states=(-1,)), dict(states=()), dict(states=("G", "G")),
           dict(link="logit"), dict(sd=[1.0, 0.0, 1.0, 1.0, 1.0, 1.0]), dict(sd=[1.0, -1.0, 1.0, 1.0, 1.0, 1.0]),
           dict(sd=[1.0, float("nan"), 1.0, 1.0, 1.0, 1.0]), dict(mean=[1.0] * 5), dict(sd=np.ones((2, 3, 6))),
           dict(mean=[8.0, 90.0, 80.0, 10.0, 0.0, 0.5], link="log"), dict(mean=[8.0, -90.0, 80.0, 10.0, 0.5, 0.5], link="log"),
           dict(mean=[8.0, float("inf"), 80.0, 10.0, 0.5, 0.5])]
    for kw in bad:
        with pytest.raises(ValueError):
            InitialStatePrior(**{"mean": MEAN, "sd": SD, **kw})
    with pytest.raises(ValueError):
        InitialStatePrior(np.tile(MEAN, (3, 1)), SD).bind(4)               # [B, 6] rows against another batch size


def test_docstring_warns_against_the_first_observation_as_the_prior():
    from inference import initial_state as IS
    for doc in (IS.__doc__, IS.InitialStatePrior.__doc__):
        assert "first observation" in doc and "twice" in doc


def test_sampler_argument_errors_raise_before_any_device_is_touched(monkeypatch):
    import models.hybrid_ode_nn as HN
    from inference import InitialStatePrior, run_population
    from inference.hmc import run_hmc
    from inference.nuts import run_nuts

    def no_device():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(HN, "_compute_device", no_device)
    x0 = torch.tensor([[8.0, 90.0, 80.0, 10.0, 0.0, 0.5]] * 3)
    data = {"initial_state": x0, "observations": torch.zeros(3, 5, 6), "time_points": torch.linspace(0, 1, 5)}
    prior = InitialStatePrior(MEAN, SD, states=("I", "GE"))
    nan_fixed = dict(data, initial_state=x0.clone())
    nan_fixed["initial_state"][1, 0] = float("nan")                        # G is not latent
    nan_latent = dict(data, initial_state=x0.clone())
    nan_latent["initial_state"][1, 4] = float("nan")                       # GE is: allowed
    from inference.initial_state import _bind
    assert _bind(prior, nan_latent, None).B == 3
    for run in (run_hmc, run_nuts):
        with pytest.raises(ValueError, match="sample_nn"):
            run(None, data, initial_state=prior)                           # sample_nn defaults to True
        with pytest.raises(ValueError, match="sample_nn"):
            run(None, data, initial_state=prior, sample_nn=True)
        bad = [dict(data=nan_fixed), dict(data=None), dict(data=None, n_patients=0), dict(n_patients=4), dict(initial_state="I"),
               dict(initial_state=InitialStatePrior(np.tile(MEAN, (2, 1)), np.tile(SD, (2, 1)))), dict(noise_sigma=-1.0)]
        for kw in bad:
            with pytest.raises(ValueError):
                run(None, **{"data": data, "initial_state": prior, "sample_nn": False, **kw})
    for kw in (dict(data=nan_fixed), dict(data=None), dict(initial_state="I")):
        a = {"data": data, "initial_state": prior, **kw}
        with pytest.raises(ValueError):
            run_population(None, a.pop("data"), **a)


def test_from_batch_against_numpy_on_a_batch_with_nans():
    from inference import InitialStatePrior
    rng = np.random.default_rng(3)
    B, T = 9, 4
    obs = np.array(MEAN) * (1 + 0.1 * rng.standard_normal((B, T, 6)))
    obs[0, 0, 1] = obs[4, 0, 1] = np.nan
    obs[:, 0, 4] = np.nan
    obs[2:, 0, 3] = np.nan                                              # GLP1: two patients left
    obs[1:, 0, 5] = np.nan                                              # FFA: one patient left
    batch = {"observations": torch.as_tensor(obs)}
    for states, inflate, link in ((("G", "I"), 1.0, "identity"), (("I", "GLP1"), 2.5, "log"), ((0, 1, 2, 3), 1.0, "identity")):
        p = InitialStatePrior.from_batch(batch, states=states, link=link, inflate=inflate)
        mean, sd = XR.from_batch(obs[:, 0], p.states, inflate)
        assert p.link == link and p.mean.shape == (6,)
        np.testing.assert_allclose(p.mean.numpy()[p.states], mean[p.states], rtol=1e-14)
        np.testing.assert_allclose(p.sd.numpy()[p.states], sd[p.states], rtol=1e-13)
    for states in (("GE",), ("FFA",), None):
        with pytest.raises(ValueError):
            InitialStatePrior.from_batch(batch, states=states)
    # a mask hides entries as NaN does
    mask = torch.ones(B, T, 6, dtype=torch.bool)
    mask[3, 0, 0] = False
    p = InitialStatePrior.from_batch({"observations": torch.as_tensor(obs), "observation_mask": mask}, states=("G",))
    hidden = obs[:, 0].copy()
    hidden[3, 0] = np.nan
    np.testing.assert_allclose(p.mean.numpy()[0], XR.from_batch(hidden, [0])[0][0], rtol=1e-14)


@pytest.mark.parametrize("link", [0, 1])
@pytest.mark.parametrize("B,lat,off", [(1, [1], 0), (3, [0, 1, 2, 3, 4, 5], 7), (5, [1, 4], 14)])
def test_restatement_transpose_equals_central_differences_of_the_restatement_map(B, lat, off, link):
    """<J v, G> = <v, J^T G> with J v from central differences of the map along v, relative to the summed magnitudes of the terms
    of <v, J^T G>.  h = 1e-6: the truncation is h^2 / 6 times third derivatives (s^3 x0 for the log link, s ~ 0.1: 1e-16
    relative), the rounding of the difference quotient eps |x0| / h relative to |J v| ~ s |x0| = 0.1 |x0|: 2.2e-16 / 1e-6 / 0.1 =
    2.2e-9 per term, summed in quadrature over few terms: 5e-9 is asserted, the bound of the population model's check."""
    rng = np.random.default_rng(10 * B + off + link)
    n_lat, K, h = len(lat), min(off, 7), 1e-6
    m = np.array(MEAN) * (1 + 0.1 * rng.standard_normal((B, 6)))
    s = 0.1 * np.abs(m) + 0.01
    idx = sorted(int(j) for j in rng.choice(17, K, replace=False))
    mu, sd = rng.uniform(0.01, 10.0, max(K, 1)), rng.uniform(0.01, 1.0, max(K, 1))
    base, x0_base = rng.uniform(0.5, 2.0, 17), rng.uniform(0.5, 2.0, (B, 6))
    D = off + B * n_lat
    for trial in range(4):
        c, v = rng.standard_normal((1, D)), rng.standard_normal((1, D))
        gx0, gode = rng.standard_normal((1, B, 6)), rng.standard_normal((1, 17))
        Jx = (XR.x0_params(c + h * v, off, B, lat, link, m, s, x0_base)[0] - XR.x0_params(c - h * v, off, B, lat, link, m, s, x0_base)[0]) / (2 * h)
        Jo = (XR.ode_params(c + h * v, idx, mu, sd, base)[0] - XR.ode_params(c - h * v, idx, mu, sd, base)[0]) / (2 * h)
        g, mag = XR.x0_transpose(c, off, B, lat, link, m, s, gx0)
        go = XR.ode_transpose(gode, idx, sd)
        lhs = float((Jx * gx0).sum() + (Jo * gode).sum())
        rhs = float((v[:, off:] * g).sum() + (v[:, :K] * go).sum())
        scale = float((np.abs(v[:, off:]) * mag).sum() + (np.abs(v[:, :K]) * np.abs(go)).sum())
        assert abs(lhs - rhs) <= 5e-9 * scale, (lhs, rhs, scale)
        fixed = [j for j in range(6) if j not in lat]
        assert np.array_equal(XR.x0_params(c, off, B, lat, link, m, s, x0_base)[0][0][:, fixed], x0_base[:, fixed])


def test_result_from_arrays_maps_raw_draws_as_the_restatement_does():
    from inference import InitialStatePrior, LatentStateResult
    rng = np.random.default_rng(5)
    C, n, B, names = 3, 40, 4, ["a_GI", "k_L"]
    K = len(names)
    mu, sd = np.array([0.0104, 0.02]), np.array([0.002, 0.005])
    x0_base = np.array(MEAN) * (1 + 0.1 * rng.standard_normal((B, 6)))
    x0_base[1, 4] = np.nan
    for link in ("identity", "log"):
        prior = InitialStatePrior(MEAN, SD, states=("I", "GE"), link=link)
        lat = prior.bind(B, torch.as_tensor(x0_base))
        raw = rng.standard_normal((C, n, K + B * 2))
        r = LatentStateResult(torch.as_tensor(raw), names, mu, sd, lat)
        want = XR.x0_lat(raw[..., K:].reshape(C, n, B, 2), lat.m.numpy(), lat.s.numpy(), [1, 4], int(link == "log"))
        np.testing.assert_allclose(r.draws[..., :K].numpy(), mu + sd * raw[..., :K], rtol=1e-14)
        np.testing.assert_allclose(r.draws[..., K:].numpy().reshape(C, n, B, 2), want, rtol=1e-14)
        x0 = r.initial_states().numpy()
        assert x0.shape == (C, n, B, 6) and np.all(np.isfinite(x0))
        np.testing.assert_allclose(x0[..., [1, 4]], want, rtol=1e-14)
        assert np.array_equal(x0[..., [0, 2, 3, 5]], np.broadcast_to(x0_base[:, [0, 2, 3, 5]], (C, n, B, 4)))
        s = r.samples
        assert list(s) == ["ode.a_GI", "ode.k_L", "x0"] and s["x0"].shape == (C, n, B, 2) and s["ode.k_L"].shape == (C, n)
        assert tuple(r.rhat().shape) == (K + B * 2,) and tuple(r.ess("mean").shape) == (K + B * 2,)
        assert r.n_chains == C and r.n_draws == n and torch.equal(r.raw, torch.as_tensor(raw))
        with pytest.raises(ValueError):
            r.predict()
    with pytest.raises(ValueError):
        LatentStateResult(torch.zeros(2, 3, 7), names, mu, sd, lat)
    # the start point: w at the finite latent entries of the batch, clamped to +-3, 0 where they are missing
    lat = InitialStatePrior(MEAN, SD, states=("I", "GE")).bind(B, torch.as_tensor(x0_base))
    w = lat.start().numpy()
    want = np.clip((x0_base[:, [1, 4]] - np.array(MEAN)[[1, 4]]) / np.array(SD)[[1, 4]], -3, 3)
    want[1, 1] = 0.0
    np.testing.assert_allclose(w, want, rtol=1e-14)
    far = x0_base.copy()
    far[0, 1], far[1, 4] = 1e4, 0.5
    assert float(InitialStatePrior(MEAN, SD, states=("I",)).bind(B, torch.as_tensor(far)).start()[0, 0]) == 3.0


def test_new_symbols_are_declared_listed_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hode.h")).read()
    assert "Initial-state model" in hdr
    declared = set(re.findall(r"\b(hode_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(hode.lib_path())
    for name in ("hode_x0_params_f32", "hode_x0_params_f64", "hode_x0_grad_f32", "hode_x0_grad_f64"):
        assert name in declared and name in hode.capi.SYMBOLS and hasattr(lib, name), name
    assert callable(hode.capi.x0_params) and callable(hode.capi.x0_grad)
    import inference
    assert inference.InitialStatePrior is not None and "InitialStatePrior" in inference.__all__ and "LatentStateResult" in inference.__all__


def test_return_codes_without_a_launch():
    """HODE_EINVAL, checked on the host, nothing launched: A, B or n_lat < 1, popcount(lat_mask) != n_lat, K != popcount(ode_mask),
    ld < off + B n_lat, a bad link, off < K with the constants block, and NULL required pointers."""
    lib = hode.load()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    u = ctypes.c_uint32

    def params(A=2, B=3, n_lat=2, ld=13, off=7, lat_mask=0b10010, link=0, K=7, ode_mask=0x7f, coords=one, m=one, s=one, x0_base=one,
               x0_out=one, mu=one, sd=one, ode_base=one, ode_p=one, f=lib.hode_x0_params_f32):
        return f(z, A, B, n_lat, ld, off, coords, u(lat_mask), link, m, s, x0_base, x0_out, K, u(ode_mask), mu, sd, ode_base, ode_p)

    def grad(A=2, B=3, n_lat=2, ld=13, off=7, lat_mask=0b10010, link=0, K=7, ode_mask=0x7f, coords=one, m=one, s=one, gx0=one, sd=one,
             gode=one, glik=one, f=lib.hode_x0_grad_f64):
        return f(z, A, B, n_lat, ld, off, coords, u(lat_mask), link, m, s, gx0, K, u(ode_mask), sd, gode, glik)
    for f in (params, grad):
        for kw in (dict(A=0), dict(A=-1), dict(B=0), dict(n_lat=0), dict(n_lat=7, lat_mask=0x7f), dict(lat_mask=0b10), dict(lat_mask=0b111),
                   dict(lat_mask=0b1010000), dict(K=6), dict(K=8), dict(K=-1, ode_mask=0), dict(K=18, ode_mask=0x3ffff), dict(ld=12),
                   dict(off=-1), dict(off=6), dict(link=2), dict(link=-1), dict(coords=z), dict(m=z), dict(s=z), dict(sd=z)):
            assert f(**kw) == -1, (f.__name__, kw)
    for kw in (dict(x0_base=z), dict(x0_out=z), dict(mu=z), dict(ode_base=z)):
        assert params(**kw) == -1, kw
    for kw in (dict(gx0=z), dict(glik=z)):
        assert grad(**kw) == -1, kw
    for f in (lib.hode_x0_params_f32, lib.hode_x0_params_f64):
        assert params(A=0, f=f) == -1 and params(K=6, f=f) == -1
    for f in (lib.hode_x0_grad_f32, lib.hode_x0_grad_f64):
        assert grad(B=0, f=f) == -1 and grad(lat_mask=0b1, f=f) == -1
