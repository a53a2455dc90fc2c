"""bench.py as the driver launches it for N > 1 -- `python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2`
-- rehearsed on ONE GPU with the gloo backend (the RCCL path differs only by the backend name: the same all_reduce call on
a device tensor instead of a host-staged one).  Checks the JSON contract of the line rank 0 prints, the collective the
training leg reports, and that the 2-rank step IS the single-process step on the union of the two shards."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_two_ranks_gloo_on_one_gpu_matches_single_process_step():
    import bench
    import hode
    B = 256
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--patients-per-gpu", str(B), "--train-steps", "2", "--full"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline"):
        assert key in out, key
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["unit"] == "patient-trajectories/s" and out["dtype"] == "f32" and out["vs_baseline"] is None
    assert out["config"]["patients_per_gpu"] == B and "workload" in out["config"]
    assert abs(out["value"] - 2 * B * 2 / (out["ms_per_step"] * 2e-3)) < 1e-6 * out["value"]      # whole-job aggregate over both ranks
    assert out["roofline"]["bound"] == "valu_fp32" and 0 < out["roofline"]["frac"] < 1
    assert "cpu_baseline" not in out and "vi_step" not in out      # rank-0-at-N=1 legs only
    tr = out["train_step"]
    assert tr["collective"].startswith("1 x all_reduce(sum) of 13 529 fp64")
    # the same step in ONE process on the union of the two shards: first-step loss of the 2-rank run == global mean loss
    dev = torch.device("cuda")
    nn_t, ode = bench.synth_weights(0).to(dev), bench.ODE_DEFAULT.to(dev)
    tot, n = 0.0, 0
    for rank in range(2):
        x0, t, meal, tv = (v.to(dev) for v in bench.synth_cohort(B, 1000 + rank))
        obs, student = bench.train_problem(dev, x0, t, meal, tv, ode, nn_t, rank)
        ls, _, _, _ = hode.train.hip_loss_and_grads(student, ode, x0, t, meal, tv, obs, 64, 4, 2 * B * 241 * 6)
        tot += float(ls)
        n += B * 241 * 6
    assert abs(tr["loss_first_last"][0] - tot / n) < 1e-6 * (tot / n)
    assert np.isfinite(tr["value"]) and tr["value"] > 0


def test_bench_two_ranks_uneven_shards_is_the_single_process_step_on_the_whole_cohort():
    """`--total-patients 37` over two ranks = shards of 19 and 18 (hode.train.shard_bounds) through bench.py's own path: the
    global-mean scaling, the fp64 message and the whole-job value must not assume equal shards."""
    import bench
    import hode
    N = 37
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--total-patients", str(N), "--train-steps", "2", "--no-zscore", "--full"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["config"]["patients_total"] == N and out["config"]["patients_per_gpu"] == N / 2 and "zscore_regime" not in out
    assert abs(out["value"] - N * 2 / (out["ms_per_step"] * 2e-3)) < 1e-6 * out["value"]
    dev = torch.device("cuda")
    nn_t, ode = bench.synth_weights(0).to(dev), bench.ODE_DEFAULT.to(dev)
    x0, t, meal, tv = (v.to(dev) for v in bench.synth_cohort(N, 1000))
    tot = 0.0
    for rank in range(2):
        lo, hi = hode.train.shard_bounds(N, rank, 2)
        assert hi - lo == (19 if rank == 0 else 18)
        obs, student = bench.train_problem(dev, x0[lo:hi].contiguous(), t, meal[lo:hi].contiguous(), tv[lo:hi].contiguous(), ode, nn_t, rank)
        ls, _, _, _ = hode.train.hip_loss_and_grads(student, ode, x0[lo:hi].contiguous(), t, meal[lo:hi].contiguous(), tv[lo:hi].contiguous(),
                                                    obs, 64, 4, N * 241 * 6)
        tot += float(ls)
    first = out["train_step"]["loss_first_last"][0]
    assert abs(first - tot / (N * 241 * 6)) < 1e-6 * first


def test_rccl_backend_one_rank_runs_the_data_parallel_step_and_the_sharded_elbo(tmp_path):
    """The RCCL path itself ("nccl" backend: device-tensor all_reduce of the fp64 message, `elbo(group=...)`'s gradient
    collective) on the one GPU a test box has: a process group of ONE rank.  It cannot show scaling, but it executes
    `dist.init_process_group("nccl", device_id=...)`, the collectives on device buffers and the code around them exactly as an
    8-rank job does (that path had never run).  Results must be the bits of the same step without a group.
    Round 4 adds the data side's exchange: GlucoseDataset(group=...)'s all-gather of the window moments (13 doubles per rank)."""
    code = f"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd")!r})
import bench, hode, models
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
x0, t, meal, tv = (v.to(dev) for v in bench.synth_cohort(64, 3))
nn_t, ode = bench.synth_weights(0).to(dev), bench.ODE_DEFAULT.to(dev)
obs, student = bench.train_problem(dev, x0, t, meal, tv, ode, nn_t, 0)
def run(n_steps):
    state = hode.train.TrainState(student.clone())
    def compute(p):
        ls, gnn, gode, _ = hode.train.hip_loss_and_grads(p, ode, x0, t, meal, tv, obs, 64, 4, obs.numel(), state=state)
        return ls, gnn, gode, obs.numel()
    losses = [float(hode.train.train_step(state, compute)) for _ in range(n_steps)]
    return state.p.clone(), losses
p_plain, l_plain = run(2)
def vi():
    torch.manual_seed(0)
    m = models.HybridODENN(nn_hidden=16, nn_layers=2, use_variational=True, device=dev)
    with torch.no_grad():
        for n_, p_ in m.variational_params.means.items():
            if n_.startswith("ode_"): p_.copy_(getattr(m.ode_core, n_[4:]))
        for p_ in m.variational_params.log_stds.values(): p_.fill_(-6.0)
    return m
batch = {{"initial_state": x0[:8], "observations": obs[:8, :31].contiguous(), "time_points": t[:31].contiguous(),
         "external_inputs": {{"meal": meal[:8, :31].contiguous(), "tVNS": tv[:8, :31].contiguous()}}}}
m = vi(); torch.manual_seed(1); e0 = m.elbo(batch, n_samples=3, noise_sigma=1.0); e0.backward()
g0 = torch.cat([p_.grad.reshape(-1) for p_ in m.variational_params.means.values()]).clone()
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT={str(_free_port())!r}, RANK="0", WORLD_SIZE="1")
dist.init_process_group("nccl", device_id=dev)            # "nccl" IS RCCL on ROCm
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
p_grp, l_grp = run(2)
m = vi(); torch.manual_seed(1); e1 = m.elbo(batch, n_samples=3, noise_sigma=1.0, group=True); e1.backward()
g1 = torch.cat([p_.grad.reshape(-1) for p_ in m.variational_params.means.values()]).clone()
# the dataset's one exchange step (DESIGN 7): GlucoseDataset(group=...) all-gathers its shard's window moments over RCCL
import numpy as np, pandas as pd
from hode.datagen import GlucoseDataset
tb = np.load({os.path.join(ROOT, "tests", "golden", "g9_4gi_dataset_table.npz")!r}, allow_pickle=False)
csv = {str(tmp_path / "all.csv")!r}
pd.DataFrame(tb["table"], columns=list(tb["columns"])).to_csv(csv, index=False, float_format="%.17g")
d_plain = GlucoseDataset(csv, sequence_length=20, stride=10)
d_grp = GlucoseDataset(csv, sequence_length=20, stride=10, group=True)
assert np.array_equal(d_plain.state_mean, d_grp.state_mean) and np.array_equal(d_plain.state_std, d_grp.state_std)
ia = np.arange(len(d_plain))
assert torch.equal(d_plain.batch(ia)["observations"], d_grp.batch(ia)["observations"])
dist.barrier(); torch.cuda.synchronize(); dist.destroy_process_group()
assert torch.equal(p_plain, p_grp), float((p_plain - p_grp).abs().max())
assert max(abs(a - b) / abs(a) for a, b in zip(l_plain, l_grp)) < 1e-12
assert abs(float(e0) - float(e1)) < 1e-9 * abs(float(e0)) and float((g0 - g1).abs().max()) <= 1e-6 * float(g0.abs().max())
print("rccl one-rank ok")
"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "rccl one-rank ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """`bench.py --steps K --dump-outputs DIR` times K steps, reports ms_per_step, and writes what the timed forward solve
    returned for its synthetic cohort (seeded: the same inputs every run) -- checked against a solve of those inputs here."""
    import bench
    import hode
    B = 128
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--patients-per-gpu", str(B),
           "--no-cpu-baseline", "--no-train", "--no-vi", "--no-generic", "--no-data-side", "--no-sobol", "--no-class-path",
           "--no-zscore", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert sorted(os.listdir(out_dir)) == ["nfev.npy", "nsteps.npy", "status.npy", "y.npy"]
    dev = torch.device("cuda")
    x0, t, meal, tv = (v.to(dev) for v in bench.synth_cohort(B, 1000))
    sol = hode.solve_fwd(x0, t, meal, tv, None, bench.ODE_DEFAULT.to(dev), bench.synth_weights(0).to(dev), 64, 4, rtol=1e-6, atol=1e-8)
    y = np.load(out_dir / "y.npy")
    assert y.dtype == np.float32 and y.shape == (B, 241, 6)
    assert np.allclose(y, sol.y.cpu().numpy(), rtol=1e-6, atol=1e-7)
    assert np.array_equal(np.load(out_dir / "status.npy"), sol.status.cpu().numpy().astype(np.float64))
    assert np.array_equal(np.load(out_dir / "nsteps.npy"), sol.nsteps.cpu().numpy().astype(np.float64))


def test_bench_plain_run_prints_the_headline_alone():
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline line and nothing else -- no secondary leg, no
    CPU baseline -- with the same fields and arithmetic as a --full run's headline."""
    B = 128
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--patients-per-gpu", str(B)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert set(out) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                        "vs_baseline", "dtype", "data", "config", "roofline"}
    assert out["metric"] == "patient-trajectories/s (6-state, 240-step dopri5)" and out["unit"] == "patient-trajectories/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["steps"] == 2 and out["warmup"] == 1
    assert abs(out["value"] - B * 2 / (out["ms_per_step"] * 2e-3)) < 1e-6 * out["value"]
    assert out["config"]["trajectories_ok"] == B and 0 < out["roofline"]["frac"] < 1
