"""The forward kernels' hybrid hidden layer (mlp_hidden_blk_lds, csrc/hode_mlp.h: the last K rotations of a layer fetched through
LDS) as hipcc compiles it for gfx950 -- no GPU: csrc/hode_solve_fwd.hip goes to assembly, device code only.

Checks of the code that was written, nothing else: the registers, scratch, occupancy and LDS of the instantiations, and in the
accepted-step block of the benchmark kernel the number of DPP rotation moves and LDS fetches that the shipped K of that
instantiation means (18 hidden layers per DP5(4) step: 6 stages x 3 matrices)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "hybrid-ode-for-glp-1-and-glucose_amd", "csrc", "hode_solve_fwd.hip")
KERNEL = "_ZN4hode16solve_fwd_kernelIfLi{NL}ELi{M}ELi{LB}ELb{TAPE}ELb{GD}ELb{MULTI}ELb1EEEvNS_9SolveArgsIT_EEi"
BENCH = KERNEL.format(NL=4, M=0, LB=2, TAPE=0, GD=0, MULTI=0)          # solve_fwd_kernel<float, 4, DP54, 2, false, false, false, true>
TAPING = KERNEL.format(NL=4, M=0, LB=2, TAPE=1, GD=0, MULTI=0)
LDS_BASE, LDS_ROT = 2368, 768                                          # rows + cvec + ybuf | 4 rows x 48 dwords
# shipped K per instantiation (FwdRot, csrc/hode_solve_fwd.hip): the benchmark kernel takes the lean K = 8, the taping one keeps K = 0
SHIPPED_K = {BENCH: 8, TAPING: 0}
# scratch bytes per lane of the fp32 instantiations with three hidden matrices BEFORE the hybrid layer: none may exceed its figure
# (method, tape, gd, multi) -> bytes
SCRATCH_BEFORE = {(0, 1, 1, 0): 36, (0, 1, 0, 0): 0, (0, 0, 1, 0): 16, (0, 0, 0, 1): 12, (0, 0, 0, 0): 0,
                  (1, 1, 1, 0): 8, (1, 1, 0, 0): 0, (1, 0, 1, 0): 0, (1, 0, 0, 0): 0}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path_factory.mktemp("fwd_lds_rot") / "fwd.s"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "--cuda-device-only", "-S", "-Wno-unused-function",
                        SRC, "-o", str(out), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    res = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name: |\Z)", r.stderr, re.S):
        f = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))  # noqa: E731
        res[name] = dict(vgprs=f("VGPRs"), scratch=f("ScratchSize [bytes/lane]"), occupancy=f("Occupancy [waves/SIMD]"), lds=f("LDS Size [bytes/block]"))
    return res, out.read_text()


def step_block(asm, kernel):
    """The accepted-step block: the straight-line block of the kernel with the most packed FMAs (the six unrolled stages)."""
    body = re.search(rf"^{re.escape(kernel)}:[^\n]*\n(.*?)\n\s*s_endpgm", asm, re.S | re.M).group(1)
    return max(re.split(r"^\.LBB\d+_\d+:.*$", body, flags=re.M), key=lambda b: b.count("v_pk_fma_f32"))


@pytest.mark.parametrize("kernel", [BENCH, TAPING], ids=["benchmark", "taping"])
def test_registers_scratch_occupancy_and_lds(compiled, kernel):
    r = compiled[0][kernel]
    assert r["vgprs"] <= 256 and r["scratch"] == 0 and r["occupancy"] == 2, r
    assert r["lds"] == LDS_BASE + (LDS_ROT if SHIPPED_K[kernel] else 0), r


def test_no_three_matrix_instantiation_gained_scratch_or_lost_occupancy(compiled):
    for (m, tape, gd, multi), before in SCRATCH_BEFORE.items():
        r = compiled[0][KERNEL.format(NL=4, M=m, LB=2, TAPE=tape, GD=gd, MULTI=multi)]
        assert r["scratch"] <= before and r["occupancy"] == 2 and r["vgprs"] <= 256, ((m, tape, gd, multi), r)
    two = [r for k, r in compiled[0].items() if k.startswith("_ZN4hode16solve_fwd_kernelIfLi3E")]
    assert len(two) == 9 and all(r["scratch"] == 0 and r["occupancy"] == 2 and r["lds"] == LDS_BASE + LDS_ROT for r in two), two


def test_step_block_of_the_benchmark_kernel_has_the_moves_and_fetches_of_its_k(compiled):
    K = SHIPPED_K[BENCH]
    blk = step_block(compiled[1], BENCH)
    assert blk.count("v_permlane32_swap_b32 v4, v5") == 18                         # one finish per hidden layer
    assert len(re.findall(r"v_mov_b32_dpp v8, v10 row_ror:\d+", blk)) == 18 * (15 - K)
    # K / 2 two-rotation fetches per layer; the lean form issues the first of them as two ds_read_b32 into v9 and v11
    assert blk.count("ds_read2_b32") + len(re.findall(r"ds_read_b32 v9,", blk)) == 18 * K // 2
    assert len(re.findall(r"ds_read_b32 v9,", blk)) == len(re.findall(r"ds_read_b32 v11,", blk)) == 18
    assert blk.count("ds_write2_b32") == 18 and blk.count("v_pk_fma_f32") == 18 * 30 and "scratch_" not in blk


def test_taping_kernel_keeps_the_dpp_layer(compiled):
    body = re.search(rf"^{re.escape(TAPING)}:[^\n]*\n(.*?)\n\s*s_endpgm", compiled[1], re.S | re.M).group(1)
    layers = body.count("v_permlane32_swap_b32 v4, v5")
    assert layers >= 18 and len(re.findall(r"v_mov_b32_dpp v8, v10 row_ror:\d+", body)) == 15 * layers          # K = 0
    assert "ds_read2_b32" not in body and "ds_write2_b32" not in body
