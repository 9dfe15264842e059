"""The split-f16 x2h edge kernel (edge_x2h_f16.hip: scores and aggregation on the f16 matrix pipe) against the CPU oracle in fp32 and
fp64, through the C ABI: `stages.x2h_attention` runs one x2h block the way a layer of the forward does (node stage, (general,
protein-only) list pair, launch_edge_x2h_dual), which picks the split-f16 kernel unless CBGX_X2H_F16=0.

Yardstick: `assert_fp32_grade` of tests/test_gpu_range.py -- the error stays within 8 x the fp32 oracle's own error against fp64 plus
2e-6 of the magnitude, and inside 1e-4 of the magnitude."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cbgbench_amd import stages
from cbgbench_amd.unitransformer import graph_ptr_from_batch
from oracle import unitransformer as OU
from tests.test_gpu_range import DEV, block_gpu, block_reference, load, model_with, scaled_sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_fp32_grade(got, ref32, ref64, what, fp32_relative_only=False):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    scale = float(ref64.abs().max())
    e_gpu = float((got.double() - ref64).abs().max())
    e_cpu = float((ref32.double() - ref64).abs().max())
    print(f"{what}: magnitude {scale:.3g}, libcbgx err {e_gpu:.3e}, fp32 oracle err {e_cpu:.3e}")
    assert e_gpu <= 8 * e_cpu + 2e-6 * scale, f"{what}: |err| {e_gpu:.3e}, the fp32 oracle's own {e_cpu:.3e} (magnitude {scale:.3e})"
    if not fp32_relative_only:
        assert e_gpu <= max(1e-4 * scale, 4 * e_cpu), f"{what}: |err| {e_gpu:.3e} vs magnitude {scale:.3e}"


def check_x2h(got, r32, r64, h, what):
    """the output h' = h + update, and the update itself (the residual would hide a small update's error behind |h|)"""
    assert_fp32_grade(got, r32, r64, what)
    assert_fp32_grade(got - h, r32 - h, r64 - h.double(), what + " (update)", fp32_relative_only=True)


def run_case(golden_dir, sd, case, h_of, what):
    g = load(golden_dir, case)
    h = h_of(g["h"])
    got = block_gpu(model_with(sd), g, h, "x2h")
    check_x2h(got, block_reference(sd, g, h, "x2h", torch.float32), block_reference(sd, g, h, "x2h", torch.float64), h, what)


# ---- 1. plain parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["denoiser_2graphs", "denoiser_linker"])
def test_block_parity(golden_dir, synthetic_sd, case):
    run_case(golden_dir, synthetic_sd, case, lambda h: h, f"x2h {case}")


# ---- 2. range, block level (the grid of tests/test_gpu_range.py, and the LayerNorm affine alone: the case that moves kh) ------------
@pytest.mark.parametrize("wscale", [1e-3, 1e-2, 1.0, 30.0])
def test_block_with_all_tensors_scaled(golden_dir, synthetic_sd, wscale):
    run_case(golden_dir, scaled_sd(synthetic_sd, lambda k: wscale), "denoiser_2graphs", lambda h: h, f"x2h weights x {wscale:g}")


@pytest.mark.parametrize("seed", [0, 1])
def test_block_with_mixed_scales_per_tensor(golden_dir, synthetic_sd, seed):
    import zlib
    choices = (1e-3, 1e-2, 0.1, 1.0, 10.0, 30.0)
    rule = lambda k: choices[(zlib.crc32(k.encode()) + seed) % len(choices)]
    run_case(golden_dir, scaled_sd(synthetic_sd, rule), "denoiser_linker", lambda h: h, f"x2h mixed scales #{seed}")


@pytest.mark.parametrize("hscale", [1e-3, 1e2, 1e4, 3e5])
def test_block_with_large_and_small_features(golden_dir, synthetic_sd, hscale):
    def h_of(h0):
        h = (h0 * hscale).clone()
        h[3] = h[3] / hscale          # one row at its original magnitude
        h[5] = 0.0                    # one zero row
        return h
    run_case(golden_dir, synthetic_sd, "denoiser_2graphs", h_of, f"x2h features x {hscale:g}")


@pytest.mark.parametrize("ascale", [1e-3, 30.0])
def test_block_with_layernorm_affine_scaled(golden_dir, synthetic_sd, ascale):
    """only gamma and beta of the MLPs' LayerNorms: the hidden activations' bound, and with it kh, moves by the factor"""
    sd = scaled_sd(synthetic_sd, lambda k: ascale if ".net.1." in k else 1.0)
    assert any(".net.1." in k and ".x2h_layers." in k for k in sd)
    run_case(golden_dir, sd, "denoiser_2graphs", lambda h: h, f"x2h LayerNorm affine x {ascale:g}")


# ---- 3. whole denoiser -------------------------------------------------------------------------------------------------------------
def denoiser_outputs(m, g):
    with torch.no_grad():
        return [t.cpu() for t in m.denoiser(x=g["x"].to(DEV), h=g["h"].to(DEV), batch_idx=g["batch_idx"].to(DEV),
                                            lig_flag=g["lig_flag"].to(DEV), gen_flag=g["gen_flag"].to(DEV))]


@pytest.fixture(scope="module")
def denoiser_case(golden_dir, synthetic_sd):
    g = load(golden_dir, "denoiser_2graphs")
    ref = {dt: OU.unitransformer_forward(synthetic_sd, g["x"].to(dt), g["h"].to(dt), g["batch_idx"], g["lig_flag"], g["gen_flag"])
           for dt in (torch.float32, torch.float64)}
    return g, ref


def test_whole_denoiser(denoiser_case, synthetic_sd):
    g, ref = denoiser_case
    out = denoiser_outputs(model_with(synthetic_sd), g)
    for name, got, k in (("x_out", out[0], 0), ("h_out", out[1], 1), ("logits", out[2], 2)):
        assert_fp32_grade(got, ref[torch.float32][k], ref[torch.float64][k], f"denoiser {name}")
    lig = g["lig_flag"]
    assert torch.equal(out[2][lig].argmax(-1), ref[torch.float64][2][lig].argmax(-1))


# ---- 4. the smallest shapes at which the kernel can go wrong -----------------------------------------------------------------------
def small_batch():
    """graphs of 1 node (degree 0), 12 (degree 11: invalid slots in both halves), 20 (half 1 partly empty), 33 (all 32 slots) and one
    of 40 whose 18 ligand atoms sit in a tight cluster far from the protein atoms: their first 16 slots hold ligand atoms only"""
    gen = torch.Generator().manual_seed(7)
    xs, ligs, batch = [], [], []
    for b, n in enumerate((1, 12, 20, 33)):
        xs.append(torch.randn(n, 3, generator=gen) * 2.5 + 40.0 * b)
        lig = torch.zeros(n, dtype=torch.bool)
        if n > 1:
            lig[-3:] = True
        ligs.append(lig)
        batch += [b] * n
    centre = torch.tensor([200.0, 0.0, 0.0])
    x_lig = centre + torch.randn(18, 3, generator=gen) * 0.6
    d = torch.randn(22, 3, generator=gen)
    x_prot = centre + d / d.norm(dim=1, keepdim=True) * (8.0 + 2.0 * torch.rand(22, 1, generator=gen))
    xs += [x_prot, x_lig]
    ligs += [torch.zeros(22, dtype=torch.bool), torch.ones(18, dtype=torch.bool)]
    batch += [4] * 40
    x, lig = torch.cat(xs), torch.cat(ligs)
    h = torch.randn(x.shape[0], 128, generator=gen)
    return x, h, lig, torch.tensor(batch)


def test_smallest_shapes(synthetic_sd):
    x, h, lig, batch = small_batch()
    m = model_with(synthetic_sd)
    packed = m.denoiser.packed_weights(torch.device(DEV))
    xd = x.to(DEV)
    nbr, deg = stages.knn_graph(xd, graph_ptr_from_batch(batch.to(DEV)))
    assert deg.cpu().tolist() == [0] + [11] * 12 + [19] * 20 + [32] * 73
    first16 = nbr[-18:, :16].cpu().long()
    assert bool(lig[first16].all()) and not bool(lig[nbr[-18:, 16:].cpu().long()].all())      # the clustered ligand atoms
    e_w = stages.edge_gate(packed, xd, nbr, deg)
    got = stages.x2h_attention(packed, 0, xd, h.to(DEV), nbr, deg, lig.to(DEV).to(torch.uint8), e_w).cpu()
    ei = stages.edge_index_from_nbr(nbr, deg).cpu()
    mask = torch.arange(32)[None, :] < deg.cpu()[:, None]
    ew_edges = e_w.cpu()[mask][:, None]
    et = OU.build_edge_type(ei, lig)
    ref = {}
    for dt in (torch.float32, torch.float64):
        sdd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in synthetic_sd.items() if k.startswith("denoiser")}
        ref[dt] = OU.x2h_attention(sdd, "denoiser.blocks.0.x2h_layers.0", x.to(dt), h.to(dt), et, ei, ew_edges.to(dt))
    check_x2h(got, ref[torch.float32], ref[torch.float64], h, "x2h smallest shapes")
    assert torch.equal(got[0], h[0])          # degree 0: no edge, no update


# ---- 5. the knob ---------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r})
from tests.test_gpu_range import load, model_with
from tests.test_gpu_x2h_f16 import denoiser_outputs
from oracle import weights
g = load({golden!r}, "denoiser_2graphs")
m = model_with(weights.synthetic_state_dict(13, 9, seed=0))
a, b = denoiser_outputs(m, g), denoiser_outputs(m, g)
np.savez({out!r}, **{{f"a{{k}}": t.numpy() for k, t in enumerate(a)}}, **{{f"b{{k}}": t.numpy() for k, t in enumerate(b)}})
"""


def test_knob_selects_the_kernel_per_process(denoiser_case, synthetic_sd, golden_dir, tmp_path):
    """CBGX_X2H_F16=0 in a fresh process runs the exact-fp32 kernel: its outputs and this process's differ by less than the yardstick,
    and each is the same in two calls.  (Run under CBGX_X2H_F16=0 the roles swap: the child then gets the split-f16 kernel.)"""
    g, ref = denoiser_case
    m = model_with(synthetic_sd)
    here = [denoiser_outputs(m, g), denoiser_outputs(m, g)]
    other = "1" if os.environ.get("CBGX_X2H_F16") == "0" else "0"
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, CBGX_X2H_F16=other)
    subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, golden=golden_dir, out=out)], check=True, env=env, cwd=ROOT, timeout=300)
    z = np.load(out)
    for k, name in enumerate(("x_out", "h_out", "logits")):
        assert torch.equal(here[0][k], here[1][k]), f"{name}: two calls of this process differ"
        assert np.array_equal(z[f"a{k}"], z[f"b{k}"]), f"{name}: two calls of the child process differ"
        there = torch.from_numpy(z[f"a{k}"])
        r32, r64 = ref[torch.float32][k], ref[torch.float64][k]
        assert_fp32_grade(here[0][k], r32, r64, f"{name}, this process")
        assert_fp32_grade(there, r32, r64, f"{name}, CBGX_X2H_F16={other}")
        scale, e_cpu = float(r64.abs().max()), float((r32.double() - r64).abs().max())
        diff = float((here[0][k] - there).abs().max())
        print(f"{name}: knob on vs off max |diff| {diff:.3e}")
        assert diff <= 8 * e_cpu + 2e-6 * scale, f"{name}: the two kernels differ by {diff:.3e}"
