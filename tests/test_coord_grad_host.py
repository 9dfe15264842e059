"""CPU side of the coordinate gradient (cbgx_unitransformer_backward_ex / cbgx_h2x_stack_backward_ex, gate_bwd_dx_mfma_kernel):
  * a lane-level model of what the kernel's DX variant adds to the gate backward -- the product V = R' W1^T on the layouts of the forward
    product, the sum over the units in the D layout of dpre, the hand-back of dL/dd to the edge's own lane and the node / neighbour
    coordinate terms -- against torch.autograd through the gate MLP;
  * the C ABI of the two new entry points (exported by both libraries, argument errors returned without touching a device);
  * the oracle's coordinate gradient against the reference's own UniTransformer autograd (when the reference tree is present), so that
    the yardstick of tests/test_gpu_coord_grad.py is pinned to the reference and not only to the oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cbgbench_amd import _native
from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH
from oracle import unitransformer as OU
from tests.lanesim import C_, MU, Q_, mfma

G, GH = 20, 160
F32 = np.float32


def row16_sum(v):
    return v.reshape(4, 16).sum(1, keepdims=True).repeat(16, 1).reshape(64)


def simulate_tile_dx(xi, xnb, valid, dew16, W1, b1, gam, bet, w2, b2):
    """one tile of gate_bwd_dx_mfma_kernel: node i at xi [3], its 16 slots' neighbours xnb [16,3] (invalid slots: nb = i), upstream
    dew16 [16] (0 on invalid slots).  Returns (dx_i [3], dx_nb [16,3]) -- the atomics of the tile."""
    f = F32
    xnb = np.where(valid[:, None], xnb, xi[None])
    d16 = np.sqrt(((xi[None] - xnb) ** 2).sum(1)).astype(f)
    dist = d16[C_]                                    # lane (j, *) holds slot j
    dew = dew16[C_].astype(f)
    y = [np.zeros((4, 64), f) for _ in range(10)]
    for s in range(5):
        ra = np.exp(-0.5 * (dist - MU[4 * s + Q_]) ** 2).astype(f)
        for nt in range(10):
            y[nt] = mfma(ra, W1[16 * nt + C_, 4 * s + Q_], y[nt])
    ssum = np.zeros((4, 64), f)
    for nt in range(10):
        y[nt] = y[nt] + b1[16 * nt + C_][None]
        ssum += y[nt]
    mean = np.stack([row16_sum(ssum[r]) for r in range(4)]) / GH
    var = np.zeros((4, 64), f)
    for nt in range(10):
        y[nt] = y[nt] - mean
        var += y[nt] ** 2
    rstd = 1.0 / np.sqrt(np.stack([row16_sum(var[r]) for r in range(4)]) / GH + 1e-5)
    acc = np.zeros((4, 64), f)
    for nt in range(10):
        y[nt] = y[nt] * rstd
        acc += w2[16 * nt + C_][None] * np.maximum(y[nt] * gam[16 * nt + C_][None] + bet[16 * nt + C_][None], 0)
    dacc = np.zeros((4, 64), f)
    for r in range(4):
        ew = 1.0 / (1.0 + np.exp(-(row16_sum(acc[r]) + b2)))
        dacc[r] = dew[4 * Q_ + r] * ew * (1 - ew)
    s1 = np.zeros((4, 64), f); s2 = np.zeros((4, 64), f)
    for nt in range(10):
        ga, be, ww = gam[16 * nt + C_][None], bet[16 * nt + C_][None], w2[16 * nt + C_][None]
        ya = y[nt] * ga + be
        dn = np.where(ya > 0, dacc * ww, 0) * ga
        s1 += dn
        s2 += dn * y[nt]
    s1 = np.stack([row16_sum(s1[r]) for r in range(4)]) / GH
    s2 = np.stack([row16_sum(s2[r]) for r in range(4)]) / GH
    # ---- the DX part: rd[s] = A operand of V = R' W1^T (edge j, g = 4 s + q); V in the D layout of dpre
    rd = [(-(dist - MU[4 * s + Q_]) * np.exp(-0.5 * (dist - MU[4 * s + Q_]) ** 2)).astype(f) for s in range(5)]
    ddp = np.zeros((4, 64), f)
    for nt in range(10):
        ga, be, ww = gam[16 * nt + C_][None], bet[16 * nt + C_][None], w2[16 * nt + C_][None]
        dn = np.where(y[nt] * ga + be > 0, dacc * ww * ga, 0)
        dp = rstd * (dn - s1 - y[nt] * s2)
        v = np.zeros((4, 64), f)
        for s in range(5):
            v = mfma(rd[s], W1[16 * nt + C_, 4 * s + Q_], v)
        ddp += dp * v
    # dL/dd of edge 4 q + r in row q; lane (j, *) takes __shfl(row16_sum(ddp[r]), 16 (j >> 2)) at r = j & 3
    red = np.stack([row16_sum(ddp[r]) for r in range(4)])
    dd = np.stack([red[r][16 * (C_ >> 2)] for r in range(4)])
    ddj = dd[C_ & 3, L64]
    inv = np.where(dist > 0, ddj / np.where(dist > 0, dist, 1), 0)
    c = np.stack([(xi[k] - xnb[C_, k]) * inv for k in range(3)])      # [3][64]
    dxi = np.array([row16_sum(c[k])[0] for k in range(3)])            # lane 0's atomics
    dxnb = np.zeros((16, 3), f)
    for lane in range(16):                                             # q == 0 lanes, valid slots only
        if valid[lane]:
            dxnb[lane] = -c[:, lane]
    return dxi, dxnb


L64 = np.arange(64)


def test_gate_dx_tile_matches_autograd():
    g = torch.Generator().manual_seed(1)
    W1 = torch.randn(GH, G, generator=g) * 0.4
    b1 = torch.randn(GH, generator=g) * 0.2
    gam = 1 + 0.3 * torch.randn(GH, generator=g)
    bet = 0.2 * torch.randn(GH, generator=g)
    w2 = torch.randn(GH, generator=g) * 0.3
    b2 = 0.1
    xi = (torch.randn(3, generator=g) * 2).double().requires_grad_(True)
    xnb = (torch.randn(16, 3, generator=g) * 3).double()
    xnb[5] = xi.detach()                 # a valid neighbour at distance 0: contributes nothing (the edge backwards' convention)
    xnb = xnb.requires_grad_(True)
    valid = np.ones(16, bool)
    valid[[3, 11, 15]] = False           # padded slots
    dew = torch.randn(16, generator=g).double()
    dew[torch.from_numpy(~valid)] = 0.0
    # autograd through the reference's gate: dist -> GaussianSmearing -> Linear -> LayerNorm -> ReLU -> Linear -> sigmoid
    rel = xi[None] - xnb
    d = torch.sqrt((rel ** 2).sum(1).clamp(min=1e-30))
    dsafe = torch.where(torch.from_numpy(valid) & (d > 1e-12), d, d.detach())
    r = OU.gaussian_smearing(dsafe[:, None], torch.float64)
    y = r @ W1.double().t() + b1.double()
    n = torch.nn.functional.layer_norm(y, (GH,), gam.double(), bet.double(), 1e-5)
    ew = torch.sigmoid(torch.relu(n) @ w2.double() + b2)
    (ew * dew).sum().backward()
    dxi, dxnb = simulate_tile_dx(xi.detach().numpy().astype(F32), xnb.detach().numpy().astype(F32), valid, dew.numpy().astype(F32),
                                 W1.numpy(), b1.numpy(), gam.numpy(), bet.numpy(), w2.numpy(), b2)
    ref_i, ref_nb = xi.grad.numpy(), xnb.grad.numpy()
    scale = max(np.abs(ref_i).max(), np.abs(ref_nb).max())
    assert scale > 1e-3
    assert np.abs(dxi - ref_i).max() <= 1e-4 * scale, (dxi, ref_i)
    assert np.abs(dxnb - ref_nb).max() <= 1e-4 * scale, np.abs(dxnb - ref_nb).max()
    assert not dxnb[~valid].any() and not dxnb[5].any()


def test_gate_derivative_convention_matches_oracle_smearing():
    """the kernel's rbf and its derivative (expf(-0.5 t^2), -t expf(-0.5 t^2), t = d - mu) are the oracle's GaussianSmearing and its
    autograd derivative"""
    d = torch.linspace(0.0, 12.0, 97, dtype=torch.float64).requires_grad_(True)
    r = OU.gaussian_smearing(d[:, None], torch.float64)
    t = d.detach()[:, None] - torch.from_numpy(MU).double()[None]
    assert torch.allclose(r.detach(), torch.exp(-0.5 * t * t), rtol=1e-12, atol=0)
    for gi in (0, 7, 19):
        (gd,) = torch.autograd.grad(r[:, gi].sum(), d, retain_graph=True)
        assert torch.allclose(gd, -t[:, gi] * torch.exp(-0.5 * t[:, gi] ** 2), rtol=1e-10, atol=1e-14)


# ---- C ABI ------------------------------------------------------------------------------------------
EX = ("cbgx_unitransformer_backward_ex", "cbgx_h2x_stack_backward_ex")


def test_ex_entries_are_declared_and_exported_by_both_libraries():
    import subprocess
    hdr = open(os.path.join(os.path.dirname(LIBPATH), "..", "..", "include", "cbgx.h")).read()
    for name in EX:
        assert name + "(" in hdr and name in _native.EXPORTS
        for path in (LIBPATH, XCHECK_LIBPATH):
            sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
            assert f" {name}\n" in sym, (path, name)


@pytest.mark.parametrize("path", [LIBPATH, XCHECK_LIBPATH], ids=["product", "xcheck"])
def test_ex_argument_errors_without_a_device(path):
    """NULL pointers and a wrong gradient count come back as CBGX_E_INVALID before anything is launched"""
    lib = _native._load(path) if path != LIBPATH else _native.lib()
    E_INVALID = -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    grads = (ctypes.c_void_p * 4)(p, p, p, p)
    n, L, C = 10, 9, 13
    # denoiser: NULL packed / tape / flags / workspace
    rc = lib.cbgx_unitransformer_backward_ex(None, L, C, None, 0, None, None, n, None, None, None, grads, 4, None, p, None, 0, None)
    assert rc == E_INVALID, rc
    # ... and 4 gradient tensors where 6 + 36 L + 4 are expected
    rc = lib.cbgx_unitransformer_backward_ex(p, L, C, p, 64, p, p, n, None, None, None, grads, 4, None, p, p, 64, None)
    assert rc == E_INVALID and b"gradient tensors" in lib.cbgx_last_error(), (rc, lib.cbgx_last_error())
    # the H2X stack: NULL pointers, then 4 gradient tensors where 6 + 18 L are expected
    rc = lib.cbgx_h2x_stack_backward_ex(None, 3, None, 0, None, None, None, n, None, grads, 4, None, p, None, 0, None)
    assert rc == E_INVALID, rc
    rc = lib.cbgx_h2x_stack_backward_ex(p, 3, p, 64, p, p, p, n, p, grads, 4, p, p, p, 64, None)
    assert rc == E_INVALID and b"gradient tensors" in lib.cbgx_last_error(), (rc, lib.cbgx_last_error())


# ---- the yardstick against the reference ---------------------------------------------------------
def _reference_root():
    from oracle import ref_shim
    return ref_shim.REFERENCE_ROOT


needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(_reference_root(), "repo")), reason="needs the reference tree")


@needs_reference
@pytest.mark.parametrize("case", ["denoiser_2graphs", "denoiser_linker"])
def test_oracle_coordinate_gradient_equals_reference_autograd(golden_dir, case):
    """x.grad (and h.grad) of a random-weighted score of the reference's own UniTransformer (unmodified, through oracle/ref_shim.py)
    equal the oracle's, in float64"""
    from oracle import ref_shim
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref_model = ref_shim.build_reference_targetdiff(13, num_layers=2, seed=3).double()
    den = ref_model.denoiser
    sd = {"denoiser." + k: v for k, v in den.state_dict().items()}
    z = np.load(os.path.join(golden_dir, case + ".npz"))
    g = {k: torch.from_numpy(z[k]) for k in ("x", "h", "batch_idx", "lig_flag", "gen_flag")}
    gen = torch.Generator().manual_seed(4)
    N = g["x"].shape[0]
    wx, wh, wl = (torch.randn(N, 3, generator=gen).double(), 0.1 * torch.randn(N, 128, generator=gen).double(),
                  torch.randn(N, 13, generator=gen).double())
    grads = []
    for run in ("reference", "oracle"):
        x = g["x"].double().clone().requires_grad_(True)
        h = g["h"].double().clone().requires_grad_(True)
        if run == "reference":
            xo, ho, lo = den(x, h, g["batch_idx"], g["lig_flag"], g["gen_flag"])
        else:
            xo, ho, lo = OU.unitransformer_forward(sd, x, h, g["batch_idx"], g["lig_flag"], g["gen_flag"])
        ((xo * wx).sum() + (ho * wh).sum() + (lo * wl).sum()).backward()
        grads.append((x.grad, h.grad))
    (rx, rh), (ox, oh) = grads
    assert float(rx[~g["lig_flag"]].norm()) > 0          # protein rows have a coordinate gradient too
    assert float((ox - rx).norm()) <= 1e-9 * float(rx.norm()), float((ox - rx).norm() / rx.norm())
    assert float((oh - rh).norm()) <= 1e-9 * float(rh.norm())
