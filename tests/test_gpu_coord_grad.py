"""Gradients with respect to the input COORDINATES (cbgx_unitransformer_backward_ex / cbgx_h2x_stack_backward_ex and the autograd
bridges above them) against torch.autograd on the CPU oracle, which tests/test_coord_grad_host.py pins to the reference's own
UniTransformer.

With the reference, ``x.requires_grad_()`` + ``loss.backward()`` fills ``x.grad`` through the layer chain (every block's distance
features, h2x's rel_x) and through the distance gate e_w = sigmoid(MLP(rbf(|x_i - x_j|))) computed once from x.  Each check here is
a random-weighted score of the outputs the caller reads; the criterion is the suite's: ||g - g_ref||_2 <= 2e-4 ||g_ref||_2 for x.grad
and h.grad (1e-3 for the parameter tensors, as in tests/test_gpu_training.py), with the verified ReLU-flip exception of tests/relu_flip.py (ONE near-zero unit, flipped in the oracle, must explain every deviating
tensor)."""
import contextlib
import os

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import synthetic
from cbgbench_amd.unitransformer import UniTransformer
from oracle import diffbp as OB
from oracle import unitransformer as OU
from oracle import weights as W
from tests.relu_flip import relu_margins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
NUM_CLASSES = 13


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return {k: torch.from_numpy(z[k]) if z[k].ndim else z[k].item() for k in z.files}


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def failures(got, ref):
    """{name: message} of the tensors whose relative L2 error exceeds the tolerance: TOL for x / h, the suite's 1e-3 of the norm for
    parameter tensors (tests/test_gpu_training.py::oracle_failures); a tensor whose reference is ~0 must be ~0 too"""
    out = {}
    for k, b in ref.items():
        tol = TOL if k in ("x", "h") else 1e-3
        a = got[k]
        assert a is not None, f"{k}: no gradient"
        if float(b.double().norm()) < 1e-9:
            if float(a.detach().abs().max()) > 1e-6:
                out[k] = f"{k}: reference zero, got max {float(a.detach().abs().max()):.2e}"
            continue
        e = rel_err(a, b)
        if e > tol:
            out[k] = f"{k}: relative L2 error {e:.2e}"
    return out


def check(got, oracle_run):
    """got {name: tensor}; oracle_run(force) -> (near, ref {name: tensor}).  Plain comparison, or ONE verified ReLU flip."""
    near, ref = oracle_run(None)
    bad = failures(got, ref)
    if not bad:
        return ref
    # a flip moves the gradients of the MLP it sits in: the candidates are that MLP's units (any MLP's if only x / h deviate)
    mlps = {k.rsplit(".net.", 1)[0] for k in bad if ".net." in k}
    cands = [(p, ru) for p, lst in sorted(near.items()) if not mlps or any(p.endswith(m) for m in mlps) for ru in sorted(set(lst))]
    assert cands and len(cands) <= 24, (list(bad.values()), len(cands))
    for prefix, ru in cands:
        _, ref_f = oracle_run({prefix: [ru]})
        if not failures(got, ref_f):
            print(f"ReLU flip verified: {prefix} row {ru[0]} unit {ru[1]} explains {sorted(bad)}")
            return ref_f
    raise AssertionError(f"{list(bad.values())} (not explained by flipping any of the {len(cands)} near-zero units)")


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def gate_detached():
    """the oracle with the gate's coordinate path cut: what the backward gave before cbgx_unitransformer_backward_ex"""
    orig = OU.edge_gate
    OU.edge_gate = lambda *a, **k: orig(*a, **k).detach()
    try:
        yield
    finally:
        OU.edge_gate = orig


# ---- the denoiser ---------------------------------------------------------------------------------
def denoiser_sd(sd, num_layers=None):
    """the denoiser's own state dict (module keys), optionally truncated to its first `num_layers` blocks"""
    out = {}
    for k, v in sd.items():
        if not k.startswith("denoiser."):
            continue
        k = k[len("denoiser."):]
        if num_layers is not None and k.startswith("blocks.") and int(k.split(".")[1]) >= num_layers:
            continue
        out[k] = v
    return out


def make_denoiser(sd, num_layers=9):
    cfg = C.default_targetdiff_config(NUM_CLASSES)
    m = C.get_model(cfg)
    dcfg = dict(m.denoiser.cfg)
    dcfg["num_layers"] = num_layers
    den = UniTransformer(type(m.denoiser.cfg)(dcfg))
    den.load_state_dict(denoiser_sd(sd, num_layers), strict=True)
    return den.to(DEV)


def sources_rows(g):
    """A1 = gen | lig | in-neighbours of gen rows: where CBGX_FWD_H_ON_SOURCES defines h_out"""
    src, dst = OU.knn_graph(g["x"], g["batch_idx"], 32)
    a1 = g["gen_flag"] | g["lig_flag"]
    a1 = a1.clone()
    a1[src[g["gen_flag"][dst]]] = True
    return a1


def score_weights(g, seed, with_h, h_rows=None):
    gen = torch.Generator().manual_seed(seed)
    N = g["x"].shape[0]
    wx = torch.randn(N, 3, generator=gen) * g["gen_flag"][:, None].float()
    wl = torch.randn(N, NUM_CLASSES, generator=gen) * g["lig_flag"][:, None].float()
    wh = None
    if with_h:
        wh = torch.randn(N, 128, generator=gen) * 0.1
        if h_rows is not None:
            wh = wh * h_rows[:, None].float()
    return wx, wl, wh


def score(xo, ho, lo, w):
    wx, wl, wh = [None if t is None else t.to(device=xo.device, dtype=xo.dtype) for t in w]
    s = (xo * wx).sum() + (lo * wl).sum()
    return s if wh is None else s + (ho * wh).sum()


def oracle_denoiser(sd, g, w, num_layers=None, force=None, dtype=torch.float64):
    """autograd of score(oracle forward) -> (near, {"x": dx, "h": dh, param name: dparam})"""
    sdd = {k: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() and not k.endswith("offset") else v)
           for k, v in denoiser_sd(sd, num_layers).items()}
    x = g["x"].to(dtype).clone().requires_grad_(True)
    h = g["h"].to(dtype).clone().requires_grad_(True)
    with relu_margins(force) as near:
        xo, ho, lo = OU.unitransformer_forward({"denoiser." + k: v for k, v in sdd.items()}, x, h, g["batch_idx"], g["lig_flag"],
                                               g["gen_flag"])
        s = score(xo, ho, lo, w)
    s.backward()
    ref = {"x": x.grad, "h": h.grad}
    ref.update({k: v.grad for k, v in sdd.items() if isinstance(v, torch.Tensor) and v.requires_grad})
    return near, ref


def gpu_denoiser(den, g, w, mode, with_h):
    x = g["x"].to(DEV).clone().requires_grad_(True)
    h = g["h"].to(DEV).clone().requires_grad_(True)
    den.zero_grad(set_to_none=True)
    kw = {"ligand_outputs_only": True} if mode == "ligand_outputs_only" else ({"h_on_sources": True} if mode == "h_on_sources" else {})
    xo, ho, lo = den(x, h, g["batch_idx"].to(DEV), g["lig_flag"].to(DEV), g["gen_flag"].to(DEV), **kw)
    s = score(xo, ho if with_h else None, lo, w if with_h else w[:2] + (None,))
    s.backward()
    torch.cuda.synchronize()
    got = {"x": x.grad, "h": h.grad}
    got.update({k: p.grad for k, p in den.named_parameters()})
    return got


@pytest.fixture(scope="module")
def den(synthetic_sd):
    return make_denoiser(synthetic_sd)


CASES = ["denoiser_2graphs", "denoiser_small_graphs", "denoiser_linker", "denoiser_eg5_pocket10"]
MODES = [("full", False), ("full", True), ("ligand_outputs_only", False), ("h_on_sources", True)]


@pytest.mark.parametrize("mode,with_h", MODES, ids=["full", "full_h", "ligand_outputs_only", "h_on_sources_h"])
@pytest.mark.parametrize("case", CASES)
def test_denoiser_coordinate_gradient_matches_autograd(golden_dir, synthetic_sd, den, case, mode, with_h):
    """x.grad (and h.grad and every parameter gradient, with x requiring grad too) of the 9-layer denoiser against the oracle, in
    each forward / backward pruning mode the training path has"""
    g = load(golden_dir, case)
    w = score_weights(g, seed=5, with_h=with_h, h_rows=sources_rows(g) if mode == "h_on_sources" else None)
    got = gpu_denoiser(den, g, w, mode, with_h)
    ref = check(got, lambda force: oracle_denoiser(synthetic_sd, g, w, force=force))
    # protein rows get a gradient through the distances and the gate, which must be there and match on its own
    prot = ~g["lig_flag"]
    assert float(ref["x"][prot].norm()) > 1e-3 * float(ref["x"].norm())
    assert rel_err(got["x"][prot.to(DEV)], ref["x"][prot]) <= TOL
    assert rel_err(got["x"][g["lig_flag"].to(DEV)], ref["x"][g["lig_flag"]]) <= TOL


@pytest.mark.parametrize("case", ["denoiser_2graphs", "denoiser_linker", "denoiser_small_graphs"])
def test_denoiser_coordinate_gradient_in_edge_row_mode(golden_dir, synthetic_sd, den, case):
    """CBGX_BX_EDGE_ROWS=1: the x2h blocks sum their neighbour rows through edge rows; the coordinate gradient is unchanged"""
    g = load(golden_dir, case)
    w = score_weights(g, seed=6, with_h=True)
    with env(CBGX_BX_EDGE_ROWS="1"):
        got = gpu_denoiser(den, g, w, "full", True)
    check(got, lambda force: oracle_denoiser(synthetic_sd, g, w, force=force))


@pytest.mark.parametrize("case", ["denoiser_2graphs", "denoiser_small_graphs"])
def test_one_layer_denoiser_gate_path(golden_dir, synthetic_sd, case):
    """A 1-layer denoiser, where the gate is a large share of dL/dx: the gradient matches the oracle WITH the gate's coordinate path
    and is far from the oracle without it (so the new gate kernel is what closes the gap)"""
    g = load(golden_dir, case)
    den1 = make_denoiser(synthetic_sd, num_layers=1)
    w = score_weights(g, seed=7, with_h=True)
    got = gpu_denoiser(den1, g, w, "full", True)
    ref = check(got, lambda force: oracle_denoiser(synthetic_sd, g, w, num_layers=1, force=force))
    with gate_detached():
        _, ref_ng = oracle_denoiser(synthetic_sd, g, w, num_layers=1)
    gate_share = rel_err(ref_ng["x"], ref["x"])
    assert gate_share > 100 * TOL, gate_share
    assert rel_err(got["x"], ref_ng["x"]) > 50 * TOL


def test_frozen_weight_guidance_gradient(golden_dir, synthetic_sd):
    """Gradient guidance: every parameter frozen, grad mode on, torch.autograd.grad(score(x_out), x) -- the taped path must be taken
    (not the no-grad sampling path) and return the oracle's gradient"""
    g = load(golden_dir, "denoiser_2graphs")
    den1 = make_denoiser(synthetic_sd)
    for p in den1.parameters():
        p.requires_grad_(False)
    w = score_weights(g, seed=8, with_h=False)
    x = g["x"].to(DEV).clone().requires_grad_(True)
    with torch.enable_grad():
        xo, _, lo = den1(x, g["h"].to(DEV), g["batch_idx"].to(DEV), g["lig_flag"].to(DEV), g["gen_flag"].to(DEV))
        (gx,) = torch.autograd.grad(score(xo, None, lo, w), x)
    assert gx is not None

    def oracle_run(force):
        near, ref = oracle_denoiser(synthetic_sd, g, w, force=force)
        return near, {"x": ref["x"]}
    check({"x": gx}, oracle_run)


def test_coordinate_gradient_at_config5_shape(synthetic_sd):
    """32 real-size graphs in one batch (BASELINE configs[4]: ~16.5 k nodes, the fp32 atomics at full scale, the listed-row pruning of
    ligand_outputs_only); graphs do not interact, so x.grad on each of 16 seed-chosen graphs is checked against the oracle run on that
    graph alone"""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    B = 32
    batch = synthetic.denovo_batch(B, seed=406)
    gen = torch.Generator().manual_seed(9)
    parts = []
    for b in range(B):
        xr = batch["protein_pos"][batch["protein_element_batch"] == b]
        xl = batch["ligand_pos"][batch["ligand_element_batch"] == b]
        parts.append((torch.cat([xr, xl]), xr.shape[0], xl.shape[0]))
    x = torch.cat([p[0] for p in parts]).float()
    N = x.shape[0]
    assert N > 14_000
    batch_idx = torch.cat([torch.full((p[1] + p[2],), b, dtype=torch.int64) for b, p in enumerate(parts)])
    lig = torch.cat([torch.cat([torch.zeros(p[1], dtype=torch.bool), torch.ones(p[2], dtype=torch.bool)]) for p in parts])
    h = torch.randn(N, 128, generator=gen)
    g = {"x": x, "h": h, "batch_idx": batch_idx, "lig_flag": lig, "gen_flag": lig.clone()}
    w = score_weights(g, seed=10, with_h=False)
    den9 = make_denoiser(synthetic_sd)
    got = gpu_denoiser(den9, g, w, "ligand_outputs_only", False)["x"].cpu()
    chosen = torch.randperm(B, generator=torch.Generator().manual_seed(11))[:16].tolist()
    for b in chosen:
        rows = batch_idx == b
        gb = {k: v[rows] for k, v in g.items()}
        gb["batch_idx"] = torch.zeros(int(rows.sum()), dtype=torch.int64)
        wb = tuple(t[rows] for t in w[:2]) + (None,)

        def oracle_run(force, gb=gb, wb=wb):
            near, ref = oracle_denoiser(synthetic_sd, gb, wb, force=force, dtype=torch.float32)
            return near, {"x": ref["x"]}
        check({"x": got[rows]}, oracle_run)


# ---- DiffBP's CoMPredictor (H2X stack on its own graph) ----------------------------------------------
@pytest.fixture(scope="module")
def bp():
    sd = W.synthetic_state_dict_diffbp(NUM_CLASSES, 9, seed=0, num_timesteps=1000)
    m = C.get_model(C.default_diffbp_config(NUM_CLASSES))
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), sd


@pytest.mark.parametrize("case", ["denoiser_2graphs", "denoiser_linker", "denoiser_small_graphs", "denoiser_small_graphs/all_rows"])
def test_com_predictor_coordinate_gradient(golden_dir, bp, case, monkeypatch):
    """CoMPredictor with x_composed.requires_grad_(): x.grad, h.grad and the stack's parameter gradients against oracle.diffbp.com_head
    autograd (the stack's blocks, its own distance gate and the zero-COM noise term).  `/all_rows`: the stack's taped forward and backward
    without their row lists (CBGX_TRAIN_STACK_LISTS=0, read at every call), the same bounds."""
    case, _, variant = case.partition("/")
    if variant == "all_rows":
        monkeypatch.setenv("CBGX_TRAIN_STACK_LISTS", "0")
    m, sd = bp
    head = m.com_head
    g = load(golden_dir, case)
    lig, gen_f, bi = g["lig_flag"], g["gen_flag"], g["batch_idx"]
    bl = bi[lig]
    B = int(bi.max()) + 1
    rg = torch.Generator().manual_seed(12)
    n_lig = int(lig.sum())
    x_lig_pred = torch.randn(n_lig, 3, generator=rg)
    w1, w2 = torch.randn(n_lig, 3, generator=rg), torch.randn(n_lig, 3, generator=rg)

    head.zero_grad(set_to_none=True)
    x = g["x"].to(DEV).clone().requires_grad_(True)
    h = g["h"].to(DEV).clone().requires_grad_(True)
    noise, shift = head(x_lig_pred.to(DEV), bl.to(DEV), x, h, gen_f.to(DEV), lig.to(DEV), bi.to(DEV))
    ((noise * w1.to(DEV)).sum() + (shift * w2.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    got = {"x": x.grad, "h": h.grad}
    got.update({k: p.grad for k, p in head.named_parameters()})

    def oracle_run(force):
        sdd = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and not k.endswith("offset") else v)
               for k, v in sd.items() if k.startswith("com_head.")}
        xr = g["x"].double().clone().requires_grad_(True)
        hr = g["h"].double().clone().requires_grad_(True)
        with relu_margins(force) as near:
            nr, sr = OB.com_head(sdd, x_lig_pred.double(), bl, xr, hr, gen_f, lig, bi, B)
            s = (nr * w1.double()).sum() + (sr * w2.double()).sum()
        s.backward()
        ref = {"x": xr.grad, "h": hr.grad}
        ref.update({k[len("com_head."):]: v.grad for k, v in sdd.items() if isinstance(v, torch.Tensor) and v.requires_grad})
        return near, ref

    check(got, oracle_run)


# ---- the fused input side: PLContextEmbedder + compose_context ------------------------------------
def test_fused_compose_embed_coordinate_gradient(synthetic_sd):
    """compose_embed's fused launch (cbgx_embed_compose) makes the composed x differentiable when x_rec / x_lig require grad: their
    gradients equal the unfused tensor path's (cat + index) through plain autograd"""
    from cbgbench_amd.targetdiff import TargetDiff, compose_embed
    m = C.get_model(C.default_targetdiff_config(NUM_CLASSES))
    m.load_state_dict(synthetic_sd, strict=True)
    m = m.to(DEV)
    batch = synthetic.batch_to(synthetic.denovo_batch(3, seed=17), DEV)
    bl, br = batch["ligand_element_batch"], batch["protein_element_batch"]
    sort_idx, batch_idx, lig_flag, lig_rows, graph_ptr = TargetDiff.compose_plan(bl, br, 3)
    n_lig = bl.shape[0]
    c_lig = torch.nn.functional.one_hot(batch["ligand_atom_type"], NUM_CLASSES).float()
    gen_r = torch.zeros(br.shape[0], dtype=torch.bool, device=DEV)
    gen_l = torch.ones(n_lig, dtype=torch.bool, device=DEV)
    wx = torch.randn(sort_idx.shape[0], 3, generator=torch.Generator().manual_seed(13)).to(DEV)
    wh = torch.randn(sort_idx.shape[0], 128, generator=torch.Generator().manual_seed(14)).to(DEV)
    out = []
    for fused in (True, False):
        xr = batch["protein_pos"].float().clone().requires_grad_(True)
        xl = batch["ligand_pos"].float().clone().requires_grad_(True)
        x, h, gflag = compose_embed(m.context_embedder, xr, xl, batch["protein_atom_feature"].float(), batch["protein_aa_type"], c_lig,
                                    sort_idx, gen_r, gen_l, fused=fused)
        if fused:
            assert "ComposeEmbed" in type(h.grad_fn).__name__, type(h.grad_fn).__name__
            assert x.requires_grad and not gflag.requires_grad
        ((x * wx).sum() + (h * wh).sum()).backward()
        out.append((xr.grad.clone(), xl.grad.clone(), x.detach().clone()))
    assert torch.equal(out[0][2], out[1][2])
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # without a coordinate that requires grad, the composed x stays non-differentiable (the training step's graph is unchanged)
    x, _, _ = compose_embed(m.context_embedder, batch["protein_pos"].float(), batch["ligand_pos"].float(),
                            batch["protein_atom_feature"].float(), batch["protein_aa_type"], c_lig, sort_idx, gen_r, gen_l)
    assert not x.requires_grad
