"""DiffBP training with ligands of more than 48 atoms, and its fused forward noising, on the CPU.

Beyond 48 ligand atoms the reference's ``interior_loss`` restricts every protein atom to its 48 nearest ligand atoms
(``torch_cluster.knn(..., k=48)``, diffbp.py:18-28).  ``diffbp_loss_kernel`` (cbgbench_amd/csrc/train_loss_diffbp.hip) makes that
selection itself for ligands of up to 128 atoms; ``diffbp_noise_kernel`` is the forward noising in front of the networks.  Here:

  * the oracle against the reference on two reference-made fixtures with ligands of 60 / 52 and 75 / 49 atoms
    (scripts/make_golden_large_ligands.py), and the conditions on those inputs that make them a test of the selection;
  * a model of the kernel's selection (bisection on the bit pattern of d^2, ties by ligand index) against ``torch.topk``;
  * a model of the kernel's loss formulas with the selection against autograd on the tensor path of ``DiffBP.get_loss``;
  * a model of the noising kernel (its summation order included) against the oracle's restatement on all DiffBP training fixtures;
  * the C ABI of the new exports.

The GPU suite (tests/test_gpu_diffbp_large_ligands.py) runs the kernels themselves against the same yardsticks."""
import os
import re

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native
from cbgbench_amd.diffsbdd import DiffsbddVariationalScheduler as S
from cbgbench_amd.targetdiff import TargetDiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 48
BIG_CASES = ["train_loss_diffbp_big", "train_loss_diffbp_big_ctx"]
ALL_CASES = ["train_loss_diffbp", "train_loss_diffbp_ctx", "train_loss_diffbp_ctx_t0"] + BIG_CASES


# ---- the reference-made fixtures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BIG_CASES)
def test_oracle_matches_reference_on_large_ligands(golden_dir, case):
    """the reference's four losses and the gradients of all 404 tensors, at the bounds of the existing DiffBP golden test"""
    from tests.test_oracle_golden import test_diffbp_training_loss_and_gradients_match_reference as check
    check(golden_dir, case)


def knn_margins(xs, x_rec, bl, br, k=K):
    """per graph with more than k ligand atoms: the smallest relative gap between the k-th and the (k+1)-th smallest d^2 over its
    protein atoms (d^2 as the oracle's knn_cross computes it) -> {graph: gap}"""
    out = {}
    for g in torch.unique(bl).tolist():
        xl, xp = xs[bl == g], x_rec[br == g]
        if xl.shape[0] <= k or xp.shape[0] == 0:
            continue
        d2 = ((xp[:, None, :] - xl[None, :, :]) ** 2).sum(-1).sort(dim=1).values
        out[g] = float(((d2[:, k] - d2[:, k - 1]) / d2[:, k - 1]).min())
    return out


def oracle_interior_inputs(sd, batch, t, eps, u):
    """what the oracle's get_loss hands to its interior_loss: (xs, x_rec, bl, br)"""
    from oracle import diffbp as OD
    seen = {}
    orig = OD.interior_loss

    def spy(xs, x_rec, bl, br, **kw):
        seen["args"] = (xs.detach().clone(), x_rec, bl, br)
        return orig(xs, x_rec, bl, br, **kw)
    OD.interior_loss = spy
    try:
        with torch.no_grad():
            OD.get_loss(sd, batch, t, eps, u, 13, 1000)
    finally:
        OD.interior_loss = orig
    return seen["args"]


@pytest.mark.parametrize("case", BIG_CASES)
def test_large_ligand_fixtures_exercise_the_selection(golden_dir, case):
    """conditions on the INPUTS: at the oracle's xs every protein atom of every graph with more than 48 ligand atoms has a relative gap
    of at least 1e-5 between its 48th and 49th d^2 (fp32 rounding cannot swap them), and the interior loss with k = 48 differs from
    the unrestricted one by more than the loss tolerance of the GPU test (2e-4 |loss| + 1e-6): a kernel without the restriction fails"""
    from oracle import diffbp as OD
    from oracle import weights as W
    from tests.test_host_models_cpu import golden_batch, load
    g = load(golden_dir, case)
    batch = golden_batch(g)
    sizes = torch.bincount(batch["ligand_element_batch"])
    assert int((sizes > K).sum()) == 2 and int(sizes.max()) <= 128
    sd = W.synthetic_state_dict_diffbp(13, 9, seed=0, num_timesteps=1000)
    xs, x_rec, bl, br = oracle_interior_inputs(sd, batch, g["t"], g["eps"], g["u"])
    gaps = knn_margins(xs, x_rec, bl, br)
    assert len(gaps) == 2 and min(gaps.values()) >= 1e-5, gaps
    l48, linf = float(OD.interior_loss(xs, x_rec, bl, br, k=K)), float(OD.interior_loss(xs, x_rec, bl, br, k=1 << 20))
    assert abs(l48 - g["loss_inter"]) <= 1e-6 * abs(l48) + 1e-7
    assert abs(l48 - linf) > 2e-4 * abs(l48) + 1e-6, (l48, linf)


# ---- the kernel's selection ----------------------------------------------------------------------------------------------------------
def select_model(d2, k=K):
    """diffbp_loss_kernel's selection on rows of non-negative fp32 d^2 [P, nl] (nl > k) -> bool [P, nl], exactly k per row.
    T = the smallest bit pattern b with |{l : bits(d2_l) <= b}| >= k, found by 31 halvings of [0, bits(inf)]; kept: d2 < T, and of the
    ties d2 == T the lowest ligand indices up to `cut`."""
    bits = np.ascontiguousarray(d2, dtype=np.float32).view(np.uint32).astype(np.int64)
    P, nl = bits.shape
    lo, hi = np.zeros(P, np.int64), np.full(P, 0x7F800000, np.int64)
    for _ in range(31):
        mid = lo + ((hi - lo) >> 1)
        ok = (bits <= mid[:, None]).sum(1) >= k
        hi = np.where(ok, mid, hi)
        lo = np.where(ok, lo, mid + 1)
    below, tie = bits < lo[:, None], bits == lo[:, None]
    cut = np.full(P, nl, np.int64)
    for p in np.flatnonzero(below.sum(1) + tie.sum(1) > k):
        cut[p] = np.flatnonzero(tie[p])[k - below[p].sum() - 1]
    return below | (tie & (np.arange(nl)[None, :] <= cut[:, None]))


def lexicographic_smallest(d2, k=K):
    keep = np.zeros(d2.shape, bool)
    for p in range(d2.shape[0]):
        keep[p, np.lexsort((np.arange(d2.shape[1]), d2[p]))[:k]] = True
    return keep


@pytest.mark.parametrize("nl", [49, 50, 64, 86, 127, 128])
def test_selection_model_equals_topk(nl):
    rng = np.random.default_rng(nl)
    d2 = (rng.standard_normal((200, nl, 3)).astype(np.float32) ** 2).sum(-1) * np.float32(rng.uniform(0.01, 400.0))
    keep = select_model(d2)
    assert (keep.sum(1) == K).all()
    idx = torch.topk(torch.from_numpy(d2), K, dim=1, largest=False).indices.numpy()
    ref = np.zeros_like(keep)
    np.put_along_axis(ref, idx, True, axis=1)
    assert (keep == ref).all() and (keep == lexicographic_smallest(d2)).all()


def test_selection_model_breaks_exact_ties_by_index():
    rng = np.random.default_rng(5)
    rows = []
    for nl in (49, 64, 86, 128):
        base = (rng.standard_normal((40, nl, 3)).astype(np.float32) ** 2).sum(-1)
        for p in range(40):
            srt = np.sort(base[p])
            m = int(rng.integers(2, 9))                       # m copies of the 48th value, straddling the boundary
            lo = int(rng.integers(K - m + 1, K))              # sorted ranks lo .. lo + m - 1 include rank 47 and rank 48
            pos = rng.permutation(nl)
            row = srt.copy()
            row[lo:lo + m] = srt[K - 1]
            rows.append(np.pad(row[np.argsort(pos)], (0, 128 - nl), constant_values=np.inf))
    rows += [np.pad(np.zeros(60, np.float32), (0, 68), constant_values=np.inf),            # every distance equal (and zero)
             np.pad(np.full(128, 3.5, np.float32), (0, 0))]
    d2 = np.stack(rows).astype(np.float32)
    keep = select_model(d2)
    assert (keep.sum(1) == K).all()
    assert (keep == lexicographic_smallest(d2)).all()
    # the VALUES are those of torch.topk (which of several equal entries it reports is unspecified)
    vals = torch.topk(torch.from_numpy(d2), K, dim=1, largest=False).values.numpy()
    assert (np.sort(np.where(keep, d2, np.inf), axis=1)[:, :K] == vals).all()
    assert keep[-2, :K].all() and keep[-1, :K].all()


# ---- the kernel's loss formulas with the selection -----------------------------------------------------------------------------------
def kernel_model_knn(xo, x_in, x_stack, logits, sort_idx, graph_ptr, pos_noise, com_noise, v0, type_flag, gen, t, n_rec, acp, betas,
                     rho=2.0, gamma=5.0, cap=128):
    """tests/test_diffbp_loss_model.py::kernel_model with what the kernel adds for large ligands: the 48-nearest selection of a graph with
    more than 48 ligand atoms (no gradient through it), and a graph over the cap contributing nothing -> (..., bad)"""
    N, Cn, B, n_lig = xo.shape[0], logits.shape[1], t.shape[0], pos_noise.shape[0]
    a_pos, a_int, b_com, b_int = (torch.zeros(N, 3) for _ in range(4))
    z_atom = torch.zeros(N, Cn)
    gstats = torch.zeros(B, 6)
    bad = 0
    for g in range(B):
        r0, r1 = int(graph_ptr[g]), int(graph_ptr[g + 1])
        rows = torch.arange(r0, r1)
        lrow = rows[sort_idx[rows] >= n_rec]
        prow = rows[sort_idx[rows] < n_rec]
        ai = sort_idx[lrow] - n_rec
        nl = lrow.numel()
        if nl > cap:
            bad = 1
            continue
        a, b = acp[t[g]], betas[t[g]]
        kap, isb = -b / ((1 - a).sqrt() * (1 - b).sqrt()), 1.0 / (1 - b).sqrt()
        xt = x_in[lrow]
        nz, dl = xo[lrow] - xt, x_stack[lrow] - xt
        eps, com = nz - nz.sum(0) / max(nl, 1), (dl.sum(0) / max(nl, 1)).expand(nl, 3)
        gn, tf = gen[ai], type_flag[ai]
        mp, mc = ((eps - pos_noise[ai]) ** 2).sum(1), ((com - com_noise[ai]) ** 2).sum(1)
        xs = torch.where(gn[:, None], (xt + b * (-(eps + com) / (1 - a).sqrt())) * isb, xt)
        p = torch.softmax(logits[lrow], 1)
        u = torch.softmax(p, 1) - torch.nn.functional.one_hot(v0[ai], Cn).float()
        ce = -p.gather(1, v0[ai, None])[:, 0] + torch.logsumexp(p, 1)
        dz = p * (u - (p * u).sum(1, keepdim=True))
        cg, ct = max(float(gn.sum()), 1.0), max(float(tf.sum()), 1.0)
        d = xs[:, None, :] - x_in[prow][None, :, :]                  # [nl, P, 3]
        d2 = (d ** 2).sum(-1)
        e = torch.exp(-d2 / rho)
        if nl > K and prow.numel():
            e = e * torch.from_numpy(select_model(d2.t().contiguous().numpy())).t().float()
        acc, sx = e.sum(1), (e[:, :, None] * d).sum(1)
        rr = gamma - (-rho * torch.log(acc + 1e-3))
        w = torch.where(rr >= 0, -2.0 / (n_lig * (acc + 1e-3)), torch.zeros_like(acc))
        gi = torch.where(gn[:, None], kap * w[:, None] * sx, torch.zeros(nl, 3))
        gp = torch.where(gn[:, None], 2.0 * (eps - pos_noise[ai]) / cg, torch.zeros(nl, 3))
        gc = torch.where(gn[:, None], 2.0 * (com - com_noise[ai]) / cg, torch.zeros(nl, 3))
        a_pos[lrow] = gp - gp.mean(0)
        a_int[lrow] = gi - gi.mean(0)
        b_com[lrow] = gc.mean(0).expand(nl, 3)
        b_int[lrow] = gi.mean(0).expand(nl, 3)
        z_atom[lrow] = torch.where(tf[:, None], dz / ct, torch.zeros(nl, Cn))
        gstats[g] = torch.stack([mp[gn].sum() / cg, mc[gn].sum() / cg, ce[tf].sum() / ct, rr.clamp(min=0).sum(), gn.sum().float(),
                                 tf.sum().float()])
    top = lambda col: float(max([g for g in range(B) if gstats[g, col] > 0], default=-1) + 1) or 1.0
    dg, dt = top(4), top(5)
    losses = torch.stack([gstats[:, 0].sum() / dg, gstats[:, 2].sum() / dt, gstats[:, 1].sum() / dg, gstats[:, 3].sum() / max(n_lig, 1)])
    return losses, (1.0 / dg, 1.0 / dt), a_pos, a_int, b_com, b_int, z_atom, bad


def loss_entry_inputs(sizes_r, sizes_l, seed, frozen=0.2):
    """seeded operands of the loss entry (what the two networks would hand it) for graphs of the given protein / ligand sizes"""
    gen = torch.Generator().manual_seed(seed)
    B = len(sizes_r)
    br = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes_r))
    bl = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes_l))
    n_rec, n_lig = br.shape[0], bl.shape[0]
    sort_idx, batch_idx, lig_flag, lig_rows, graph_ptr = TargetDiff.compose_plan(bl, br, B)
    N = n_rec + n_lig
    x_in = torch.randn(N, 3, generator=gen) * 2.5
    x_in[lig_rows] = x_in[lig_rows] * 0.5                       # ligands inside their pockets: the interior term is active
    d = dict(B=B, br=br, bl=bl, n_rec=n_rec, n_lig=n_lig, sort_idx=sort_idx, lig_flag=lig_flag, lig_rows=lig_rows, graph_ptr=graph_ptr,
             x_in=x_in, xo=x_in + 0.3 * torch.randn(N, 3, generator=gen), x_stack=x_in + 0.2 * torch.randn(N, 3, generator=gen),
             logits=torch.randn(N, 13, generator=gen), pos_noise=torch.randn(n_lig, 3, generator=gen),
             com_noise=torch.randn(n_lig, 3, generator=gen), v0=torch.randint(0, 13, (n_lig,), generator=gen))
    d["gen"] = torch.rand(n_lig, generator=gen) >= frozen
    d["type_flag"] = d["gen"] & (torch.rand(n_lig, generator=gen) < 0.6)
    d["t"] = torch.randint(0, 1000, (B,), generator=gen)
    return d


@pytest.mark.parametrize("seed", [0, 1])
def test_fused_loss_formulas_with_selection_match_autograd_on_the_tensor_path(seed):
    """ligands of 49, 64, 86 and 128 atoms next to small ones, as tests/test_diffbp_loss_model.py does for small ligands"""
    m = C.get_model(C.default_diffbp_config(13)).train()
    sizes_r, sizes_l = [70, 95, 120, 150, 60, 81], [49, 64, 86, 128, 7, 48]
    c = loss_entry_inputs(sizes_r, sizes_l, seed)
    B, bl, br, lig_rows, lig_flag, x_in, t = c["B"], c["bl"], c["br"], c["lig_rows"], c["lig_flag"], c["x_in"], c["t"]
    xo, x_stack, logits = (c[k].clone().requires_grad_(True) for k in ("xo", "x_stack", "logits"))
    ps = m.pos_scheduler
    x_t, x_rec = x_in[lig_rows], x_in[~lig_flag]
    noise = xo[lig_rows] - x_t
    x_lig_pred = noise - S.scatter_mean(noise, bl, B)[bl]
    x_com_pred = S.scatter_mean((x_stack - x_in)[lig_rows], bl, B)[bl]
    loss_pos = ps.get_score_loss(x_lig_pred, c["pos_noise"], t, c["gen"], bl, score_in=False)[0]
    loss_com = ps.get_score_loss(x_com_pred, c["com_noise"], t, c["gen"], bl, score_in=False, info_tag="com")[0]
    loss_atom = m.type_scheduler.get_loss(logits[lig_rows], c["v0"], c["v0"], t, c["type_flag"], bl, pred_logit=True)[0]
    xs = ps.xs_mean(x_lig_pred + x_com_pred, x_t, t, bl, gen_flag=c["gen"])
    loss_inter = m.interior_loss(xs, x_rec, bl, br, n_graphs=B, max_ligand_atoms=max(sizes_l))
    # the inputs exercise the restriction: no exact tie at the boundary, and k = 48 is not k = infinity
    assert min(knn_margins(xs.detach(), x_rec, bl, br).values()) > 1e-6
    unrestricted = m.interior_loss(xs.detach(), x_rec, bl, br, k=1 << 20, n_graphs=B, max_ligand_atoms=max(sizes_l))
    assert abs(float(unrestricted) - float(loss_inter.detach())) > 1e-3 * float(unrestricted)
    wts = {"pos": 1.0, "atom": 0.7, "com": 1.3, "inter": 0.9}
    (wts["pos"] * loss_pos + wts["atom"] * loss_atom + wts["com"] * loss_com + wts["inter"] * loss_inter).backward()
    with torch.no_grad():
        losses, scal, a_pos, a_int, b_com, b_int, z_atom, bad = kernel_model_knn(
            xo.detach(), x_in, x_stack.detach(), logits.detach(), c["sort_idx"], c["graph_ptr"], c["pos_noise"], c["com_noise"], c["v0"],
            c["type_flag"], c["gen"], t, c["n_rec"], ps.alphas_cumprod.float(), ps.betas.float())
    assert bad == 0
    for k, ref in zip(range(4), (loss_pos, loss_atom, loss_com, loss_inter)):
        assert abs(float(losses[k]) - float(ref.detach())) <= 2e-5 * abs(float(ref.detach())) + 1e-7, (k, float(losses[k]), float(ref.detach()))
    assert float(loss_inter.detach()) > 0.0
    gx = wts["pos"] * scal[0] * a_pos + wts["inter"] * a_int
    gs = wts["com"] * scal[0] * b_com + wts["inter"] * b_int
    gl = wts["atom"] * scal[1] * z_atom
    for got, ref, name in ((gx, xo.grad, "x_out"), (gs, x_stack.grad, "x_stack"), (gl, logits.grad, "logits")):
        assert float(ref[~lig_flag].abs().max()) == 0.0 and float(got[~lig_flag].abs().max()) == 0.0, name
        assert torch.allclose(got, ref, rtol=2e-4, atol=2e-7), (name, float((got - ref).abs().max()), float(ref.abs().max()))


# ---- the noising kernel --------------------------------------------------------------------------------------------------------------
def noise_model(x0, v0, t, gen, eps, u, sort_idx, graph_ptr, n_rec, num_classes, acp, T, absorbing=0):
    """diffbp_noise_kernel: one workgroup of 256 threads per graph of the composed order; thread-strided partial sums of eps, then the
    halving tree; products of x_t rounded one by one -> (x_t, pos_noise, com_noise, v_t, c_t, type_flag)"""
    x_t, pos_noise, com_noise = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
    v_t, type_flag = torch.empty_like(v0), torch.empty(v0.shape[0], dtype=torch.bool)
    for g in range(t.shape[0]):
        rows = torch.arange(int(graph_ptr[g]), int(graph_ptr[g + 1]))
        ai = (sort_idx[rows] - n_rec)[sort_idx[rows] >= n_rec]
        nl = ai.numel()
        red = torch.zeros(256, 3)
        for i in range(0, nl, 256):                                # thread tid adds atoms tid, tid + 256, ... in that order
            part = eps[ai[i:i + 256]]
            red[:part.shape[0]] += part
        h = 128
        while h > 0:
            red[:h] += red[h:2 * h]
            h >>= 1
        com = red[0] / float(max(nl, 1))
        a = acp[t[g]]
        sa, sb = a.sqrt(), (1.0 - a).sqrt()
        prob = t[g].float().clamp(min=0.0) / float(T)
        gn = gen[ai]
        x_t[ai] = torch.where(gn[:, None], sa * x0[ai] + sb * eps[ai], x0[ai])
        com_noise[ai] = com.expand(nl, 3)
        pos_noise[ai] = eps[ai] - com
        tf = (u[ai] < prob) & gn
        type_flag[ai] = tf
        v_t[ai] = torch.where(tf, torch.full_like(v0[ai], absorbing), v0[ai])
    return x_t, pos_noise, com_noise, v_t, torch.nn.functional.one_hot(v_t, num_classes).float(), type_flag


@pytest.mark.parametrize("case", ALL_CASES)
def test_noising_model_matches_the_oracle(golden_dir, case):
    from oracle import diffbp as OD
    from oracle import weights as W
    from tests.test_host_models_cpu import golden_batch, load
    g = load(golden_dir, case)
    batch, t = golden_batch(g), g["t"]
    x0, v0, bl, br = batch["ligand_pos"], batch["ligand_atom_type"], batch["ligand_element_batch"], batch["protein_element_batch"]
    gen = batch.get("ligand_gen_flag", torch.ones(x0.shape[0], dtype=torch.bool))
    B = int(t.shape[0])
    sd = W.synthetic_state_dict_diffbp(13, 9, seed=0, num_timesteps=1000)
    tb = {"alphas_cumprod": sd["pos_scheduler.alphas_cumprod"]}
    x_ref, pn_ref, cn_ref = OD.pos_forward_add_noise_zero_center(tb, x0, t, bl, gen, g["eps"], B)
    v_ref, c_ref, f_ref = OD.mask_forward_add_noise(1000, 13, v0, t, bl, gen, g["u"])
    sort_idx, _, _, _, graph_ptr = TargetDiff.compose_plan(bl, br, B)
    x_t, pos_noise, com_noise, v_t, c_t, type_flag = noise_model(x0, v0, t, gen, g["eps"], g["u"], sort_idx, graph_ptr, br.shape[0], 13,
                                                                 tb["alphas_cumprod"], 1000)
    assert torch.equal(v_t, v_ref) and torch.equal(c_t, c_ref) and torch.equal(type_flag, f_ref)
    assert bool(type_flag.any()) and bool((type_flag <= gen).all())
    for got, ref, name in ((x_t, x_ref, "x_t"), (pos_noise, pn_ref, "pos_noise"), (com_noise, cn_ref, "com_noise")):
        assert float((got - ref).abs().max()) <= 4e-7 * float(ref.abs().max()), name
    assert torch.equal(x_t[~gen], x0[~gen])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_training_exports_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    declared = set(re.findall(r"\b(cbgx_[a-z0-9_]+)\s*\(", hdr))
    lib = _native.lib()
    for name in ("cbgx_diffbp_train_noise", "cbgx_diffbp_loss_knn", "cbgx_diffbp_loss"):
        assert name in declared and name in _native.EXPORTS and hasattr(lib, name), name
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    assert int(re.search(r"#define\s+CBGX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6
    from cbgbench_amd import diffbp
    assert diffbp.FUSED_MAX_LIGAND_ATOMS == 128
