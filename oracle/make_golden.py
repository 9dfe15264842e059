"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/* from the REFERENCE itself.

Runs only in the build container (needs /root/reference).  Imports the
reference's unmodified ``TargetDiff`` / ``UniTransformer`` through
``oracle/ref_shim.py``, loads the deterministic synthetic weights of
``oracle/weights.py`` with ``load_state_dict(strict=True)``, runs the reference
on seeded inputs and stores inputs + outputs as small ``.npz`` fixtures.  The
oracle (``tests/test_oracle_golden.py``) and the HIP path (``tests/test_gpu_*``)
are both checked against these files.

    python -m oracle.make_golden            # rewrites tests/golden/
"""
import json
import os
import shutil
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim, weights as W  # noqa: E402
from cbgbench_amd import synthetic as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _np(t):
    t = t.detach().cpu()
    if t.dtype == torch.int64:
        return t.numpy().astype(np.int64)
    return t.numpy()


def compose_inputs(model, batch, x_lig, c_lig):
    """Exactly targetdiff.py:155-160 on the reference modules; returns the denoiser kwargs."""
    from repo.modules.common import compose_context
    x_rec = batch["protein_pos"]
    aa = F.one_hot(batch["protein_aa_type"], 20).float()
    lig_flag, rec_flag = batch["ligand_lig_flag"], batch["protein_lig_flag"]
    gen_l = batch.get("ligand_gen_flag", lig_flag)
    gen_r = torch.zeros_like(rec_flag)
    bl, br = batch["ligand_element_batch"], batch["protein_element_batch"]
    xl, xr, hl, hr = model.context_embedder(x_lig, x_rec, c_lig, batch["protein_atom_feature"], aa,
                                            bl, br, lig_flag, rec_flag, None)
    ctx, batch_idx, _ = compose_context({"x": xl, "h": hl, "gen_flag": gen_l, "lig_flag": lig_flag},
                                        {"x": xr, "h": hr, "gen_flag": gen_r, "lig_flag": rec_flag}, bl, br)
    return ctx, batch_idx


def small_batch(sizes, seed, num_classes=13, ctx=None):
    rng = np.random.default_rng(seed)
    pockets = [S.make_pocket(rng, nr, radius=7.0) for nr, _ in sizes]
    return S.make_batch(pockets, [nl for _, nl in sizes], rng, num_classes, n_ctx_list=ctx)


def sidechain_order(batch, seed):
    """Sidechain-style context mask: the ligand rows of every graph in a seeded random order, so that context and generated
    atoms interleave instead of the context forming a prefix.  Position, type and ``ligand_gen_flag`` move together; the graph
    ids stay sorted."""
    rng = np.random.default_rng(seed)
    bl = batch["ligand_element_batch"].numpy()
    perm = np.concatenate([rng.permutation(np.flatnonzero(bl == g)) for g in range(int(bl.max()) + 1)])
    out = dict(batch)
    for k in ("ligand_pos", "ligand_atom_type", "ligand_gen_flag"):
        out[k] = batch[k][torch.from_numpy(perm)]
    return out


def _denoiser_case(model, name, batch):
    c_lig = F.one_hot(batch["ligand_atom_type"], model.num_classes).float()
    ctx, batch_idx = compose_inputs(model, batch, batch["ligand_pos"], c_lig)
    with torch.no_grad():
        x, h = ctx["x"], ctx["h"]
        den = model.denoiser
        edge_index = den._connect_edge(x, ctx["lig_flag"], batch_idx)
        edge_type = den._build_edge_type(edge_index, ctx["lig_flag"])
        src, dst = edge_index
        e_w = torch.sigmoid(den.dist_emb(torch.norm(x[dst] - x[src], p=2, dim=-1, keepdim=True)))
        h_l0 = den.blocks[0].x2h_layers[0](x, h, edge_type, edge_index, e_w)
        x_l0, _ = den.blocks[0](x, h, edge_type, edge_index, e_w=e_w, gen_flag=ctx["gen_flag"])
        xo, ho, logits = den(batch_idx=batch_idx, **ctx)
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"),
        x=_np(x), h=_np(h), batch_idx=_np(batch_idx), lig_flag=_np(ctx["lig_flag"]), gen_flag=_np(ctx["gen_flag"]),
        edge_index=_np(edge_index).astype(np.int32), edge_type=_np(edge_type.argmax(-1)).astype(np.int8), e_w=_np(e_w),
        h_layer0=_np(h_l0), x_layer0=_np(x_l0), x_out=_np(xo), h_out=_np(ho), logits=_np(logits),
    )
    print(name, "N =", x.shape[0], "E =", edge_index.shape[1])


def _step_case(model, name, batch, t_idx, seed):
    """One pass of the loop body targetdiff.py:150-180 with torch RNG seeded so that the
    scheduler's randn_like / rand_like draws can be replayed as explicit eps / u."""
    C = model.num_classes
    x_lig = batch["ligand_pos"]
    c_lig = F.one_hot(batch["ligand_atom_type"], C).float()
    bl = batch["ligand_element_batch"]
    gen_l = batch.get("ligand_gen_flag", batch["ligand_lig_flag"])
    B = int(bl.max()) + 1
    t = torch.full((B,), t_idx, dtype=torch.long)
    with torch.no_grad():
        ctx, batch_idx = compose_inputs(model, batch, x_lig, c_lig)
        x, h, v = model.denoiser(batch_idx=batch_idx, **ctx)
        x_pred, c_pred = x[ctx["lig_flag"]], v[ctx["lig_flag"]]
        torch.manual_seed(seed)
        x_next = model.pos_scheduler.backward_remove_noise(x_pred, x_lig, t, bl, gen_l, type="denoise")
        c_next, v_next = model.type_scheduler.backward_remove_noise(c_pred, c_lig, t, bl, gen_l, pred_logit=True)
    torch.manual_seed(seed)
    eps = torch.randn_like(x_lig)
    u = torch.rand(x_lig.shape[0], C)
    d = {k: _np(v) for k, v in batch.items()}
    np.savez_compressed(os.path.join(OUT, name + ".npz"), t_idx=t_idx, eps=_np(eps), u=_np(u),
                        x_pred=_np(x_pred), c_pred=_np(c_pred), x_next=_np(x_next), c_next=_np(c_next),
                        v_next=_np(v_next), **{"batch_" + k: v for k, v in d.items()})
    print(name, "t =", t_idx)


def _train_case(model, name, batch, seed, t_override=None):
    """``model.train(); loss_dict, _ = model(batch); sum_weighted_losses(...).backward()`` (train.py:185-189) on the
    unmodified reference, torch RNG seeded so that sample_time's randint, forward_add_noise's randn_like and
    log_sample_categorical's rand_like can be replayed as explicit draws / eps / u.  Stores the two losses, the
    gradient norm of every trainable tensor, full gradients of the small tensors and a strided sample of the
    large ones."""
    C = model.num_classes
    T = model.num_diffusion_timesteps
    bl = batch["ligand_element_batch"]
    B = int(bl.max()) + 1
    model.train()
    model.zero_grad()
    torch.manual_seed(seed)
    if t_override is None:
        loss_dict, _ = model(batch)
    else:   # get_loss with a fixed t (covers the t == 0 decoder-NLL branch deterministically)
        lig_flag, rec_flag = batch["ligand_lig_flag"], batch["protein_lig_flag"]
        loss_dict, _ = model.get_loss(batch["ligand_pos"], batch["protein_pos"], batch["ligand_atom_type"],
                                      batch["protein_atom_feature"], batch["protein_aa_type"], lig_flag, rec_flag,
                                      bl, batch["protein_element_batch"], batch.get("ligand_gen_flag", lig_flag),
                                      torch.zeros_like(rec_flag), t_override)
    loss = 1.0 * loss_dict["pos"] + 100.0 * loss_dict["atom"]
    loss.backward()
    torch.manual_seed(seed)
    if t_override is None:
        draws = torch.randint(0, T, size=(B // 2 + 1,))
        t = torch.cat([draws, T - draws - 1], 0)[:B]
    else:
        draws, t = torch.zeros(0, dtype=torch.long), t_override
    eps = torch.randn_like(batch["ligand_pos"])
    u = torch.rand(batch["ligand_pos"].shape[0], C)
    out = {"seed": seed, "draws": _np(draws), "t": _np(t), "eps": _np(eps), "u": _np(u),
           "loss_pos": _np(loss_dict["pos"]), "loss_atom": _np(loss_dict["atom"])}
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out["gnorm/" + k] = np.float64(g.double().norm().item())
        flat = g.reshape(-1)
        out["g/" + k] = _np(flat if flat.numel() <= 2048 else flat[::61])
    out.update({"batch_" + k: _np(v) for k, v in batch.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    model.eval()
    model.zero_grad()
    print(name, "loss", float(loss_dict["pos"]), float(loss_dict["atom"]), "t", t.tolist())


def _sample_case(name, batch, T, seed):
    """Full ``TargetDiff.sample`` (targetdiff.py:127-184) of a T-step model, torch RNG seeded."""
    M = ref_shim.load_reference()
    cfg = ref_shim.targetdiff_config(13, 9)
    cfg.generator.num_diffusion_timesteps = T
    model = M.get_model(cfg).eval()
    model.load_state_dict(W.synthetic_state_dict(13, 9, seed=0, num_timesteps=T), strict=True)
    torch.manual_seed(seed)
    with torch.no_grad():
        traj = model.sample(batch)
    out = {"T": T, "seed": seed}
    for k, (xx, cc, bb) in traj.items():
        out[f"traj_x_{k}"] = _np(xx)
        out[f"traj_c_{k}"] = _np(cc)
    out.update({"batch_" + k: _np(v) for k, v in batch.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "keys", sorted(traj.keys()))


def _diffsbdd_case(name, batch, T, seed):
    """Full ``DiffSBDD.sample`` (diffsbdd.py:240-319) of a T-step model, torch RNG seeded; also dumps the state-dict
    key listing and the reference's own gamma table."""
    M = ref_shim.load_reference()
    cfg = ref_shim.AttrDict(
        type="diffsbdd", num_atomtype=8,
        encoder=dict(type="unitransformer", node_feat_dim=128, n_heads=16, num_layers=9),
        generator=dict(pos_schedule=dict(type="polynomial_2"), atom_schedule=dict(type="polynomial_2"),
                       num_diffusion_timesteps=T, time_sampler="random"),
        embedder=dict(emb_dim=128, atom=dict(type="linear"), residue=dict(type="linear")))
    model = M.get_model(cfg).eval()
    ref_sd = model.state_dict()
    with open(os.path.join(OUT, "state_dict_keys_diffsbdd.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in ref_sd.items()}, f, indent=0)
    sd = W.synthetic_state_dict_diffsbdd(8, 9, seed=0, num_timesteps=T)
    assert torch.equal(sd["pos_scheduler.gamma.gamma"], ref_sd["pos_scheduler.gamma.gamma"])
    model.load_state_dict(sd, strict=True)
    torch.manual_seed(seed)
    with torch.no_grad():
        traj = model.sample(batch)
    out = {"T": T, "seed": seed, "gamma": _np(ref_sd["pos_scheduler.gamma.gamma"])}
    for k, (xx, cc, bb) in traj.items():
        out[f"traj_x_{k}"] = _np(xx)
        out[f"traj_c_{k}"] = _np(cc)
    out.update({"batch_" + k: _np(v) for k, v in batch.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    # and the 1000-step gamma table of a freshly built reference model
    cfg.generator.num_diffusion_timesteps = 1000
    np.savez_compressed(os.path.join(OUT, "diffsbdd_gamma_T1000.npz"),
                        gamma=_np(M.get_model(cfg).state_dict()["pos_scheduler.gamma.gamma"]))
    print(name, "keys", sorted(traj.keys()))


def _diffbp_case(name, batch, T, seed):
    """Full ``DiffBP.sample`` (diffbp.py:240-299) of a T-step model, torch RNG seeded."""
    M = ref_shim.load_reference()
    cfg = ref_shim.AttrDict(
        type="diffbp", num_atomtype=13,
        encoder=dict(type="unitransformer", node_feat_dim=128, n_heads=16, num_layers=9),
        generator=dict(pos_schedule=dict(type="sigmoid", beta_start=1.0e-7, beta_end=2.0e-3),
                       atom_schedule=dict(type="uniform"), num_diffusion_timesteps=T, time_sampler="symmetric",
                       com_schedule=dict(type="log", sigma_min=1.0e-7, sigma_max=5.0)),
        embedder=dict(emb_dim=128, atom=dict(type="linear"), residue=dict(type="linear")))
    model = M.get_model(cfg).eval()
    with open(os.path.join(OUT, "state_dict_keys_diffbp.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in model.state_dict().items()}, f, indent=0)
    model.load_state_dict(W.synthetic_state_dict_diffbp(13, 9, seed=0, num_timesteps=T), strict=True)
    torch.manual_seed(seed)
    with torch.no_grad():
        traj = model.sample(batch)
    out = {"T": T, "seed": seed}
    for k, (xx, cc, bb) in traj.items():
        out[f"traj_x_{k}"] = _np(xx)
        out[f"traj_c_{k}"] = _np(cc)
    out.update({"batch_" + k: _np(v) for k, v in batch.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "keys", sorted(traj.keys()))


EXAMPLES = {   # scripts/example/<dir>: (protein PDB, ligand SDF)
    "Eg5": ("3zcw_protein.pdb", "3zcw_ligand.sdf"),
    "adrb1": ("2VT4_protein.pdb", "2VT4_ligand.sdf"),
    "drd2": ("6CM4_protein.pdb", "6CM4_ligand.sdf"),
    "smarca2": ("6HAX_protein.pdb", "6HAX_ligand.sdf"),
}


def eg5_pocket(radius=10.0):
    return example_pocket("Eg5", radius)


def example_pocket(example, radius=10.0):
    """scripts/example/<example> (Eg5 = PDB 3ZCW, adrb1 = 2VT4, drd2 = 6CM4, smarca2 = 6HAX): heavy atoms of residues with any atom
    within ``radius`` A of a ligand heavy atom -- the pocket criterion of datasets/parsers/protein_parser.py:167-177 --
    parsed from plain text (no RDKit/BioPython here)."""
    base = os.path.join(ref_shim.REFERENCE_ROOT, "scripts", "example", example)
    pdb_name, sdf_name = EXAMPLES[example]
    lig = []
    with open(os.path.join(base, sdf_name)) as f:
        lines = f.read().splitlines()
    na = int(lines[3][:3])
    for ln in lines[4:4 + na]:
        if ln[31:34].strip() != "H":
            lig.append([float(ln[0:10]), float(ln[10:20]), float(ln[20:30])])
    lig = np.array(lig, np.float32)
    atoms = []
    aa3 = ["ALA", "CYS", "ASP", "GLU", "PHE", "GLY", "HIS", "ILE", "LYS", "LEU", "MET", "ASN", "PRO", "GLN",
           "ARG", "SER", "THR", "VAL", "TRP", "TYR"]
    elem_idx = {"H": 0, "C": 1, "N": 2, "O": 3, "S": 4, "SE": 5}
    with open(os.path.join(base, pdb_name)) as f:
        for ln in f:
            if not ln.startswith("ATOM"):
                continue
            el = ln[76:78].strip().upper()
            res = ln[17:20]
            if el == "H" or el not in elem_idx or res not in aa3:
                continue
            atoms.append((ln[21], int(ln[22:26]), ln[26], res, ln[12:16].strip(), el,
                          float(ln[30:38]), float(ln[38:46]), float(ln[46:54])))
    pos = np.array([a[6:9] for a in atoms], np.float32)
    d = np.sqrt(((pos[:, None] - lig[None]) ** 2).sum(-1)).min(1)
    keep_res = {(a[0], a[1], a[2]) for a, dd in zip(atoms, d) if dd <= radius}
    sel = [i for i, a in enumerate(atoms) if (a[0], a[1], a[2]) in keep_res]
    pos = pos[sel]
    feat = np.zeros((len(sel), 7), np.float32)
    aa = np.zeros(len(sel), np.int64)
    for r, i in enumerate(sel):
        a = atoms[i]
        feat[r, elem_idx[a[5]]] = 1.0
        feat[r, 6] = a[4] in ("N", "CA", "C", "O")
        aa[r] = aa3.index(a[3])
    centre = pos.mean(0, keepdims=True)
    return (pos - centre).astype(np.float32), feat, aa, (lig - centre).astype(np.float32)


def denoiser_case(model, name, *a, **k):
    if _selected(name):
        _denoiser_case(model, name, *a, **k)


def step_case(model, name, *a, **k):
    if _selected(name):
        _step_case(model, name, *a, **k)


def train_case(model, name, *a, **k):
    if _selected(name):
        _train_case(model, name, *a, **k)


def sample_case(name, *a, **k):
    if _selected(name):
        _sample_case(name, *a, **k)


def diffbp_case(name, *a, **k):
    if _selected(name):
        _diffbp_case(name, *a, **k)


def diffsbdd_case(name, *a, **k):
    if _selected(name):
        _diffsbdd_case(name, *a, **k)


def diffbp_train_case(name, batch, seed, t_override=None):
    """DiffBP training step of the unmodified reference (diffbp.py:154-231; loss weights all 1,
    configs/denovo/train/diffbp.yml:37-41): the four losses and the gradient of every trainable tensor.  With
    ``t_override`` the reference's ``get_loss`` runs at that time vector and no time is drawn."""
    if not _selected(name):
        return
    M = ref_shim.load_reference()
    T = 1000
    cfg = ref_shim.AttrDict(
        type="diffbp", num_atomtype=13,
        encoder=dict(type="unitransformer", node_feat_dim=128, n_heads=16, num_layers=9),
        generator=dict(pos_schedule=dict(type="sigmoid", beta_start=1.0e-7, beta_end=2.0e-3),
                       atom_schedule=dict(type="uniform"), num_diffusion_timesteps=T, time_sampler="symmetric",
                       com_schedule=dict(type="log", sigma_min=1.0e-7, sigma_max=5.0)),
        embedder=dict(emb_dim=128, atom=dict(type="linear"), residue=dict(type="linear")))
    model = M.get_model(cfg)
    model.load_state_dict(W.synthetic_state_dict_diffbp(13, 9, seed=0, num_timesteps=T), strict=True)
    model.train()
    model.zero_grad()
    bl = batch["ligand_element_batch"]
    B = int(bl.max()) + 1
    torch.manual_seed(seed)
    if t_override is None:
        loss_dict, _ = model(batch)
    else:
        lig_flag, rec_flag = batch["ligand_lig_flag"], batch["protein_lig_flag"]
        loss_dict, _ = model.get_loss(batch["ligand_pos"], batch["protein_pos"], batch["ligand_atom_type"],
                                      batch["protein_atom_feature"], batch["protein_aa_type"], lig_flag, rec_flag, bl,
                                      batch["protein_element_batch"], batch.get("ligand_gen_flag", lig_flag),
                                      torch.zeros_like(rec_flag), t_override)
    sum(loss_dict.values()).backward()
    torch.manual_seed(seed)
    if t_override is None:
        draws = torch.randint(0, T, size=(B // 2 + 1,))
        t = torch.cat([draws, T - draws - 1], 0)[:B]
    else:
        t = t_override
    eps = torch.randn_like(batch["ligand_pos"])
    u = torch.rand(batch["ligand_pos"].shape[0])
    out = {"seed": seed, "t": _np(t), "eps": _np(eps), "u": _np(u)}
    for k, v in loss_dict.items():
        out["loss_" + k] = _np(v)
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out["gnorm/" + k] = np.float64(g.double().norm().item())
        flat = g.reshape(-1)
        out["g/" + k] = _np(flat if flat.numel() <= 2048 else flat[::61])
    out.update({"batch_" + k: _np(v) for k, v in batch.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, {k: float(v) for k, v in loss_dict.items()}, "t", t.tolist())


def diffsbdd_train_case(name, batch, seed, t_override=None):
    """DiffSBDD training step of the unmodified reference (diffsbdd.py:45-195): the two losses and all gradients."""
    if not _selected(name):
        return
    M = ref_shim.load_reference()
    T = 1000
    cfg = ref_shim.AttrDict(
        type="diffsbdd", num_atomtype=8,
        encoder=dict(type="unitransformer", node_feat_dim=128, n_heads=16, num_layers=9),
        generator=dict(pos_schedule=dict(type="polynomial_2"), atom_schedule=dict(type="polynomial_2"),
                       num_diffusion_timesteps=T, time_sampler="random"),
        embedder=dict(emb_dim=128, atom=dict(type="linear"), residue=dict(type="linear")))
    model = M.get_model(cfg)
    model.load_state_dict(W.synthetic_state_dict_diffsbdd(8, 9, seed=0, num_timesteps=T), strict=True)
    model.train()
    model.zero_grad()
    bl = batch["ligand_element_batch"]
    B = int(bl.max()) + 1
    torch.manual_seed(seed)
    if t_override is None:
        loss_dict, _ = model(batch)
    else:
        lig_flag, rec_flag = batch["ligand_lig_flag"], batch["protein_lig_flag"]
        loss_dict, _ = model.get_loss(batch["ligand_pos"], batch["protein_pos"], batch["ligand_atom_type"],
                                      batch["protein_atom_feature"], batch["protein_aa_type"], lig_flag, rec_flag, bl,
                                      batch["protein_element_batch"], batch.get("ligand_gen_flag", lig_flag),
                                      torch.zeros_like(rec_flag), t_override)
    sum(loss_dict.values()).backward()
    torch.manual_seed(seed)
    t = torch.randint(0, T + 1, size=(B,)).float() if t_override is None else t_override
    eps_x = torch.randn_like(batch["ligand_pos"])
    eps_c = torch.randn(batch["ligand_pos"].shape[0], 8)
    out = {"seed": seed, "t": _np(t), "eps_x": _np(eps_x), "eps_c": _np(eps_c)}
    for k, v in loss_dict.items():
        out["loss_" + k] = _np(v)
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        out["gnorm/" + k] = np.float64(g.double().norm().item())
        flat = g.reshape(-1)
        out["g/" + k] = _np(flat if flat.numel() <= 2048 else flat[::61])
    out.update({"batch_" + k: _np(v) for k, v in batch.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, {k: float(v) for k, v in loss_dict.items()}, "t", t.tolist())


def diffsbdd_eval_case(name, batch, seed, eval_interval=3):
    """DiffSBDD.forward of the unmodified reference in eval mode (diffsbdd.py:72-86): variational bound averaged over
    ``eval_interval`` evenly spaced times, two denoiser calls per time."""
    if not _selected(name):
        return
    M = ref_shim.load_reference()
    T = 1000
    cfg = ref_shim.AttrDict(
        type="diffsbdd", num_atomtype=8, eval_interval=eval_interval,
        encoder=dict(type="unitransformer", node_feat_dim=128, n_heads=16, num_layers=9),
        generator=dict(pos_schedule=dict(type="polynomial_2"), atom_schedule=dict(type="polynomial_2"),
                       num_diffusion_timesteps=T, time_sampler="random"),
        embedder=dict(emb_dim=128, atom=dict(type="linear"), residue=dict(type="linear")))
    model = M.get_model(cfg)
    model.load_state_dict(W.synthetic_state_dict_diffsbdd(8, 9, seed=0, num_timesteps=T), strict=True)
    model.eval()
    torch.manual_seed(seed)
    with torch.no_grad():
        loss_dict, results = model(batch)
    assert len(results) == eval_interval
    torch.manual_seed(seed)
    n = batch["ligand_pos"].shape[0]
    out = {"seed": seed, "eval_interval": eval_interval}
    for k in range(eval_interval):     # draw order per time: pos noise, type noise, then the t = 0 pair
        for tag, shape in (("eps_x", (n, 3)), ("eps_c", (n, 8)), ("eps_x0", (n, 3)), ("eps_c0", (n, 8))):
            out[f"{tag}_{k}"] = _np(torch.randn(*shape))
    for k, v in loss_dict.items():
        out["loss_" + k] = _np(v)
    out.update({"batch_" + k: _np(v) for k, v in batch.items()})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, {k: float(v) for k, v in loss_dict.items()})


def priors_case(name):
    """Ligand-size prior of the reference (repo/datasets/transforms/init_lig.py:28-52,232-258): pocket size function and
    bin lookup on seeded pockets, the bin edges, and per-bin mean / support of the histogram table (the table itself is
    the reference's data file and is NOT stored), plus 4000 draws of sample_atom_num per pocket under a fixed numpy seed
    for a distribution check of the vectorised sampler."""
    if not _selected(name):
        return
    ref_shim.load_reference()
    import repo.datasets.transforms.init_lig as IL
    rng = np.random.default_rng(71)
    out = {}
    sizes, bins = [], []
    for k, (n, rad) in enumerate([(350, 12.0), (500, 12.0), (650, 12.0), (120, 7.0), (40, 5.0), (600, 16.0), (450, 14.0)]):
        pos, _, _ = S.make_pocket(rng, n, radius=rad)
        out[f"pos_{k}"] = pos
        sz = IL.AssignMolSize().get_space_size(torch.from_numpy(pos))
        sizes.append(float(sz))
        bins.append(IL._get_bin_idx(float(sz), IL.config_atom_num))
    out["space_size"] = np.array(sizes, np.float64)
    out["bin_idx"] = np.array(bins, np.int64)
    cfg = IL.config_atom_num
    out["bounds"] = np.array(cfg["bounds"], np.float64)
    out["bin_mean"] = np.array([float(np.dot(v, p)) for v, p in cfg["bins"]])
    out["bin_min"] = np.array([int(np.min(v)) for v, _ in cfg["bins"]])
    out["bin_max"] = np.array([int(np.max(v)) for v, _ in cfg["bins"]])
    np.random.seed(5)
    out["draw_mean"] = np.array([np.mean([IL.sample_atom_num(sz) for _ in range(4000)]) for sz in sizes])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, sizes, bins)


def context_prior_case(name):
    """The reference's transform chain of a context task -- configs/linker/test/targetdiff.yml:20-31 (frag / scaffold / sidechain
    share it): assign_gensize -> assign_genatomtype -> center_pos(ligand, ctx_flag) -> assign_genpos -> merge -- run on seeded
    pockets with fixed context atoms, three replicas each as sample.py:177 makes them, for the three type priors the shipped
    configs use (uniform: targetdiff, absorbing: diffbp, gaussian: diffsbdd).  Stored: the inputs, every merged key of every
    replica, and the merged key list: the schema and the deterministic part (context rows, centring, flags) of the batch that
    cbgbench_amd/priors.py builds."""
    if not _selected(name):
        return
    ref_shim.load_reference()
    import repo.datasets.transforms.init_lig as IL
    import repo.datasets.transforms.translation  # noqa: F401  (registers center_pos; the module re-uses the class name)
    import repo.datasets.transforms.merge as MG
    from repo.datasets.transforms._base import TRANSFORM_DICT
    rng = np.random.default_rng(91)
    out = {}
    excluded = ["gen_bond_index", "gen_bond_type", "bond_index", "bond_type", "ctx_bond_index", "ctx_bond_type", "gen_index",
                "ctx_index", "cross_bond_index", "cross_bond_type"]
    cases = [("uniform", "add_aromatic", 13), ("absorbing", "add_aromatic", 13), ("gaussian", "basic", 8)]
    pockets = []
    for k, (n, n_ctx) in enumerate([(70, 9), (55, 14), (64, 0)]):
        pos, feat, aa = S.make_pocket(rng, n, radius=8.0)
        pos = pos + rng.standard_normal(3).astype(np.float32) * 4.0          # an un-centred frame, like the raw pocket files
        cpos, ctyp = S.make_context(rng, n_ctx, 8) if n_ctx else (np.zeros((0, 3), np.float32), np.zeros(0, np.int64))
        cpos = cpos + pos.mean(0, keepdims=True)
        pockets.append((pos, feat, aa, cpos, ctyp))
        out[f"pocket{k}_pos"], out[f"pocket{k}_feat"], out[f"pocket{k}_aa"] = pos, feat, aa
        out[f"pocket{k}_ctx_pos"], out[f"pocket{k}_ctx_type"] = cpos, ctyp
    keys = None
    for ci, (dist, mode, C) in enumerate(cases):
        np.random.seed(100 + ci)
        torch.manual_seed(200 + ci)
        for k, (pos, feat, aa, cpos, ctyp) in enumerate(pockets):
            for rep in range(3):
                n_ctx = cpos.shape[0]
                data = ref_shim.AttrDict(
                    protein=dict(pos=torch.from_numpy(pos.copy()), atom_feature=torch.from_numpy(feat), aa_type=torch.from_numpy(aa),
                                 element=torch.zeros(pos.shape[0], dtype=torch.long), lig_flag=torch.zeros(pos.shape[0], dtype=torch.bool)),
                    ligand=dict(pos=torch.from_numpy(cpos.copy()), atom_type=torch.from_numpy(ctyp.copy()),
                                element=torch.zeros(n_ctx, dtype=torch.long), ctx_flag=torch.ones(n_ctx, dtype=torch.bool),
                                gen_flag=torch.zeros(n_ctx, dtype=torch.bool), lig_flag=torch.ones(n_ctx, dtype=torch.bool)))
                data = IL.AssignGenSize("prior_distcond")(data)
                data = IL.AssignGenType(dist, mode)(data)
                data = TRANSFORM_DICT["center_pos"]("ligand", "ctx_flag")(data)
                data = IL.AssignGenPos("gaussian")(data)
                merged = MG.MergeKeys(["protein", "ligand"], to_graph=False, excluded_subkeys=excluded)(data)
                if keys is None:
                    keys = sorted(merged.keys())
                assert sorted(merged.keys()) == keys
                for kk, v in merged.items():
                    out[f"{dist}_p{k}_r{rep}_{kk}"] = _np(v)
    out["merged_keys"] = np.array(keys)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, keys)


def atom_num_table(name="atom_num_dist.npy"):
    """the reference's atom-count histogram table (repo/datasets/transforms/_atom_num_dist.npy: a pickled {'bounds', 'bins'}
    dict), stored as a data fixture so that tests/test_priors.py reads it from tests/golden/"""
    shutil.copyfile(os.path.join(ref_shim.REFERENCE_ROOT, "repo", "datasets", "transforms", "_atom_num_dist.npy"), os.path.join(OUT, name))
    print(name)


def _selected(name):
    """``python -m oracle.make_golden train_`` regenerates only the fixtures whose name contains an argument."""
    sel = sys.argv[1:]
    return not sel or any(a in name for a in sel)


def main():
    os.makedirs(OUT, exist_ok=True)
    M = ref_shim.load_reference()
    for C, tag in ((13, "add_aromatic"), (8, "basic")):
        torch.manual_seed(0)
        m = M.get_model(ref_shim.targetdiff_config(C, 9))
        with open(os.path.join(OUT, f"state_dict_keys_{tag}.json"), "w") as f:
            json.dump({k: list(v.shape) for k, v in m.state_dict().items()}, f, indent=0)
    model = M.get_model(ref_shim.targetdiff_config(13, 9)).eval()
    sd = W.synthetic_state_dict(13, 9, seed=0)
    model.load_state_dict(sd, strict=True)

    # schedule tables straight from a freshly constructed reference model
    torch.manual_seed(0)
    fresh = M.get_model(ref_shim.targetdiff_config(13, 9)).state_dict()
    np.savez_compressed(os.path.join(OUT, "schedule_tables.npz"),
                        **{k: _np(v) for k, v in fresh.items() if "scheduler" in k})

    denoiser_case(model, "denoiser_2graphs", small_batch([(70, 9), (55, 13)], seed=11))
    # graphs with n <= k nodes (degree n-1 < 32), a 2-node graph and a protein-only single node
    denoiser_case(model, "denoiser_small_graphs", small_batch([(20, 5), (28, 5), (1, 1), (30, 4), (1, 0)], seed=12))
    denoiser_case(model, "denoiser_linker", small_batch([(60, 14), (48, 11)], seed=13, ctx=[9, 7]))

    pos, feat, aa, lig = eg5_pocket()
    rng = np.random.default_rng(14)
    b = S.make_batch([(pos, feat, aa)], [lig.shape[0]], rng, 13)
    b["ligand_pos"] = torch.from_numpy(lig + rng.standard_normal(lig.shape).astype(np.float32) * 0.5)
    denoiser_case(model, "denoiser_eg5_pocket10", b)
    # the other three example targets of the reference (real pocket geometry, 10 A pockets as sample.py cuts them); two samples
    # of the ligand per pocket with different noise, as the samplers batch them
    for k, ex in enumerate(("adrb1", "drd2", "smarca2")):
        if not _selected(f"denoiser_{ex}_pocket10"):
            continue
        pos, feat, aa, lig = example_pocket(ex)
        rng = np.random.default_rng(140 + k)
        b = S.make_batch([(pos, feat, aa), (pos, feat, aa)], [lig.shape[0], lig.shape[0]], rng, 13)
        noisy = [lig + rng.standard_normal(lig.shape).astype(np.float32) * sg for sg in (0.5, 2.0)]
        b["ligand_pos"] = torch.from_numpy(np.concatenate(noisy, 0))
        denoiser_case(model, f"denoiser_{ex}_pocket10", b)

    step_case(model, "step_t500", small_batch([(64, 10), (50, 12)], seed=21), 500, seed=5)
    step_case(model, "step_t0", small_batch([(64, 10), (50, 12)], seed=22), 0, seed=6)
    step_case(model, "step_t999_linker", small_batch([(58, 15), (44, 12)], seed=23, ctx=[10, 8]), 999, seed=7)
    train_case(model, "train_loss_denovo", small_batch([(64, 10), (50, 12), (57, 9)], seed=61), seed=15)
    # (batch seed 62 put one value-net ReLU of block 2 within fp32 rounding of zero: centred and uncentred evaluation of the
    # first Linear then disagree by 2 % in that channel's gradients -- same effect as noted at train_loss_diffsbdd_t0)
    train_case(model, "train_loss_t0_linker", small_batch([(58, 15), (44, 12)], seed=68, ctx=[10, 8]), seed=16,
               t_override=torch.tensor([0, 700]))
    priors_case("priors_atom_num")
    if _selected("atom_num_dist"):
        atom_num_table()
    context_prior_case("priors_context_tasks")
    diffsbdd_train_case("train_loss_diffsbdd", small_batch([(64, 10), (50, 12), (57, 9)], seed=64, num_classes=8), seed=18)
    # (seed chosen so that no ReLU of the t = 0 graph sits within rounding of zero: with the unnormalised t = 0 term such
    # a unit makes two fp32 evaluation orders differ by 0.5 % in one tensor -- seen with seed 65)
    diffsbdd_train_case("train_loss_diffsbdd_t0", small_batch([(58, 11), (44, 8)], seed=67, num_classes=8), seed=19,
                        t_override=torch.tensor([0.0, 640.0]))
    diffsbdd_eval_case("eval_loss_diffsbdd", small_batch([(64, 10), (50, 12)], seed=69, num_classes=8), seed=20)
    diffbp_train_case("train_loss_diffbp", small_batch([(64, 10), (50, 12), (57, 9)], seed=63), seed=17)
    sample_case("sample_T5", small_batch([(40, 8), (36, 6)], seed=31), T=5, seed=9)
    b = small_batch([(44, 9), (37, 8)], seed=51)
    b["ligand_atom_type"] = torch.zeros_like(b["ligand_atom_type"])        # absorbing-state prior (assign_atomtype: absorbing)
    diffbp_case("diffbp_sample_T5", b, T=5, seed=13)
    diffsbdd_case("diffsbdd_sample_T5", small_batch([(42, 9), (38, 7)], seed=41, num_classes=8), T=5, seed=11)

    # context tasks (linker / frag / scaffold / sidechain configs): fixed context atoms next to generated ones.  "_ctx" cases
    # with sidechain_order interleave the two kinds; the others keep make_batch's context prefix (linker-style).
    b = sidechain_order(small_batch([(44, 12), (37, 10)], seed=52, ctx=[5, 4]), seed=1)
    b["ligand_atom_type"] = torch.where(b["ligand_gen_flag"], torch.zeros_like(b["ligand_atom_type"]), b["ligand_atom_type"])
    diffbp_case("diffbp_sample_T5_ctx", b, T=5, seed=14)
    diffsbdd_case("diffsbdd_sample_T5_ctx", small_batch([(42, 11), (38, 9)], seed=42, num_classes=8, ctx=[5, 3]), T=5, seed=12)
    diffbp_train_case("train_loss_diffbp_ctx", sidechain_order(small_batch([(64, 14), (50, 12), (57, 9)], seed=73, ctx=[6, 5, 0]),
                                                               seed=2), seed=21)
    # the last graph at t = 0: no type-masked atom there, so the per-graph loss tables end below B
    diffbp_train_case("train_loss_diffbp_ctx_t0", small_batch([(58, 13), (44, 11), (50, 10)], seed=74, ctx=[5, 4, 3]), seed=22,
                      t_override=torch.tensor([650, 300, 0]))
    # a context graph at t = 0: zero_time_loss masks with gen & (t == 0)
    diffsbdd_train_case("train_loss_diffsbdd_ctx", sidechain_order(small_batch([(58, 12), (44, 10), (50, 9)], seed=75, num_classes=8,
                                                                               ctx=[5, 0, 4]), seed=3),
                        seed=23, t_override=torch.tensor([0.0, 640.0, 300.0]))


if __name__ == "__main__":
    main()
