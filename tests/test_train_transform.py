"""Per-visit transforms of training batches (``priors.TrainingPlan``, ``train_cli.apply_plan``, purpose TRAIN_PROTEIN_NORMAL), the parts
that need no GPU: plan parsing, the tensor restatement against the reference's own transform classes bit for bit, the identity plan, the
driver on a stub model, the frame against the sampling path's, the addresses and moments of the protein draws, and the C ABI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

import cbgbench_amd as C
from cbgbench_amd import _native, noise as N, priors, registry, synthetic, train_cli
from cbgbench_amd.config import Config
from cbgbench_amd.priors import TrainingPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle.ref_shim import REFERENCE_ROOT as REFERENCE     # where the reference tree lives when it is on this machine
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "repo")), reason="the reference tree is not on this machine")

# ---- plan parsing ------------------------------------------------------------------------------------------------------------------
# the transform lists of the shipped diffusion train configs (configs/*/common/fa_data_train*.yml, denovo/common/linker_data_train.yml)
LISTS = {
    "denovo/fa_data_train": ("""
        - {type: featurize_protein_fa}
        - {type: featurize_ligand_fa, mode: add_aromatic}
        - {type: add_pos_noise, noise_std: 0.1}
        - {type: center_pos, center_flag: protein}
        - {type: merge, keys: [protein, ligand]}""", (0.1, "protein")),
    "denovo/fa_data_train_diffsbdd": ("""
        - {type: featurize_protein_fa}
        - {type: featurize_ligand_fa, mode: basic}
        - {type: center_whole_pos}
        - {type: merge, keys: [protein, ligand]}""", (0.0, "whole")),
    "linker/fa_data_train": ("""
        - {type: choose_ctx_gen}
        - {type: featurize_protein_fa}
        - {type: featurize_ligand_fa, mode: add_aromatic}
        - {type: add_pos_noise, noise_std: 0.1}
        - {type: center_pos, center_flag: ligand, mask_flag: ctx_flag}
        - {type: merge, keys: [protein, ligand]}""", (0.1, "context")),
    "linker/fa_data_train_diffsbdd": ("""
        - {type: choose_ctx_gen}
        - {type: featurize_protein_fa}
        - {type: featurize_ligand_fa, mode: basic}
        - {type: add_pos_noise, noise_std: 0.1}
        - {type: center_pos, center_flag: ligand, mask_flag: ctx_flag}
        - {type: merge, keys: [protein, ligand]}""", (0.1, "context")),
    "denovo/linker_data_train": ("""
        - {type: select_linker}
        - {type: choose_ctx_gen}
        - {type: featurize_protein_fa}
        - {type: featurize_ligand_fa, mode: basic}
        - {type: add_pos_noise, noise_std: 0.1}
        - {type: center_pos, center_flag: protein}
        - {type: merge, keys: [protein, ligand]}""", (0.1, "protein")),
}


def _cfg(transform_yaml, split="train"):
    return Config({"data": {split: {"transform": yaml.safe_load(transform_yaml)}}})


@pytest.mark.parametrize("name", sorted(LISTS))
def test_plan_of_the_shipped_transform_lists(name):
    text, (std, center) = LISTS[name]
    plan = TrainingPlan.from_config(_cfg(text), "train")
    assert (plan.noise_std, plan.center) == (std, center) and plan == TrainingPlan(std, center)
    # no data.val: validation is not noised and takes the train list's centring
    val = TrainingPlan.from_config(_cfg(text), "val")
    assert (val.noise_std, val.center) == (0.0, center)
    # a val list of its own is read like a train list
    both = _cfg(text)
    both["data"]["val"] = {"transform": yaml.safe_load(LISTS["denovo/fa_data_train_diffsbdd"][0])}
    assert TrainingPlan.from_config(both, "val") == TrainingPlan(0.0, "whole")
    assert TrainingPlan.from_config(both, "train") == TrainingPlan(std, center)


def test_default_plan_is_the_identity():
    for cfg in (Config({}), Config({"model": {"type": "targetdiff"}}), Config({"data": {}}), Config({"data": {"train": {}}}),
                _cfg("- {type: featurize_ligand_fa, mode: add_aromatic}"), None):
        for split in ("train", "val"):
            plan = TrainingPlan.from_config(cfg, split)
            assert (plan.noise_std, plan.center) == (0.0, "protein") and plan.identity
    assert not TrainingPlan(0.1, "protein").identity and not TrainingPlan(0.0, "context").identity
    for fixture in ("targetdiff_train_tiny.yml", "targetdiff_T20.yml"):
        config, _ = C.load_config(os.path.join(ROOT, "tests", "fixtures", fixture))
        assert TrainingPlan.from_config(config, "train").identity and TrainingPlan.from_config(config, "val").identity
    config, _ = C.load_config(os.path.join(ROOT, "tests", "fixtures", "linker_targetdiff_train_tiny.yml"))
    assert TrainingPlan.from_config(config, "train") == TrainingPlan(0.1, "context")
    assert TrainingPlan.from_config(config, "val") == TrainingPlan(0.0, "context")


@pytest.mark.parametrize("text, match", [
    ("- {type: add_pos_noise, noise_std: 0.1, frame_mode: true}", "frame_mode"),
    ("- {type: add_pos_noise, noise_std: 0.1, graph_name: ligand}", "graph_name"),
    ("- {type: center_pos, center_flag: protein}\n- {type: add_pos_noise, noise_std: 0.1}", "order"),
    ("- {type: center_whole_pos}\n- {type: add_pos_noise, noise_std: 0.1}", "order"),
    ("- {type: center_pos, center_flag: protein, mask_flag: ctx_flag}", "center_flag"),
    ("- {type: center_pos, center_flag: ligand, mask_flag: gen_flag}", "center_flag"),
    ("- {type: center_pos, center_flag: whole}", "center_flag"),
    ("- {type: center_pos, center_flag: protein}\n- {type: center_whole_pos}", "two centring"),
    ("- {type: add_pos_noise, noise_std: 0.1}\n- {type: add_pos_noise, noise_std: 0.1}", "twice"),
    ("- {type: add_pos_noise, noise_std: -0.1}", "noise_std"),
    ("- {type: center_frame_pos, center_flag: protein}", "center_frame_pos"),
])
def test_unknown_combinations_raise(text, match):
    with pytest.raises(ValueError, match=match):
        TrainingPlan.from_config(_cfg(text), "train")
    with pytest.raises(ValueError, match="split"):
        TrainingPlan.from_config(_cfg(text), "test")


@needs_reference
def test_plan_of_all_shipped_diffusion_train_configs():
    seen = []
    for task in ("denovo", "linker", "frag", "scaffold", "sidechain"):
        for method in ("targetdiff", "diffbp", "diffsbdd"):
            config, _ = C.load_config(os.path.join(REFERENCE, "configs", task, "train", method + ".yml"))
            plan = TrainingPlan.from_config(config, "train")
            if task == "denovo":
                expect = (0.0, "whole") if method == "diffsbdd" else (0.1, "protein")
            else:
                expect = (0.1, "context")
            assert (plan.noise_std, plan.center) == expect, (task, method, plan)
            val = TrainingPlan.from_config(config, "val")
            assert val.noise_std == 0.0 or "val" in config.data, (task, method, val)
            seen.append(plan)
    assert len(seen) == 15


# ---- the tensor restatement against the reference's classes ---------------------------------------------------------------------------
def _one_graph(n_rec=37, n_lig=9, n_ctx=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    gen = torch.ones(n_lig, dtype=torch.bool)
    gen[:n_ctx] = False
    return {"protein_pos": torch.randn(n_rec, 3, generator=g) * 7.0 + torch.tensor([1.5, -2.0, 0.7]),
            "ligand_pos": torch.randn(n_lig, 3, generator=g) * 2.0 + torch.tensor([0.3, 0.9, -1.1]),
            "protein_element_batch": torch.zeros(n_rec, dtype=torch.long), "ligand_element_batch": torch.zeros(n_lig, dtype=torch.long),
            "ligand_gen_flag": gen[torch.randperm(n_lig, generator=g)], "num_graphs": 1}


@needs_reference
@pytest.mark.parametrize("case", ["protein", "context", "context_fallback", "ligand", "whole"])
def test_tensor_restatement_equals_the_reference_classes(case):
    """AddPosNoise then CenterPos / CenterWholePos of the reference on an attribute-dict stand-in for ``data``; eps replayed after
    torch.manual_seed.  Positions and translation bit-equal."""
    import importlib

    from oracle import ref_shim
    ref_shim.load_reference()
    importlib.import_module("repo.datasets.transforms.translation")
    T = importlib.import_module("repo.datasets.transforms._base").TRANSFORM_DICT
    center = case.split("_")[0]
    batch = _one_graph(n_ctx=0 if case == "context_fallback" else 4)
    data = ref_shim.AttrDict({"protein": {"pos": batch["protein_pos"].clone()},
                              "ligand": {"pos": batch["ligand_pos"].clone(), "ctx_flag": ~batch["ligand_gen_flag"]}})
    torch.manual_seed(1234)
    data = T["add_pos_noise"](noise_std=0.1)(data)
    if center == "whole":
        data = T["center_whole_pos"]()(data)
    else:
        data = T["center_pos"](center_flag="protein" if center == "protein" else "ligand", mask_flag="ctx_flag" if center == "context" else None)(data)
    torch.manual_seed(1234)
    eps = torch.randn_like(batch["protein_pos"])
    out = train_cli.apply_plan(batch, TrainingPlan(0.1, center), eps=eps)
    assert torch.equal(out["protein_pos"], data.protein.pos) and torch.equal(out["ligand_pos"], data.ligand.pos)
    assert torch.equal(out["translation"], data.protein.translation[:1]) and torch.equal(out["translation"], data.ligand.translation[:1])
    # eps drawn by apply_plan itself from the torch generator: the same draw
    torch.manual_seed(1234)
    own = train_cli.apply_plan(batch, TrainingPlan(0.1, center))
    assert torch.equal(own["protein_pos"], data.protein.pos)
    # out of place: the batch that came in still holds the stored coordinates
    fresh = _one_graph(n_ctx=0 if case == "context_fallback" else 4)
    assert own is not batch and torch.equal(batch["protein_pos"], fresh["protein_pos"]) and torch.equal(batch["ligand_pos"], fresh["ligand_pos"])


def test_restatement_on_a_batch_is_the_restatement_on_its_graphs():
    """three graphs (one without context atoms, one without ligand atoms): every graph of the batch gets the bits it gets alone; an empty
    centre set gives the zero vector"""
    cx = _complexes([(21, 6, 2), (30, 5, 0), (17, 0, 0), (0, 4, 1)], seed=5)
    cs = train_cli.ComplexSet(cx, center=False)
    for center in TrainingPlan.CENTERS:
        plan = TrainingPlan(0.1, center)
        batch = cs.collate([0, 1, 2, 3], ptrs=True)
        eps = torch.randn(batch["protein_pos"].shape[0], 3, generator=torch.Generator().manual_seed(3))
        out = train_cli.apply_plan(batch, plan, eps=eps)
        assert out["translation"].shape == (4, 3) and torch.isfinite(out["translation"]).all()
        r0 = l0 = 0
        for g in range(4):
            one = cs.collate([g])
            nr, nl = one["protein_pos"].shape[0], one["ligand_pos"].shape[0]
            alone = train_cli.apply_plan(one, plan, eps=eps[r0:r0 + nr])
            assert torch.equal(alone["protein_pos"], out["protein_pos"][r0:r0 + nr]), (center, g)
            assert torch.equal(alone["ligand_pos"], out["ligand_pos"][l0:l0 + nl]), (center, g)
            assert torch.equal(alone["translation"][0], out["translation"][g]), (center, g)
            r0, l0 = r0 + nr, l0 + nl
        if center in ("context", "ligand"):
            assert torch.equal(out["translation"][2], torch.zeros(3))          # no ligand atom: nothing to centre on
        if center == "protein":
            assert torch.equal(out["translation"][3], torch.zeros(3))          # no protein atom


def _complexes(sizes, seed=0, num_classes=13):
    """complexes of (protein atoms, ligand atoms, context atoms) -- the context atoms first"""
    rng = np.random.default_rng(seed)
    out = []
    for nr, nl, nc in sizes:
        pos, feat, aa = synthetic.make_pocket(rng, max(nr, 1), radius=6.0)
        out.append({"protein_pos": pos[:nr] + rng.standard_normal(3).astype(np.float32), "protein_atom_feature": feat[:nr],
                    "protein_aa_type": aa[:nr], "ligand_pos": (rng.standard_normal((nl, 3)) * 1.5 + 1.0).astype(np.float32),
                    "ligand_atom_type": rng.integers(0, num_classes, size=nl).astype(np.int64),
                    "ligand_gen_flag": np.arange(nl) >= nc})
    return out


# ---- identity ------------------------------------------------------------------------------------------------------------------------
def test_identity_plan_returns_the_batch_and_draws_nothing():
    cs = train_cli.ComplexSet(_complexes([(12, 5, 2), (9, 4, 1)]))
    batch = cs.collate([0, 1])
    torch.manual_seed(7)
    state = torch.get_rng_state()
    for plan in (TrainingPlan(), TrainingPlan(0.0, "protein"), TrainingPlan.from_config(Config({}), "train"), None):
        out = train_cli.apply_plan(batch, plan)
        assert out is batch and "translation" not in out
        assert out["protein_pos"] is batch["protein_pos"] and out["ligand_pos"] is batch["ligand_pos"]
    assert torch.equal(torch.get_rng_state(), state)
    # a plan without noise draws nothing either; a plan with noise draws exactly [n_rec, 3] normals
    train_cli.apply_plan(batch, TrainingPlan(0.0, "context"))
    assert torch.equal(torch.get_rng_state(), state)
    train_cli.apply_plan(batch, TrainingPlan(0.1, "context"))
    after = torch.get_rng_state()
    torch.set_rng_state(state)
    torch.randn(batch["protein_pos"].shape[0], 3)
    assert torch.equal(torch.get_rng_state(), after) and not torch.equal(after, state)
    # counter noise is made by GPU kernels
    with pytest.raises(ValueError, match="GPU"):
        train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), noise=N.training_noise(1, [0, 1], 1))
    with pytest.raises(ValueError, match="stream keys"):
        train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), noise=N.training_noise(1, [0, 1, 2], 1))
    with pytest.raises(ValueError, match="eps must be"):
        train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), eps=torch.zeros(3, 3))


def test_collate_hands_out_both_csrs_on_request():
    cs = train_cli.ComplexSet(_complexes([(12, 5, 2), (9, 4, 1), (7, 3, 0)]))
    plain, with_ptrs = cs.collate([2, 0]), cs.collate([2, 0], ptrs=True)
    assert set(with_ptrs) - set(plain) == {"protein_ptr", "ligand_ptr"}
    assert with_ptrs["protein_ptr"].dtype == torch.int32 and with_ptrs["protein_ptr"].tolist() == [0, 7, 19]
    assert with_ptrs["ligand_ptr"].dtype == torch.int32 and with_ptrs["ligand_ptr"].tolist() == [0, 3, 8]
    both = cs.collate([2, 0], example_ids=True, ptrs=True)
    assert set(both) - set(plain) == {"protein_ptr", "ligand_ptr", "example_index"} and both["ligand_ptr"].tolist() == [0, 3, 8]


# ---- through the driver --------------------------------------------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    """a model class in the registry's sense that keeps the batches it is called with"""
    seen = []

    def __init__(self, cfg):
        super().__init__()
        self.lin = torch.nn.Linear(3, 3)

    def forward(self, batch):
        type(self).seen.append((self.training, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}))
        out = self.lin(batch["ligand_pos"])
        return {"pos": (out ** 2).mean(), "atom": (out - 1.0).abs().mean()}, {}


def _driver_config(**run):
    config, _ = C.load_config(os.path.join(ROOT, "tests", "fixtures", "linker_targetdiff_train_tiny.yml"))
    config.model = {"type": "recorder_cpu"}
    config.train.batch_size = 3
    config.train.max_iters = 2
    config.eval.val_freq = 2
    return config


def _driver_sets():
    cx = _complexes([(20 + 3 * i, 6 + i % 3, 2 + i % 2) for i in range(8)], seed=2)
    return train_cli.ComplexSet(cx[:6]), train_cli.ComplexSet(cx[6:])


def test_run_applies_the_plans_of_the_config(tmp_path):
    """a linker-style config (add_pos_noise 0.1, context centring) through ``train_cli.run`` on a stub model: in every graph of every
    training batch the context atoms' mean is zero and the protein is noised, afresh at every iteration; validation batches are centred on
    the context but not noised.  ``data_transforms=False`` gives today's batches."""
    registry.register_model("recorder_cpu")(_Recorder)
    tr, va = _driver_sets()
    _Recorder.seen = []
    train_cli.run(_driver_config(), "rec", tr, va, torch.device("cpu"), str(tmp_path), log=lambda s: None)
    seen = _Recorder.seen
    train = [b for training, b in seen if training]
    val = [b for training, b in seen if not training]
    assert len(train) == 2 and len(val) == 1
    stored_rec = {}          # example -> stored protein positions, recognised by the atom count (all different)
    for cs in (tr, va):
        for i in range(len(cs)):
            b = cs.collate([i])
            stored_rec[(cs is va, b["protein_pos"].shape[0])] = (b["protein_pos"], b["ligand_pos"])
    noise_of = {}
    for is_val, batches in ((False, train), (True, val)):
        for it, b in enumerate(batches):
            assert b["translation"].shape == (b["num_graphs"], 3)
            for g in range(b["num_graphs"]):
                P = b["protein_pos"][b["protein_element_batch"] == g]
                L = b["ligand_pos"][b["ligand_element_batch"] == g]
                ctx = ~b["ligand_gen_flag"][b["ligand_element_batch"] == g]
                assert ctx.any() and not ctx.all()
                assert float(L[ctx].mean(0).abs().max()) <= 4 * 2.0 ** -24 * float(L.abs().max())
                P0, L0 = stored_rec[(is_val, P.shape[0])]
                # the ligand is shifted rigidly by the recorded translation
                assert torch.allclose(L0 - b["translation"][g], L, atol=1e-6)
                resid = P - (P0 - b["translation"][g])
                if is_val:
                    assert float(resid.abs().max()) <= 1e-6                    # not noised
                else:
                    assert 0.05 < float(resid.std()) < 0.2                      # N(0, 0.1^2) on every coordinate
                    noise_of.setdefault(P.shape[0], []).append(resid)
                assert float(P0.mean(0).abs().max()) < 1e-5 and float(P.mean(0).abs().max()) > 1e-2      # no longer the protein frame
    # 6 examples, batches of 3: both iterations together visit every example once; a second epoch shows fresh noise per visit
    _Recorder.seen = []
    cfg = _driver_config()
    cfg.train.max_iters = 4
    cfg.eval.val_freq = 100
    train_cli.run(cfg, "rec2", tr, va, torch.device("cpu"), str(tmp_path), log=lambda s: None)
    visits = {}
    for _, b in _Recorder.seen:
        for g in range(b["num_graphs"]):
            P = b["protein_pos"][b["protein_element_batch"] == g]
            visits.setdefault(P.shape[0], []).append(P + b["translation"][g])
    assert len(visits) == 6 and all(len(v) == 2 for v in visits.values())
    for a, b in visits.values():
        assert float((a - b).abs().max()) > 1e-2
    # the switch: the batches of today
    _Recorder.seen = []
    train_cli.run(_driver_config(), "rec3", tr, va, torch.device("cpu"), str(tmp_path), log=lambda s: None, data_transforms=False)
    assert len(_Recorder.seen) == 3
    for training, b in _Recorder.seen:
        assert "translation" not in b
        for g in range(b["num_graphs"]):
            P = b["protein_pos"][b["protein_element_batch"] == g]
            assert torch.equal(P, stored_rec[(not training, P.shape[0])][0])


def test_cli_switch_is_parsed():
    src = open(os.path.join(ROOT, "cbgbench_amd", "train_cli.py")).read()
    assert "--ignore_data_transforms" in src and "data_transforms=not args.ignore_data_transforms" in src


# ---- frame consistency with the sampling path -------------------------------------------------------------------------------------------
def test_training_frame_is_the_sampling_frame_on_context_tasks():
    """one complex with context atoms: the context coordinates ``apply_plan`` (sigma 0, 'context') hands the model in training are the
    ones ``priors.build_sampling_batch(center_on_context=True)`` hands it in sampling, and so are the protein's.  Both frames come from
    original coordinates of magnitude up to M by two subtractions of fp32 means (protein mean, then context mean): each mean is within a
    few roundings of M and each subtraction rounds once; 16 * 2^-24 * M (the kernel test's bound: 16 roundings relative to the largest
    magnitude) covers the difference of the two routes."""
    cx = _complexes([(41, 9, 4)], seed=9)[0]
    cx["protein_pos"] = cx["protein_pos"] + np.float32([12.0, -30.0, 7.5])
    cx["ligand_pos"] = cx["ligand_pos"] + np.float32([12.0, -30.0, 7.5])
    M = float(max(np.abs(cx["protein_pos"]).max(), np.abs(cx["ligand_pos"]).max()))
    bound = 16 * 2.0 ** -24 * M
    out = train_cli.apply_plan(train_cli.ComplexSet([cx]).collate([0]), TrainingPlan(0.0, "context"))
    ctx = ~torch.from_numpy(cx["ligand_gen_flag"])
    ps = priors.PocketSet([(cx["protein_pos"], cx["protein_atom_feature"], cx["protein_aa_type"])])
    sb = priors.build_sampling_batch(ps, 1, 13, n_lig=[[9]], context=[(cx["ligand_pos"][ctx.numpy()], cx["ligand_atom_type"][ctx.numpy()])],
                                     center_on_context=True, rng=np.random.default_rng(0))
    a, b = out["ligand_pos"][ctx], sb["ligand_pos"][sb["ligand_ctx_flag"]]
    worst = float((a - b).abs().max())
    print(f"context atoms: max |training frame - sampling frame| = {worst:.3e} (bound {bound:.3e})")
    assert a.shape == b.shape == (4, 3) and worst <= bound
    assert float((out["protein_pos"] - sb["protein_pos"]).abs().max()) <= bound
    assert float(a.mean(0).abs().max()) <= bound
    # the total shift is the same too: stored-frame shift + the protein mean the stored frame removed = the sampler's translation
    total = out["translation"][0] + torch.from_numpy(cx["protein_pos"]).mean(0)
    assert float((total - sb["ligand_translation"][0]).abs().max()) <= bound


# ---- addresses and moments of the protein draws ----------------------------------------------------------------------------------------
def _distinct(rows):
    return np.unique(rows, axis=0).shape[0] == rows.shape[0]


@pytest.mark.parametrize("model_type, C_", [("targetdiff", 13), ("diffbp", 13), ("diffsbdd", 8)])
def test_protein_draws_share_no_address(model_type, C_):
    assert N.TRAIN_PROTEIN_NORMAL == 12 and N.PURPOSE_NAMES[12] == "train_protein_normal" and len(N.PURPOSE_NAMES) == 13
    assert N.TRAIN_PROTEIN_NORMAL < N.PURPOSE_STRIDE
    rec_ptr, lig_ptr, T = np.array([0, 3, 3, 300]), np.array([0, 1, 6, 17]), 20
    tr_keys, va_keys = N.training_noise(2024, [7, 30, 3], 3).keys, N.validation_noise(2024, [7, 30, 3]).keys
    p_tr = N.protein_addresses(tr_keys, rec_ptr, 0)
    p_va = N.protein_addresses(va_keys, rec_ptr, N.PURPOSE_STRIDE)
    assert p_tr.shape == (300, 5) and _distinct(p_tr) and _distinct(p_va)
    assert set(p_tr[:, 3].tolist()) == {12} and set(p_va[:, 3].tolist()) == {28} and set(p_tr[:, 2].tolist()) == {0}
    everything = [p_tr, p_va, N.protein_addresses(tr_keys, rec_ptr, N.PURPOSE_STRIDE),      # (same keys under the validation base)
                  N.train_addresses(model_type, tr_keys, lig_ptr, T, C_), N.train_addresses(model_type, tr_keys, lig_ptr, T, C_, t_in=[0, 0, 0])[:0]]
    everything += N.validation_addresses(model_type, va_keys, lig_ptr, T, C_, 10)[:1]
    everything += N.validation_addresses(model_type, tr_keys, lig_ptr, T, C_, 10)[:1]
    assert _distinct(np.concatenate(everything))
    # all evaluation times of a validation call, and a training call whose times are all 0 (the protein draws' step)
    val_all = np.unique(np.concatenate(N.validation_addresses(model_type, va_keys, lig_ptr, T, C_, 10)), axis=0)
    assert _distinct(np.concatenate([p_va, val_all]))
    assert _distinct(np.concatenate([p_tr, N.train_addresses(model_type, tr_keys, lig_ptr, T, C_, t_in=[0, 0, 0])]))
    # the model is fill_model on the protein CSR at step 0
    assert np.array_equal(N.protein_draw_model(tr_keys, rec_ptr), N.fill_model(tr_keys, rec_ptr, 0, 12, 3, False))
    assert not np.array_equal(N.protein_draw_model(tr_keys, rec_ptr), N.protein_draw_model(tr_keys, rec_ptr, N.PURPOSE_STRIDE))


def test_protein_draws_of_an_example_do_not_depend_on_its_batch():
    """worlds 1 / 2 / 4 with batch sizes 8 / 4 / 2 through PositionedLoader: at every iteration the draws of every example are the same
    array, whichever rank's batch holds it and wherever in that batch"""
    n, seed = 21, 2022
    sizes = 5 + (np.arange(n) * 7) % 11              # protein atoms of example i
    def draws(world, bs, it):
        got = {}
        for r in range(world):
            ids = train_cli.PositionedLoader(n, bs, rank=r, world=world, seed=seed).batch(it)
            keys = N.training_noise(seed, ids, it).keys
            ptr = np.concatenate([[0], np.cumsum(sizes[ids])])
            eps = N.protein_draw_model(keys, ptr)
            for g, ex in enumerate(ids):
                got[ex] = eps[ptr[g]:ptr[g + 1]]
        return got
    for it in (1, 2, 3, 4):
        one = draws(1, 8, it)
        assert len(one) == 8
        for world, bs in ((2, 4), (4, 2)):
            other = draws(world, bs, it)
            assert sorted(other) == sorted(one)
            for ex in one:
                assert one[ex].shape == (sizes[ex], 3) and np.array_equal(one[ex], other[ex]), (it, world, ex)
    a, b = draws(1, 8, 1), draws(1, 8, 4)            # 21 examples, 8 per iteration: iteration 4 revisits examples of iteration 1
    again = sorted(set(a) & set(b))
    assert again and all(not np.array_equal(a[ex], b[ex]) for ex in again)


MOMENT_SEED = 20261019


def test_moments_of_the_protein_draws():
    """one committed seed, 2^15 atoms (64 examples of 512 protein atoms at iteration 1), numpy model: per component the mean within
    5 / sqrt(n) of 0 and the variance within 5 * sqrt(2 / n) of 1 (five standard errors of a unit normal's mean and variance)"""
    n = 1 << 15
    keys = N.training_noise(MOMENT_SEED, np.arange(64), 1).keys
    eps = N.protein_draw_model(keys, np.arange(65) * 512)
    assert eps.shape == (n, 3)
    for k in range(3):
        mean, var = float(eps[:, k].mean()), float(eps[:, k].var())
        print(f"component {k}: mean {mean:+.5f} (bound {5 / np.sqrt(n):.5f}), variance {var:.5f} (1 +- {5 * np.sqrt(2 / n):.5f})")
        assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1.0) <= 5 * np.sqrt(2.0 / n)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_train_transform", "cbgx_train_transform_rng")


def test_entries_are_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH, sources
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _native.EXPORTS and hasattr(lib, name)
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ENTRIES:
            assert f" {name}\n" in sym, (path, name)
    for xcheck in (False, True):
        assert any(os.path.basename(s) == "train_transform.hip" for s in sources(xcheck))
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    assert "#define CBGX_NOISE_TRAIN_PROTEIN_NORMAL 12" in hdr
    rng_h = open(os.path.join(ROOT, "cbgbench_amd", "csrc", "rng.h")).read()
    assert re.search(r"TRAIN_PROTEIN_NORMAL = 12,", rng_h)
    for k, mode in train_cli.CENTER_MODES.items():
        assert f"#define CBGX_CENTER_{k.upper()} {mode}" in hdr


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    one = ctypes.c_void_p(16)        # never dereferenced: argument checks come first
    def tape(x_rec=one, x_lig=one, rec_ptr=one, lig_ptr=one, ctx=None, B=1, n_rec=4, n_lig=2, sigma=0.1, mode=0, eps=one, ro=one,
             lo=one, co=one):
        return lib.cbgx_train_transform(x_rec, x_lig, rec_ptr, lig_ptr, ctx, B, n_rec, n_lig, sigma, mode, eps, ro, lo, co, None)
    def rng(keys=one, base=0, B=1, n_rec=4, n_lig=2, sigma=0.1, mode=0, ro=one, lo=one, co=one):
        return lib.cbgx_train_transform_rng(one, one, one, one, None, B, n_rec, n_lig, sigma, mode, keys, base, ro, lo, co, None)
    bad = [tape(ro=None), tape(lo=None), tape(co=None), tape(B=-1), tape(n_rec=-1), tape(n_lig=-1), tape(sigma=-0.1),
           tape(sigma=float("nan")), tape(mode=4), tape(mode=-1), tape(eps=None), tape(x_rec=None), tape(rec_ptr=None),
           rng(ro=None), rng(lo=None), rng(co=None), rng(B=-1), rng(sigma=-1.0), rng(mode=7), rng(base=8), rng(base=-16), rng(keys=None)]
    assert bad == [-1] * len(bad), bad
    assert tape(eps=None) == -1 and b"sigma == 0" in lib.cbgx_last_error()
    assert rng(base=12) == -1 and b"purpose_base" in lib.cbgx_last_error()
    # nothing to do: no graph, no launch, no error
    assert tape(B=0, n_rec=0, n_lig=0) == 0 and rng(B=0, n_rec=0, n_lig=0) == 0
