"""The per-visit decomposition choice of training batches (the reference's ``choose_ctx_gen``: ``priors.ContextChoice``, the
``ligand_gen_index`` packing of ``train_cli.ComplexSet``, ``train_cli.apply_plan(choose=...)``, purpose TRAIN_CHOOSE_CTX), the parts that
need no GPU: parsing, packing and collating against plain loops, the tensor restatement against the reference's own classes bit for bit,
the counter-mode choice and its address, the torch generator's state, ``sample_cli.load_context`` and the C ABI."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch
import yaml

import cbgbench_amd as C
from cbgbench_amd import _native, noise as N, sample_cli, synthetic, train_cli
from cbgbench_amd.config import Config
from cbgbench_amd.priors import ContextChoice, TrainingPlan
from tests.test_train_transform import LISTS, _cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle.ref_shim import REFERENCE_ROOT as REFERENCE     # where the reference tree lives when it is on this machine
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "repo")), reason="the reference tree is not on this machine")
CONTEXT_TASKS = ("linker", "frag", "scaffold", "sidechain")
METHODS = ("targetdiff", "diffbp", "diffsbdd")


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LISTS))
def test_choice_of_the_shipped_transform_lists(name):
    text, (std, center) = LISTS[name]
    expect = ContextChoice("uniform") if "choose_ctx_gen" in text else None
    assert ContextChoice.from_config(_cfg(text), "train") == expect
    assert ContextChoice.from_config(_cfg(text), "val") == expect          # no data.val: the train list's choice
    assert (expect is None) == name.startswith("denovo/fa_data_train")
    both = _cfg(text)
    both["data"]["val"] = {"transform": yaml.safe_load("- {type: choose_ctx_gen, sampling: fix_zero, ref_key: element}\n"
                                                        "- {type: center_pos, center_flag: ligand, mask_flag: ctx_flag}")}
    assert ContextChoice.from_config(both, "val") == ContextChoice("fix_zero") and ContextChoice.from_config(both, "train") == expect
    # the plan of the same list does not know about the choice
    plan = TrainingPlan.from_config(_cfg(text), "train")
    assert plan == TrainingPlan(std, center) and plan.identity == (std == 0.0 and center == "protein")
    assert not hasattr(plan, "sampling") and not hasattr(plan, "choose")


def test_no_list_no_choice():
    for cfg in (Config({}), Config({"model": {"type": "targetdiff"}}), Config({"data": {}}), Config({"data": {"train": {}}}), None,
                _cfg("- {type: featurize_ligand_fa, mode: add_aromatic}")):
        for split in ("train", "val", "test"):
            assert ContextChoice.from_config(cfg, split) is None
    config, _ = C.load_config(os.path.join(ROOT, "tests", "fixtures", "linker_targetdiff_train_tiny.yml"))
    assert ContextChoice.from_config(config, "train") == ContextChoice("uniform") == ContextChoice.from_config(config, "val")
    assert ContextChoice().sampling == "uniform" and ContextChoice("fix_zero") != ContextChoice("uniform")
    assert "fix_zero" in repr(ContextChoice("fix_zero"))


@pytest.mark.parametrize("text, match", [
    ("- {type: choose_ctx_gen, sampling: weighted}", "sampling"),
    ("- {type: center_pos, center_flag: ligand, mask_flag: ctx_flag}\n- {type: choose_ctx_gen}", "after the centring"),
    ("- {type: center_whole_pos}\n- {type: choose_ctx_gen, sampling: fix_zero}", "after the centring"),
    ("- {type: choose_ctx_gen}\n- {type: choose_ctx_gen}", "twice"),
])
def test_unknown_choices_raise(text, match):
    with pytest.raises(ValueError, match=match):
        ContextChoice.from_config(_cfg(text), "train")
    with pytest.raises(ValueError, match="split"):
        ContextChoice.from_config(_cfg(text), "eval")
    with pytest.raises(ValueError, match="sampling"):
        ContextChoice("first")


@needs_reference
def test_choice_of_all_shipped_context_configs():
    seen = 0
    for task in CONTEXT_TASKS:
        for method in METHODS:
            config, _ = C.load_config(os.path.join(REFERENCE, "configs", task, "train", method + ".yml"))
            assert ContextChoice.from_config(config, "train") == ContextChoice("uniform"), (task, method)
            assert ContextChoice.from_config(config, "val") == ContextChoice("uniform"), (task, method)
            test, _ = C.load_config(os.path.join(REFERENCE, "configs", task, "test", method + ".yml"))
            assert ContextChoice.from_config(test, "test") == ContextChoice("fix_zero"), (task, method)
            seen += 1
    assert seen == 12
    for method in METHODS:
        config, _ = C.load_config(os.path.join(REFERENCE, "configs", "denovo", "train", method + ".yml"))
        assert ContextChoice.from_config(config, "train") is None


# ---- packing and collating -------------------------------------------------------------------------------------------------------------
def _complex(rng, nr, nl, decs=None, flag=None, num_classes=13):
    pos, feat, aa = synthetic.make_pocket(rng, max(nr, 1), radius=6.0)
    c = {"protein_pos": pos[:nr] + rng.standard_normal(3).astype(np.float32), "protein_atom_feature": feat[:nr], "protein_aa_type": aa[:nr],
         "ligand_pos": (rng.standard_normal((nl, 3)) * 1.5 + 1.0).astype(np.float32),
         "ligand_atom_type": rng.integers(0, num_classes, size=nl).astype(np.int64)}
    if decs is not None:
        c["ligand_gen_index"] = decs
    if flag is not None:
        c["ligand_gen_flag"] = flag
    return c


def _ragged(seed=0):
    """K = 1, 2 and 7; an empty decomposition, a full one, indices in non-ascending order (with a repeat), lists / arrays / tensors"""
    rng = np.random.default_rng(seed)
    specs = [(9, 5, [np.array([3, 1, 1, 0])]),
             (12, 6, [[], list(range(6))]),
             (7, 8, [np.array([7, 0]), torch.tensor([2, 4, 6]), np.array([], dtype=np.int64), np.arange(8), np.array([5]),
                     np.array([1, 3, 5, 7], dtype=np.int32), [6, 5, 4]]),
             (10, 1, [np.array([0]), np.array([], dtype=np.int64)]),
             (5, 4, [np.array([2, 3])])]
    return [_complex(rng, nr, nl, decs) for nr, nl, decs in specs], [[np.asarray(d, dtype=np.int64).reshape(-1).tolist() for d in decs]
                                                                     for _, _, decs in specs]


def test_packing_is_the_three_level_csr_of_the_lists():
    cx, lists = _ragged()
    cs = train_cli.ComplexSet(cx)
    assert cs.has_dec and cs.gen_idx.dtype == torch.int32
    dec_ptr, gen_ptr, gen_idx = [0], [0], []
    for decs in lists:                                   # the plain loop
        for d in decs:
            gen_idx += d
            gen_ptr.append(len(gen_idx))
        dec_ptr.append(len(gen_ptr) - 1)
    assert cs.dec_ptr.tolist() == dec_ptr == [0, 1, 3, 10, 12, 13] and cs.gen_ptr.tolist() == gen_ptr and cs.gen_idx.tolist() == gen_idx
    # no ligand_gen_flag in the complexes: the set collates the flag of decomposition 0
    assert cs.has_gen
    flag = cs.collate(list(range(5)))["ligand_gen_flag"]
    want = []
    for c, decs in zip(cx, lists):
        f = [False] * c["ligand_pos"].shape[0]
        for a in decs[0]:
            f[a] = True
        want += f
    assert flag.dtype == torch.bool and flag.tolist() == want
    # complexes that carry their own flag keep it
    rng = np.random.default_rng(1)
    own = train_cli.ComplexSet([_complex(rng, 6, 4, [[0], [1, 2]], flag=np.array([False, False, True, True]))])
    assert own.collate([0])["ligand_gen_flag"].tolist() == [False, False, True, True]


@pytest.mark.parametrize("ids", [[0, 1, 2, 3, 4], [2], [4, 2, 0], [1, 1, 3], [3, 2, 2, 0]])
def test_collate_rebases_the_csrs_to_the_batch(ids):
    cx, lists = _ragged()
    cs = train_cli.ComplexSet(cx)
    b = cs.collate(ids, decomps=True)
    dec_ptr, gen_ptr, gen_idx = [0], [0], []
    for i in ids:
        for d in lists[i]:
            gen_idx += d
            gen_ptr.append(len(gen_idx))
        dec_ptr.append(len(gen_ptr) - 1)
    for key, want in (("ligand_dec_ptr", dec_ptr), ("ligand_gen_ptr", gen_ptr), ("ligand_gen_idx", gen_idx)):
        assert b[key].dtype == torch.int32 and b[key].device.type == "cpu" and b[key].tolist() == want, key
    plain = cs.collate(ids)
    assert set(b) - set(plain) == set(train_cli.DECOMP_KEYS)
    assert all(torch.equal(b[k], plain[k]) if torch.is_tensor(plain[k]) else b[k] == plain[k] for k in plain)
    both = cs.collate(ids, example_ids=True, ptrs=True, decomps=True)
    assert set(both) - set(plain) == set(train_cli.DECOMP_KEYS) | {"protein_ptr", "ligand_ptr", "example_index"}


def test_refusals_at_pack_time():
    rng = np.random.default_rng(2)
    ok = _complex(rng, 6, 4, [[0, 1]])
    with pytest.raises(ValueError, match="outside"):
        train_cli.ComplexSet([ok, _complex(rng, 6, 4, [[0], [1, 4]])])
    with pytest.raises(ValueError, match="outside"):
        train_cli.ComplexSet([_complex(rng, 6, 4, [[-1]])])
    with pytest.raises(ValueError, match="outside"):
        train_cli.ComplexSet([_complex(rng, 6, 0, [[0]])])
    with pytest.raises(ValueError, match="empty list"):
        train_cli.ComplexSet([ok, _complex(rng, 6, 4, [])])
    with pytest.raises(ValueError, match="do not carry"):
        train_cli.ComplexSet([ok, _complex(rng, 6, 4)])
    with pytest.raises(ValueError, match="integers"):
        train_cli.ComplexSet([_complex(rng, 6, 4, [np.array([0.0, 1.0])])])
    # legal: an empty decomposition, a full one, a ligand without atoms
    cs = train_cli.ComplexSet([_complex(rng, 6, 4, [[], [0, 1, 2, 3]]), _complex(rng, 6, 0, [[]])])
    assert cs.dec_ptr.tolist() == [0, 2, 3] and cs.gen_ptr.tolist() == [0, 0, 4, 4]


def test_a_set_without_the_key_collates_what_it_did():
    rng = np.random.default_rng(3)
    cx = [_complex(rng, 8 + i, 3 + i, flag=np.arange(3 + i) % 2 == 0) for i in range(4)]
    cs = train_cli.ComplexSet(cx)
    assert not cs.has_dec
    for kw in ({}, {"ptrs": True}, {"example_ids": True, "ptrs": True}):
        a, b = cs.collate([3, 0, 2], **kw), cs.collate([3, 0, 2], decomps=True, **kw)
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else np.array_equal(a[k], b[k]), k
    # and apply_plan with a choice changes nothing on it: the same object for the identity plan, the same bits otherwise
    batch = cs.collate([3, 0, 2], ptrs=True, decomps=True)
    assert train_cli.apply_plan(batch, TrainingPlan(), choose=ContextChoice("uniform")) is batch
    eps = torch.randn(batch["protein_pos"].shape[0], 3, generator=torch.Generator().manual_seed(0))
    a = train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), eps=eps)
    b = train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), eps=eps, choose=ContextChoice("uniform"))
    assert list(a) == list(b) and "decomposition" not in b
    assert all(torch.equal(a[k], b[k]) for k in ("protein_pos", "ligand_pos", "translation", "ligand_gen_flag"))
    with pytest.raises(ValueError, match="choice="):
        train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), eps=eps, choose=ContextChoice("uniform"), choice=[0, 0, 0])


def test_synthetic_decompositions_are_seeded_and_leave_the_complexes_alone():
    plain = train_cli.synthetic_complexes(4, 7, 13, n_rec_range=(10, 20), n_lig_range=(3, 9))
    a = train_cli.synthetic_complexes(4, 7, 13, n_rec_range=(10, 20), n_lig_range=(3, 9), decompositions=3)
    b = train_cli.synthetic_complexes(4, 7, 13, n_rec_range=(10, 20), n_lig_range=(3, 9), decompositions=3)
    for p, x, y in zip(plain, a, b):
        assert "ligand_gen_index" not in p and set(x) - set(p) == {"ligand_gen_index"}
        assert all(np.array_equal(p[k], x[k]) for k in p)
        m = p["ligand_pos"].shape[0]
        assert len(x["ligand_gen_index"]) == 3
        for d, e in zip(x["ligand_gen_index"], y["ligand_gen_index"]):
            assert np.array_equal(d, e) and d.dtype == np.int64 and 1 <= d.size < m and np.all(np.diff(d) > 0) and d.max() < m
    assert train_cli.ComplexSet(a).has_dec
    src = open(os.path.join(ROOT, "cbgbench_amd", "train_cli.py")).read()
    assert "--synthetic_decompositions" in src and "decompositions=max(args.synthetic_decompositions, 0)" in src
    assert synthetic.decompositions(np.random.default_rng(0), 1, 2)[0].tolist() == [0]
    assert synthetic.decompositions(np.random.default_rng(0), 0, 1)[0].size == 0


# ---- the flag of a pick ----------------------------------------------------------------------------------------------------------------
def test_flag_of_every_pick_is_the_scatter_of_its_list():
    cx, lists = _ragged()
    cs = train_cli.ComplexSet(cx)
    ids = [2, 0, 1, 3, 4]
    batch = cs.collate(ids, ptrs=True, decomps=True)
    K = [len(lists[i]) for i in ids]
    for trial in range(7):
        pick = [trial % k for k in K]
        for plan in (TrainingPlan(), TrainingPlan(0.0, "context"), TrainingPlan(0.0, "whole")):
            out = train_cli.apply_plan(batch, plan, choose=ContextChoice("uniform"), choice=pick)
            want = []
            for i, k in zip(ids, pick):
                f = [False] * cx[i]["ligand_pos"].shape[0]
                for a in lists[i][k]:
                    f[a] = True
                want += f
            assert out["ligand_gen_flag"].tolist() == want and out["decomposition"].tolist() == pick
            assert out["decomposition"].dtype == torch.int32 and out is not batch
            assert ("translation" in out) == (not plan.identity)
            if plan.identity:
                assert out["protein_pos"] is batch["protein_pos"] and out["ligand_pos"] is batch["ligand_pos"]
    # the centre of 'context' is the mean of the complement; with an empty complement (a full decomposition) the whole ligand
    out = train_cli.apply_plan(batch, TrainingPlan(0.0, "context"), choose=ContextChoice("fix_zero"))
    assert out["decomposition"].tolist() == [0] * 5
    l0 = 0
    for g, i in enumerate(ids):
        L = batch["ligand_pos"][l0:l0 + cx[i]["ligand_pos"].shape[0]]
        ctx = ~out["ligand_gen_flag"][l0:l0 + L.shape[0]]
        c = L[ctx].mean(0) if bool(ctx.any()) else L.mean(0)
        assert torch.equal(out["translation"][g], c), g
        l0 += L.shape[0]
    full = train_cli.apply_plan(batch, TrainingPlan(0.0, "context"), choose=ContextChoice("uniform"), choice=[3, 0, 1, 0, 0])
    assert bool(full["ligand_gen_flag"][:8].all()) and torch.equal(full["translation"][0], batch["ligand_pos"][:8].mean(0))
    # a replayed choice outside [0, K) is clamped into it
    out = train_cli.apply_plan(batch, TrainingPlan(0.0, "ligand"), choose=ContextChoice("uniform"), choice=[99, -4, 1, 7, 0])
    assert out["decomposition"].tolist() == [6, 0, 1, 1, 0]
    with pytest.raises(ValueError, match="choice must hold"):
        train_cli.apply_plan(batch, TrainingPlan(0.0, "ligand"), choose=ContextChoice("uniform"), choice=[0, 0])
    with pytest.raises(ValueError, match="GPU"):
        train_cli.apply_plan(batch, TrainingPlan(0.0, "ligand"), choose=ContextChoice("uniform"), noise=N.training_noise(1, ids, 1))


# ---- against the reference's classes ---------------------------------------------------------------------------------------------------
INTERLEAVED = [[1, 4, 7, 10], [0, 2, 3, 11], [5, 6], [2, 5, 8, 9, 10]]          # sidechain-style: pieces spread over the ligand


@needs_reference
@pytest.mark.parametrize("k", range(4))
def test_chosen_flag_and_frame_equal_the_reference_classes(k, monkeypatch):
    """ChooseCtxGen (random.choice patched to return k), AddPosNoise, CenterPos(ligand, ctx_flag) of the reference on an attribute-dict
    stand-in for ``data``; eps replayed after torch.manual_seed.  Flags equal, positions and translation bit-equal."""
    import importlib

    from oracle import ref_shim
    ref_shim.load_reference()
    importlib.import_module("repo.datasets.transforms.translation")
    importlib.import_module("repo.datasets.transforms.select")
    T = importlib.import_module("repo.datasets.transforms._base").TRANSFORM_DICT
    rng = np.random.default_rng(4)
    cx = _complex(rng, 37, 12, [np.array(d) for d in INTERLEAVED])
    nl = 12
    none = lambda: [torch.empty(0, dtype=torch.long) for _ in INTERLEAVED]
    lig = {"pos": torch.from_numpy(cx["ligand_pos"]).clone(), "element": torch.zeros(nl, dtype=torch.long),
           "gen_index": [torch.tensor(d) for d in INTERLEAVED],
           "ctx_index": [torch.tensor(sorted(set(range(nl)) - set(d))) for d in INTERLEAVED],
           "bond_index": torch.empty(2, 0, dtype=torch.long), "bond_type": torch.empty(0, dtype=torch.long)}
    for name in ("gen_bond_type", "gen_bond_index", "ctx_bond_type", "ctx_bond_index", "cross_bond_type", "cross_bond_index"):
        lig[name] = none()
    data = ref_shim.AttrDict({"protein": {"pos": torch.from_numpy(cx["protein_pos"]).clone()}, "ligand": lig})
    monkeypatch.setattr(random, "choice", lambda seq: seq[k])
    data = T["choose_ctx_gen"]()(data)
    torch.manual_seed(99)
    data = T["add_pos_noise"](noise_std=0.1)(data)
    data = T["center_pos"](center_flag="ligand", mask_flag="ctx_flag")(data)
    torch.manual_seed(99)
    eps = torch.randn(37, 3)
    batch = train_cli.ComplexSet([cx], center=False).collate([0], ptrs=True, decomps=True)
    out = train_cli.apply_plan_tensors(batch, TrainingPlan(0.1, "context"), eps, ContextChoice("uniform"), choice=[k])
    assert torch.equal(out["ligand_gen_flag"], data.ligand.gen_flag) and torch.equal(~out["ligand_gen_flag"], data.ligand.ctx_flag)
    assert out["ligand_gen_flag"].nonzero().flatten().tolist() == INTERLEAVED[k] and out["decomposition"].tolist() == [k]
    assert torch.equal(out["protein_pos"], data.protein.pos) and torch.equal(out["ligand_pos"], data.ligand.pos)
    assert torch.equal(out["translation"], data.ligand.translation[:1])
    via = train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), eps=eps, choose=ContextChoice("uniform"), choice=[k])
    assert all(torch.equal(via[key], out[key]) for key in ("ligand_gen_flag", "protein_pos", "ligand_pos", "translation", "decomposition"))


# ---- the counter-mode choice -------------------------------------------------------------------------------------------------------------
def _philox_scalar(counter, key):
    """Philox4x32-10 on Python integers, from its definition (Salmon et al., SC'11)"""
    c, k = [int(v) for v in counter], [int(v) for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_choose_model_is_the_scalar_formula():
    assert N.TRAIN_CHOOSE_CTX == 13 and N.TRAIN_PROTEIN_NORMAL < N.TRAIN_CHOOSE_CTX < N.PURPOSE_STRIDE
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    rng_h = open(os.path.join(ROOT, "cbgbench_amd", "csrc", "rng.h")).read()
    assert "#define CBGX_NOISE_TRAIN_CHOOSE_CTX 13" in hdr and re.search(r"TRAIN_CHOOSE_CTX = 13,", rng_h)
    assert _philox_scalar((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]          # the known answer tests/test_counter_noise.py uses
    ex = np.array([0, 1, 5, 77, 4000, 123456])
    K = np.array([1, 2, 3, 7, 0, 1000])
    for base, cn in ((0, N.training_noise(2022, ex, 9)), (N.PURPOSE_STRIDE, N.validation_noise(2022, ex))):
        got = N.choose_model(cn.keys, K, base)
        for g, key in enumerate(cn.keys.tolist()):
            w0 = _philox_scalar((0, 0, base + 13, 0), (key & 0xFFFFFFFF, key >> 32))[0]
            assert got[g] == ((w0 * int(K[g])) >> 32 if K[g] else -1), (base, g)
        assert got.dtype == np.int64 and got[0] == 0 and got[4] == -1 and np.all(got[K > 0] < K[K > 0])
        assert np.array_equal(N.choose_model(cn.keys, 3, base), N.choose_model(cn.keys, np.full(6, 3), base))
    # the formula of the training time, at another address
    cn = N.training_noise(2022, ex, 9)
    assert not np.array_equal(N.choose_model(cn.keys, 1000), N.train_times(cn.keys, 1000))


@pytest.mark.parametrize("model_type, C_", [("targetdiff", 13), ("diffbp", 13), ("diffsbdd", 8)])
def test_choice_shares_no_address(model_type, C_):
    rec_ptr, lig_ptr, T = np.array([0, 3, 3, 300]), np.array([0, 1, 6, 17]), 20
    tr_keys, va_keys = N.training_noise(2024, [7, 30, 3], 3).keys, N.validation_noise(2024, [7, 30, 3]).keys
    c_tr, c_va = N.choose_addresses(tr_keys, 0), N.choose_addresses(va_keys, N.PURPOSE_STRIDE)
    assert c_tr.shape == (3, 5) and set(c_tr[:, 3].tolist()) == {13} and set(c_va[:, 3].tolist()) == {29}
    assert not c_tr[:, 1:3].any() and not c_tr[:, 4].any()
    everything = [c_tr, c_va, N.choose_addresses(tr_keys, N.PURPOSE_STRIDE),
                  N.protein_addresses(tr_keys, rec_ptr, 0), N.protein_addresses(va_keys, rec_ptr, N.PURPOSE_STRIDE),
                  N.protein_addresses(tr_keys, rec_ptr, N.PURPOSE_STRIDE),
                  N.train_addresses(model_type, tr_keys, lig_ptr, T, C_),
                  np.unique(np.concatenate(N.validation_addresses(model_type, va_keys, lig_ptr, T, C_, 10)), axis=0)]
    rows = np.concatenate(everything)
    assert np.unique(rows, axis=0).shape[0] == rows.shape[0]
    # a training call whose times are all 0 (the choice's step), and a validation call under the training keys
    rows = np.concatenate([c_tr, N.choose_addresses(tr_keys, N.PURPOSE_STRIDE),
                           N.train_addresses(model_type, tr_keys, lig_ptr, T, C_, t_in=[0, 0, 0]),
                           np.unique(np.concatenate(N.validation_addresses(model_type, tr_keys, lig_ptr, T, C_, 10)), axis=0)])
    assert np.unique(rows, axis=0).shape[0] == rows.shape[0]


def test_counter_choice_is_uniform_and_visits_every_decomposition():
    """seed 2022, examples 0..1999 x iterations 1..16 (32 000 draws): every bin count for K = 2, 3, 7 lies within 4 standard deviations
    sqrt(n p (1 - p)) of n / K; examples 0..7 at K = 3 have each seen all three decompositions by iteration 12"""
    ex = np.arange(2000)
    keys = np.concatenate([N.training_noise(2022, ex, it).keys for it in range(1, 17)])
    n = keys.size
    assert n == 32000
    for K in (2, 3, 7):
        counts = np.bincount(N.choose_model(keys, K), minlength=K)
        sd = np.sqrt(n * (1.0 / K) * (1.0 - 1.0 / K))
        worst = float(np.abs(counts - n / K).max() / sd)
        print(f"K = {K}: bin counts {counts.tolist()}, worst deviation {worst:.2f} standard deviations")
        assert counts.sum() == n and counts.shape == (K,) and worst <= 4.0
    seen = [set() for _ in range(8)]
    for it in range(1, 13):
        for e, k in enumerate(N.choose_model(N.training_noise(2022, np.arange(8), it).keys, 3)):
            seen[e].add(int(k))
    assert all(s == {0, 1, 2} for s in seen), seen
    # an example's choice depends on (seed, example, iteration), not on its batch
    a = N.choose_model(N.training_noise(2022, [5, 9, 2], 4).keys, 7)
    b = N.choose_model(N.training_noise(2022, [2, 5], 4).keys, 7)
    assert a[0] == b[1] and a[2] == b[0]


# ---- the torch-mode choice -----------------------------------------------------------------------------------------------------------
def test_torch_generator_is_touched_only_by_a_uniform_choice():
    cx, lists = _ragged()
    cs = train_cli.ComplexSet(cx)
    ids = [2, 0, 1, 3]
    with_dec, without = cs.collate(ids, ptrs=True, decomps=True), cs.collate(ids, ptrs=True)
    torch.manual_seed(11)
    state = torch.get_rng_state()
    for plan in (TrainingPlan(), TrainingPlan(0.0, "context")):
        train_cli.apply_plan(without, plan, choose=ContextChoice("uniform"))              # nothing to choose from
        train_cli.apply_plan(with_dec, plan, choose=ContextChoice("fix_zero"))            # nothing to draw
        train_cli.apply_plan(with_dec, plan, choose=ContextChoice("uniform"), choice=[1, 0, 0, 1])      # a replay
        train_cli.apply_plan(with_dec, plan)                                              # no choice asked for
        assert torch.equal(torch.get_rng_state(), state)
    for plan in (TrainingPlan(), TrainingPlan(0.0, "context"), TrainingPlan(0.1, "context")):
        torch.set_rng_state(state)
        out = train_cli.apply_plan(with_dec, plan, choose=ContextChoice("uniform"))
        after = torch.get_rng_state()
        torch.set_rng_state(state)
        u = torch.rand(4, dtype=torch.float64)
        if plan.noise_std > 0:
            eps = torch.randn(with_dec["protein_pos"].shape[0], 3)
        assert torch.equal(torch.get_rng_state(), after) and not torch.equal(after, state)
        K = torch.tensor([7, 1, 2, 2])
        assert out["decomposition"].tolist() == torch.minimum((u * K).floor().long(), K - 1).tolist()
        if plan.noise_std > 0:
            again = train_cli.apply_plan(with_dec, plan, eps=eps, choose=ContextChoice("uniform"), choice=out["decomposition"])
            assert all(torch.equal(again[k], out[k]) for k in ("protein_pos", "ligand_pos", "translation", "ligand_gen_flag"))


# ---- through the driver (stub model, CPU) ----------------------------------------------------------------------------------------------
def test_run_chooses_per_visit_on_sets_with_decompositions(tmp_path):
    from tests.test_train_transform import _Recorder, _driver_config
    from cbgbench_amd import registry
    registry.register_model("recorder_cpu")(_Recorder)
    rng = np.random.default_rng(6)
    cx = [_complex(rng, 20 + 3 * i, 9, [np.array([0, 1, 2]), np.array([3, 4, 5]), np.array([6, 7, 8])]) for i in range(8)]
    tr, va = train_cli.ComplexSet(cx[:6]), train_cli.ComplexSet(cx[6:])
    cfg = _driver_config()
    cfg.train.max_iters = 8
    cfg.eval.val_freq = 8
    _Recorder.seen = []
    lines = []
    train_cli.run(cfg, "rec", tr, va, torch.device("cpu"), str(tmp_path), log=lines.append)
    assert any(s.startswith("[data]") and "ContextChoice(sampling='uniform')" in s for s in lines)
    logged = [s for s in lines if s.startswith("[choose]")]
    train = [b for training, b in _Recorder.seen if training]
    assert len(train) == 8 and len(logged) == 8
    picks = set()
    for b, line in zip(train, logged):
        assert str(b["decomposition"].tolist()) in line
        for g in range(b["num_graphs"]):
            k = int(b["decomposition"][g])
            flag = b["ligand_gen_flag"][b["ligand_element_batch"] == g]
            assert flag.nonzero().flatten().tolist() == [3 * k, 3 * k + 1, 3 * k + 2]
            L = b["ligand_pos"][b["ligand_element_batch"] == g]
            assert float(L[~flag].mean(0).abs().max()) <= 4 * 2.0 ** -24 * float(L.abs().max())       # centred on the chosen context
            picks.add(k)
    assert picks == {0, 1, 2}          # 24 uniform draws over three decompositions
    # without the transforms: decomposition 0 everywhere, no pick recorded
    _Recorder.seen = []
    train_cli.run(_driver_config(), "rec2", tr, va, torch.device("cpu"), str(tmp_path), log=lambda s: None, data_transforms=False)
    for _, b in _Recorder.seen:
        assert "decomposition" not in b and "ligand_dec_ptr" not in b
        for g in range(b["num_graphs"]):
            assert b["ligand_gen_flag"][b["ligand_element_batch"] == g].nonzero().flatten().tolist() == [0, 1, 2]


# ---- sample_cli ------------------------------------------------------------------------------------------------------------------------
def test_load_context_from_pockets_with_decompositions():
    rng = np.random.default_rng(8)
    pockets = []
    for nl, decs in ((7, [[1, 2], [0, 6, 3]]), (5, [[4, 0]]), (6, [[], [0, 1, 2, 3, 4, 5], [5]])):
        c = _complex(rng, 10, nl, [np.array(d, dtype=np.int64) for d in decs])
        pockets.append(c)
    def complement(p, k):
        keep = np.array([a not in set(np.asarray(p["ligand_gen_index"][k]).tolist()) for a in range(p["ligand_pos"].shape[0])], dtype=bool)
        return p["ligand_pos"][keep], p["ligand_atom_type"][keep]
    def same(ctx, ks):
        assert len(ctx) == len(pockets)
        for p, k, (pos, typ) in zip(pockets, ks, ctx):
            want_pos, want_typ = complement(p, k)
            assert pos.dtype == np.float32 and typ.dtype == np.int64 and np.array_equal(pos, want_pos) and np.array_equal(typ, want_typ)
    same(sample_cli.load_context(pockets, None), [0, 0, 0])
    same(sample_cli.load_context(pockets, None, choose=ContextChoice("fix_zero")), [0, 0, 0])
    same(sample_cli.load_context(pockets, None, choose=ContextChoice("fix_zero"), counter=True), [0, 0, 0])
    r = np.random.default_rng(5)
    ks = [int(r.integers(len(p["ligand_gen_index"]))) for p in pockets]
    same(sample_cli.load_context(pockets, None, choose=ContextChoice("uniform"), rng=np.random.default_rng(5)), ks)
    drawn = {tuple(int(np.random.default_rng(s).integers(3)) for _ in range(1)) for s in range(20)}
    assert len(drawn) > 1
    with pytest.raises(ValueError, match="counter"):
        sample_cli.load_context(pockets, None, choose=ContextChoice("uniform"), rng=np.random.default_rng(5), counter=True)
    with pytest.raises(ValueError, match="outside"):
        sample_cli.load_context([dict(pockets[1], ligand_gen_index=[np.array([5])])], None)
    # pockets with ligand_ctx_* behave as before, whatever else they carry; pockets with neither give None
    ctx_pockets = [dict(p, ligand_ctx_pos=p["ligand_pos"][:2], ligand_ctx_atom_type=p["ligand_atom_type"][:2]) for p in pockets]
    for kw in ({}, {"choose": ContextChoice("uniform"), "rng": np.random.default_rng(1)}):
        got = sample_cli.load_context(ctx_pockets, None, **kw)
        assert all(np.array_equal(pos, p["ligand_pos"][:2]) and np.array_equal(typ, p["ligand_atom_type"][:2])
                   for p, (pos, typ) in zip(pockets, got))
    bare = [{k: v for k, v in p.items() if not k.startswith("ligand")} for p in pockets]
    assert sample_cli.load_context(bare, None) is None and sample_cli.load_context(bare, None, choose=ContextChoice("fix_zero")) is None


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_train_transform_choose", "cbgx_train_transform_choose_rng")


def test_entries_are_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _native.EXPORTS and hasattr(lib, name)
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ENTRIES + ("cbgx_train_transform", "cbgx_train_transform_rng"):
            assert f" {name}\n" in sym, (path, name)
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in ENTRIES)
    # the old entries keep their arguments
    assert len(_native.EXPORTS["cbgx_train_transform"][1]) == 15 and len(_native.EXPORTS["cbgx_train_transform_rng"][1]) == 16
    assert len(_native.EXPORTS[ENTRIES[0]][1]) == 22 and len(_native.EXPORTS[ENTRIES[1]][1]) == 22


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    one = ctypes.c_void_p(16)        # never dereferenced: argument checks come first
    def tape(x_rec=one, x_lig=one, rec_ptr=one, lig_ptr=one, dec_ptr=one, gen_ptr=one, gen_idx=one, choice=one, B=1, n_rec=4, n_lig=2,
             n_dec=2, n_idx=3, sigma=0.1, mode=1, eps=one, ro=one, lo=one, co=one, fo=one, ko=one):
        return lib.cbgx_train_transform_choose(x_rec, x_lig, rec_ptr, lig_ptr, dec_ptr, gen_ptr, gen_idx, choice, B, n_rec, n_lig, n_dec,
                                               n_idx, sigma, mode, eps, ro, lo, co, fo, ko, None)
    def rng(keys=one, base=0, dec_ptr=one, gen_ptr=one, gen_idx=one, B=1, n_rec=4, n_lig=2, n_dec=2, n_idx=3, sigma=0.1, mode=1, ro=one,
            lo=one, co=one, fo=one, ko=one):
        return lib.cbgx_train_transform_choose_rng(one, one, one, one, dec_ptr, gen_ptr, gen_idx, B, n_rec, n_lig, n_dec, n_idx, sigma,
                                                   mode, keys, base, ro, lo, co, fo, ko, None)
    bad = [tape(ro=None), tape(lo=None), tape(co=None), tape(fo=None), tape(ko=None), tape(B=-1), tape(n_rec=-1), tape(n_lig=-1),
           tape(n_dec=-1), tape(n_idx=-1), tape(sigma=-0.1), tape(sigma=float("nan")), tape(mode=4), tape(mode=-1), tape(eps=None),
           tape(x_rec=None), tape(rec_ptr=None), tape(dec_ptr=None), tape(gen_ptr=None), tape(gen_idx=None),
           rng(ro=None), rng(lo=None), rng(co=None), rng(fo=None), rng(ko=None), rng(B=-1), rng(n_dec=-1), rng(n_idx=-1), rng(sigma=-1.0),
           rng(mode=7), rng(base=8), rng(base=-16), rng(keys=None), rng(dec_ptr=None), rng(gen_ptr=None), rng(gen_idx=None)]
    assert bad == [-1] * len(bad), bad
    assert tape(eps=None) == -1 and b"sigma == 0" in lib.cbgx_last_error()
    assert rng(base=13) == -1 and b"purpose_base" in lib.cbgx_last_error()
    assert tape(n_dec=-1) == -1 and b"n_dec" in lib.cbgx_last_error()
    # nothing to do: no graph, no launch, no error
    assert tape(B=0, n_rec=0, n_lig=0, n_dec=0, n_idx=0) == 0 and rng(B=0, n_rec=0, n_lig=0, n_dec=0, n_idx=0) == 0
