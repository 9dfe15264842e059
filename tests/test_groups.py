"""The functional-group report without a GPU: the plain-Python model of tests/groups_model.py (written from include/cbgx.h; its templates
parsed from their names) on hand cases whose groups are written out by hand, against networkx as a referee of every isomorphism decision,
on the seeded set the GPU tests run, under relabelling; the library's template table against the model's; the C entry's declaration,
binding and argument checks; the host helpers (totals, summary, the distances to a reference) and the place of the report in
cbgbench_amd/sample_reports.py.  Every comparison of counts is ``==`` on integers."""
import ctypes
import functools
import json
import os
import random
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import torch

from cbgbench_amd import _native, geometry as G, sample_reports
from cbgbench_amd.sample_reports import SampleReports
from tests import groups_model as GM
from tests.test_valence import collate, molecule_like, relabel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = GM.NAMES


# ---- molecules from SMILES: (n, pairs, z, order, aromatic) with pairs sorted, i < j, as tests/test_valence.py builds them --------------------
def mol(smiles, seed=None):
    """the graph of a SMILES string (the model's small parser); ``seed``: its atoms in a seeded random order"""
    labels, bonds = GM.parse(smiles)
    pairs = sorted(bonds)
    case = (len(labels), pairs, [z for z, _ in labels], [1 if bonds[e] == 4 else bonds[e] for e in pairs], [int(bonds[e] == 4) for e in pairs])
    if seed is None:
        return case
    perm = list(range(len(labels)))
    random.Random(seed).shuffle(perm)
    return relabel(case, perm)


def names_of(case):
    """the model's groups of one graph -> (sorted names, sorted sizes)"""
    _, _, _, groups = GM.graph_groups(*case)
    return sorted(G.group_name(cls) for _, _, _, cls in groups), sorted(len(atoms) for atoms, _, _, _ in groups)


# one molecule per class: the group with a methyl (or more) on it.  Nothing else in the molecule is a member
POSITIVE = ("Cc1ccccc1", "CC(=O)NC", "CC(=O)OC", "Cc1ccncc1", "Cc1ncc2nc[nH]c2n1", "CS(=O)(=O)NC", "COP(=O)(OC)OC", "COCOC", "Cc1cncnc1",
            "Cc1cn[nH]c1", "CP(=O)(OC)OC", "Cc1ccc2ccccc2c1", "Cc1ccsc1", "CN=C(C)NC", "CNC(=O)NC", "Cn1ccc(=O)[nH]c1=O", "Cc1ccc2ncccc2c1",
            "Cc1cscn1", "Cc1ccc2[nH]cnc2c1", "Cc1c[nH]cn1", "CN(=O)=O", "CC(=O)NOC", "CNC(=O)OC", "CS(=O)(=O)C", "Cc1ccc2[nH]ccc2c1")
#               name: (SMILES, the names of its groups sorted, their sizes sorted)
NEAR = {
    "pyrazine": ("Cc1cnccn1", ["other"], [6]),
    "pyridazine": ("Cc1ccnnc1", ["other"], [6]),
    "isoquinoline": ("Cc1ccc2cnccc2c1", ["other"], [10]),
    "isothiazole": ("Cc1ccsn1", ["other"], [5]),
    "isoindole": ("Cc1ccc2c[nH]cc2c1", ["other"], [9]),
    "benzofuran": ("Cc1ccc2occc2c1", ["other"], [9]),
    "thioamide": ("CC(=S)NC", ["other"], [3]),
    "carbonate": ("COC(=O)OC", ["other"], [4]),
    "sulfonate": ("CS(=O)(=O)OC", ["other"], [4]),
    "phosphinate": ("CP(C)(=O)OC", ["other"], [3]),
    "orthoester": ("COC(C)(OC)OC", ["other"], [4]),
    "aminal": ("CNCNC", ["other"], [3]),
    "enamide": ("NC(=O)C=C", ["other"], [5]),
    "vinyl": ("CC=C", ["other"], [2]),
    "epoxide": ("CC1CO1", ["other"], [3]),
    "phenol": ("Oc1ccccc1", [N[0], "other"], [1, 6]),
    "biphenyl": ("c1ccccc1-c1ccccc1", [N[0], N[0]], [6, 6]),
    "pyridone": ("O=c1cccc[nH]1", ["other"], [7]),
    "nitrous_ester": ("CN(=O)O", ["other"], [3]),
    "chain_of_11": ("C=CC=CC=CC=CC=CN", ["other"], [11]),
    "azulene": ("Cc1ccc2cccc2cc1", ["other"], [10]),
    "decapentaene": ("C=CC=CC=CC=CC=C", ["other"], [10]),
    "imidic_acid": ("CC(OC)=NC", ["other"], [3]),
    "carbodiimide": ("CN=C=NC", ["other"], [3]),
    "indazole": ("Cc1ccc2[nH]ncc2c1", ["other"], [9]),
    "ethers_and_halides": ("COCCN(C)CCF", ["other", "other", "other"], [1, 1, 1]),
    "ester_on_a_ring": ("COC(=O)c1ccccc1", [N[2], N[0]], [3, 6]),
    "two_amides": ("CC(=O)NCCNC(C)=O", [N[1], N[1]], [3, 3]),
    "explicit_hydrogens": ("[H]C([H])c1ccccc1", [N[0]], [6]),
}
HAND_CASES = tuple(mol(s, seed=k) for k, s in enumerate(POSITIVE)) + tuple(mol(s, seed=100 + k) for k, (s, _, _) in enumerate(NEAR.values()))


@pytest.mark.parametrize("k", range(GM.CLASSES))
def test_one_molecule_per_class(k):
    for case in (mol(POSITIVE[k]), mol(POSITIVE[k], seed=k), mol(POSITIVE[k], seed=50 + k)):
        names, sizes = names_of(case)
        assert names == [N[k]] and sizes == [len(GM.TEMPLATES[k][0])], (k, POSITIVE[k])
        row, atom_group, atom_class, _ = GM.graph_groups(*case)
        col = dict(zip(GM.COLUMNS, row))
        assert col["n_groups"] == col["n_named"] == col[f"fg_{k}"] == 1 and col["n_other"] == 0
        assert col["largest_group"] == col["n_group_atoms"] == sizes[0]
        members = [a for a in range(case[0]) if atom_group[a] >= 0]
        assert len(members) == sizes[0] and all(atom_group[a] == members[0] and atom_class[a] == k for a in members)
        assert all(atom_class[a] == GM.NO_GROUP for a in range(case[0]) if a not in members)


@pytest.mark.parametrize("name", list(NEAR))
def test_near_misses_are_other_or_split(name):
    smiles, names, sizes = NEAR[name]
    for case in (mol(smiles), mol(smiles, seed=7), mol(smiles, seed=8)):
        assert names_of(case) == (sorted(names), sizes), name


def test_the_order_of_groups_is_the_order_of_their_smallest_atoms():
    case = mol("Oc1ccccc1CC(=O)NC")                   # O 0; ring 1..6; amide 8, 9, 10
    row, atom_group, atom_class, groups = GM.graph_groups(*case)
    assert [G.group_name(g[3]) for g in groups] == ["other", N[0], N[1]] and [g[0][0] for g in groups] == [0, 1, 8]
    assert atom_group == [0] + [1] * 6 + [-1] + [8] * 3 + [-1] and atom_class == [25] + [0] * 6 + [254] + [1] * 3 + [254]
    assert G.group_names(atom_group, atom_class) == ["other", N[0], N[1]]
    assert row == [12, 12, 3, 10, 2, 6] + [1, 1] + [0] * 23 + [1]


# ---- the templates: the library's hand-written table is the model's parsed names ----------------------------------------------------------------
ELEMENTS = (1, 6, 7, 8, 9, 15, 16, 17)


def nx_graph(labels, bonds):
    g = nx.Graph()
    for a, lab in enumerate(labels):
        g.add_node(a, label=(int(lab[0]), bool(lab[1])))
    for (i, j), t in bonds.items():
        g.add_edge(i, j, type=int(t))
    return g


def nx_same(a, b):
    return nx.is_isomorphic(a, b, node_match=lambda u, v: u["label"] == v["label"], edge_match=lambda u, v: u["type"] == v["type"])


@functools.lru_cache(maxsize=None)
def library_templates():
    """the library's table (cbgx_ligand_groups_templates) as networkx graphs with the model's labels"""
    out = []
    for t in G.group_templates():
        out.append(nx_graph([(ELEMENTS[code], bool(aro)) for code, aro in t["labels"]], {(i, j): ty for i, j, ty in t["bonds"]}))
    return out


def test_library_table_is_the_parsed_vocabulary_and_pairwise_distinct():
    assert G.GROUP_NAMES == GM.NAMES and len(G.GROUP_NAMES) == G.GROUP_CLASSES == 25
    table, lib = G.group_templates(), library_templates()
    assert [t["name"] for t in table] == list(GM.NAMES)
    for k, (labels, bonds) in enumerate(GM.TEMPLATES):
        assert nx_same(lib[k], nx_graph(labels, bonds)), N[k]
        assert len(labels) <= GM.MAX_TEMPLATE_ATOMS and len(bonds) <= G.MAX_GROUP_TEMPLATE_BONDS
        # the matcher extends a connected partial map: every atom after the first has a bond to an earlier one
        assert all(any({i, j} == {a, b} for i, j, _ in table[k]["bonds"] for b in range(a)) for a in range(1, len(labels))), N[k]
    assert max(len(labels) for labels, _ in GM.TEMPLATES) == GM.MAX_TEMPLATE_ATOMS
    for a in range(25):
        for b in range(a + 1, 25):
            assert not nx_same(lib[a], lib[b]) and not GM.isomorphic(*GM.TEMPLATES[a], *GM.TEMPLATES[b]), (N[a], N[b])


def test_the_models_recursion_is_brute_force_on_small_graphs():
    rng = random.Random(5)
    small = [t for t in GM.TEMPLATES if len(t[0]) <= 6]
    for labels, bonds in small:
        perm = list(range(len(labels)))
        rng.shuffle(perm)
        moved = [None] * len(labels)
        for a, lab in enumerate(labels):
            moved[perm[a]] = lab
        moved_bonds = {(min(perm[i], perm[j]), max(perm[i], perm[j])): t for (i, j), t in bonds.items()}
        for other_labels, other_bonds in small:
            want = GM.isomorphic_by_permutations(other_labels, other_bonds, moved, moved_bonds)
            assert GM.isomorphic(other_labels, other_bonds, moved, moved_bonds) == want
            assert want == (other_labels is labels)


# ---- the seeded set of the GPU tests -----------------------------------------------------------------------------------------------------------
# near misses that pass every cheap filter (atom count, bond count, sorted labels of some template) ...
HARD = ("Cc1cnccn1", "Cc1ccnnc1", "Cc1ccc2cnccc2c1", "Cc1ccsn1", "Cc1ccc2c[nH]cc2c1", "Cc1ccc2cccc2cc1", "CN(=O)O", "CC(OC)=NC", "CN=C=NC",
        "CN=C(NC)OC", "CN=C(OC)OC", "CC(OC)=NOC", "CS(OC)(=NC)=O", "Cc1ccc2[nH]ncc2c1", "Cc1ncc2c[nH]nc2n1", "Cn1cc(=O)cc(=O)[nH]1")
# ... and ones that do not
SOFT = ("CC(=S)NC", "COC(=O)OC", "CS(=O)(=O)OC", "CP(C)(=O)OC", "COC(C)(OC)OC", "CNCNC", "CC(=O)C=C", "CC=C", "CC1CO1", "CO", "CCl",
        "Cc1ccc2occc2c1", "CC#N", "C=CC=CC=CC=CC=CN")
SEED, N_SEEDED = 2025, 480


def decorated(rng):
    """a scaffold -- a random tree of saturated carbons, one time in four a molecule-like graph of tests/test_valence.py -- with two to five
    decorations on single bonds: template groups (half of them), hard and soft near misses; atoms in a random order"""
    if rng.random() < 0.25:
        n, pairs, z, order, aromatic = molecule_like(rng)
        pairs = list(pairs)
        anchors = [a for a in range(n) if z[a] == 6]
    else:
        n = rng.randint(2, 8)
        pairs = [(rng.randrange(a), a) for a in range(1, n)]
        z, order, aromatic = [6] * n, [1] * len(pairs), [0] * len(pairs)
        anchors = list(range(n))
    z, order, aromatic = list(z), list(order), list(aromatic)
    for _ in range(rng.randint(2, 5)):
        roll = rng.random()
        smiles = rng.choice(POSITIVE) if roll < 0.5 else rng.choice(HARD) if roll < 0.8 else rng.choice(SOFT)
        labels, bonds = GM.parse(smiles)
        pairs.append((rng.choice(anchors), n))
        order.append(1)
        aromatic.append(0)
        for (i, j), t in bonds.items():
            pairs.append((n + i, n + j))
            order.append(1 if t == 4 else t)
            aromatic.append(int(t == 4))
        z += [zz for zz, _ in labels]
        n += len(labels)
    rows = sorted(zip(pairs, order, aromatic))
    case = (n, [e for e, _, _ in rows], z, [o for _, o, _ in rows], [a for _, _, a in rows])
    perm = list(range(n))
    rng.shuffle(perm)
    return relabel(case, perm)


@functools.lru_cache(maxsize=None)
def seeded_set():
    rng = random.Random(SEED)
    return tuple(decorated(rng) for _ in range(N_SEEDED))


@functools.lru_cache(maxsize=None)
def seeded_model():
    """(the entry's arguments, the model's outputs, the model's groups per graph) of the seeded set as one batch: computed once, shared by
    the CPU and the GPU tests, never modified"""
    cases = list(seeded_set())
    args = collate(cases)
    return args, GM.batch_groups(*args), tuple(GM.graph_groups(*case)[3] for case in cases)


def passes_the_cheap_filters(labels, bonds):
    return any(len(labels) == len(tl) and len(bonds) == len(tb) and sorted(labels) == sorted(tl) for tl, tb in GM.TEMPLATES)


def test_seeded_set_covers_every_class_and_hard_near_misses():
    args, (_, atom_class, out), groups = seeded_model()
    # before anything else: the three conditions the set was seeded for
    assert all(int(out[:, 6 + k].sum()) >= 20 for k in range(GM.CLASSES + 1)), out[:, 6:32].sum(0).tolist()
    others = [(labels, bonds) for per_graph in groups for _, labels, bonds, cls in per_graph if cls == GM.OTHER]
    hard = sum(passes_the_cheap_filters(labels, bonds) for labels, bonds in others)
    assert 10 * hard >= len(others), (hard, len(others))
    assert (out[:, -1] == 0).all()
    assert out.shape == (N_SEEDED, GM.COLS) and len(others) == int(out[:, 31].sum())
    assert (out[:, 2] == out[:, 6:32].sum(1)).all() and (out[:, 4] == out[:, 6:31].sum(1)).all()
    assert int((atom_class < GM.CLASSES).sum()) + int((atom_class == GM.OTHER).sum()) == int(out[:, 3].sum())


def referee(labels, bonds):
    """the class by networkx: the library template of the same size that is isomorphic, node and edge labels matched"""
    if len(labels) > GM.MAX_TEMPLATE_ATOMS:
        return GM.OTHER
    g = nx_graph(labels, bonds)
    hits = [k for k, t in enumerate(library_templates()) if t.number_of_nodes() == len(labels) and nx_same(g, t)]
    assert len(hits) <= 1
    return hits[0] if hits else GM.OTHER


def test_networkx_agrees_on_every_group_of_the_hand_cases_and_of_the_seeded_set():
    per_graph = [GM.graph_groups(*case)[3] for case in HAND_CASES] + list(seeded_model()[2])
    n = 0
    for groups in per_graph:
        for _, labels, bonds, cls in groups:
            assert cls == referee(labels, bonds), (labels, bonds)
            n += 1
    assert n > 2000


def test_relabelling_permutes_the_atoms_and_keeps_the_counts():
    rng = random.Random(3)
    for case in HAND_CASES + seeded_set()[:60]:
        n = case[0]
        perm = list(range(n))
        rng.shuffle(perm)
        row, _, atom_class, _ = GM.graph_groups(*case)
        row2, atom_group2, atom_class2, _ = GM.graph_groups(*relabel(case, perm))
        assert row2 == row
        assert [atom_class2[perm[a]] for a in range(n)] == atom_class
        assert all((atom_group2[a] < 0) == (atom_class2[a] == GM.NO_GROUP) for a in range(n))


def test_batch_model_status_and_clamping():
    cases = [mol("Cc1ccccc1"), mol(""), mol("CC(=O)NC")]
    args = collate(cases)
    grp, cls, out = GM.batch_groups(*args)
    assert out[:, -1].tolist() == [0, 0, 0] and out[:, 2].tolist() == [1, 0, 1] and out[1].tolist() == [0] * 33
    assert grp.tolist() == [-1] + [1] * 6 + [-1, 1, 1, 1, -1] and cls.tolist() == [254] + [0] * 6 + [254, 1, 1, 1, 254]
    aro = args[6].copy()
    aro[0] = 255
    g2, c2, o2 = GM.batch_groups(*args[:6], aro)
    assert o2[:, -1].tolist() == [GM.NO_AROMATIC, 0, 0] and o2[0].tolist() == [7, 7] + [-1] * 30 + [8]
    assert g2[:7].tolist() == [-2] * 7 and c2[:7].tolist() == [255] * 7 and g2[7:].tolist() == grp[7:].tolist()
    order = args[5].copy()
    order[8] = 4
    assert GM.batch_groups(*args[:5], order, args[6])[2][:, -1].tolist() == [0, 0, GM.BAD_BONDS]
    none = GM.batch_groups(*args[:6], None)                   # no aromatic bytes: the ring is six carbons on single bonds, no members
    assert none[2][:, 2].tolist() == [0, 0, 1] and none[0][:7].tolist() == [-1] * 7


# ---- host helpers ------------------------------------------------------------------------------------------------------------------------------
def hand_counts():
    rows = [GM.graph_groups(*mol(s))[0] + [0] for s in ("Oc1ccccc1CC(=O)NC", "CCO", "CCC", "Cc1ccccc1-c1ccccc1")]
    return np.array(rows + [[300, 310] + [-1] * 30 + [1]], np.int64)


def test_summary_arithmetic_and_split_totals():
    assert G.GROUP_GRAPH_COLUMNS == GM.COLUMNS and len(G.GROUP_GRAPH_COLUMNS) == GM.COLS == 33
    gc = hand_counts()
    totals = G.group_totals(gc)
    c = dict(zip(G.GROUP_COUNT_KEYS, totals))
    assert (c["n_mol"], c["n_mol_evaluated"], c["n_mol_over_limit"]) == (5, 4, 1)
    assert (c["n_atoms"], c["n_bonds"], c["n_groups"], c["n_group_atoms"], c["n_named"]) == (12 + 3 + 3 + 13, 12 + 2 + 2 + 14, 6, 10 + 1 + 12, 4)
    assert c["n_fg_0"] == 3 and c["n_fg_1"] == 1 and c["n_other"] == 2 and c["n_mol_with_named_group"] == 2
    assert sum(c[f"n_fg_{k}"] for k in range(25)) == c["n_named"] and len(totals) == len(G.GROUP_COUNT_KEYS) == 35
    s = G.summarise_groups(gc)
    assert s == G.summarise_group_totals(totals) and set(s) == set(G.GROUP_RATIOS) | {"fg_ratio", "fg_distribution", "counts"}
    assert s["fg_ratio"][N[0]] == 3 / 4 and s["fg_ratio"][N[1]] == 1 / 4 and s["fg_ratio"][N[2]] == 0.0 and list(s["fg_ratio"]) == list(N)
    assert s["fg_distribution"][N[0]] == 3 / 4 and s["fg_distribution"][N[1]] == 1 / 4 and sum(s["fg_distribution"].values()) == 1.0
    assert s["groups_per_mol"] == 6 / 4 and s["named_group_ratio"] == 4 / 6 and s["mol_with_named_group_ratio"] == 2 / 4
    assert s["group_atom_ratio"] == 23 / 31 and s["counts"] == c
    # ranks add totals up: any split gives the whole
    for cut in range(6):
        assert [a + b for a, b in zip(G.group_totals(gc[:cut]), G.group_totals(gc[cut:]))] == totals
    empty = G.summarise_groups(np.zeros((0, 33)))
    assert all(np.isnan(empty[k]) for k in G.GROUP_RATIOS) and empty["counts"]["n_mol"] == 0
    assert all(v == 0.0 for v in empty["fg_distribution"].values()) and all(np.isnan(v) for v in empty["fg_ratio"].values())
    assert len(G.COUNT_REPORTS) == 5 and "groups" not in [r.name for r in G.COUNT_REPORTS]


def reference_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "functional_groups_reference.json")) as f:
        return json.load(f)


def test_groups_against_the_published_reference():
    ref = reference_fixture()
    assert list(ref["ratio"]) == list(ref["distribution"]) == list(N)
    s = G.summarise_groups(hand_counts())
    got = G.groups_against(s, ref)
    ratio = np.array([ref["ratio"][k] for k in N])
    mine = np.array([s["fg_ratio"][k] for k in N])
    assert got["MAE_fg"] == float(np.abs(ratio - mine).mean()) and got["not_evaluated"] == {}
    assert got["JSD_fg"] == G.distribution_jsd([s["fg_distribution"][k] for k in N], [ref["distribution"][k] for k in N])
    # vectors in the order of the vocabulary are the dicts
    vectors = {"ratio": [ref["ratio"][k] for k in N], "distribution": np.array([ref["distribution"][k] for k in N])}
    assert G.groups_against(s, vectors) == got
    # a job that is the reference has distance 0
    same = dict(s, fg_ratio=ref["ratio"], fg_distribution=ref["distribution"])
    again = G.groups_against(same, ref)
    assert again["MAE_fg"] == 0.0 and again["JSD_fg"] == 0.0
    with pytest.raises(ValueError, match="24 values"):
        G.groups_against(s, {"ratio": vectors["ratio"][:24], "distribution": vectors["distribution"]})
    with pytest.raises(ValueError, match="lacks"):
        G.groups_against(s, {"ratio": {k: 0.0 for k in N[:-1]}, "distribution": ref["distribution"]})


def test_jsd_is_scipys_on_the_reference():
    spatial = pytest.importorskip("scipy.spatial")
    ref = reference_fixture()
    q = np.array([ref["distribution"][k] for k in N])
    rng = np.random.default_rng(0)
    sets = [G.summarise_groups(hand_counts()), G.summarise_groups(seeded_model()[1][2])]
    vectors = [[s["fg_distribution"][k] for k in N] for s in sets] + [rng.random(25) for _ in range(5)]
    for s in sets:
        assert abs(G.groups_against(s, ref)["JSD_fg"] - spatial.distance.jensenshannon([s["fg_distribution"][k] for k in N], q)) <= 1e-12
    for p in vectors:
        assert abs(G.distribution_jsd(p, q) - spatial.distance.jensenshannon(np.asarray(p), q)) <= 1e-12


def test_zero_sums_have_no_distance():
    ref = reference_fixture()
    none_named = G.summarise_groups([GM.graph_groups(*mol("CCO"))[0] + [0]])
    got = G.groups_against(none_named, ref)
    assert got["JSD_fg"] is None and "no named group" in got["not_evaluated"]["JSD_fg"]
    assert got["MAE_fg"] == float(np.mean([ref["ratio"][k] for k in N]))
    s = G.summarise_groups(hand_counts())
    got = G.groups_against(s, {"ratio": ref["ratio"], "distribution": [0.0] * 25})
    assert got["JSD_fg"] is None and "reference" in got["not_evaluated"]["JSD_fg"] and got["MAE_fg"] is not None
    nothing = G.groups_against(G.summarise_groups(np.zeros((0, 33))), ref)
    assert nothing["MAE_fg"] is None and nothing["JSD_fg"] is None and set(nothing["not_evaluated"]) == {"MAE_fg", "JSD_fg"}


# ---- the reports' host side -------------------------------------------------------------------------------------------------------------------
def fake_reports(calls):
    """stand-ins for geometry.batch_*: they count their calls, check what they are handed and return CPU tensors for two graphs of 4 + 1
    atoms and three bonds (acetamide-like N C O C: one amide; one carbon over a limit)"""
    i32, u8 = torch.int32, torch.uint8
    amide = [4, 3, 1, 3, 1, 3] + [0, 1] + [0] * 23 + [0, 0]
    made = {
        "bonds": {"bond_index": torch.tensor([[0, 1, 1], [1, 2, 3]], dtype=i32), "bond_order": torch.tensor([1, 2, 1], dtype=u8),
                  "bond_length": torch.tensor([1.3, 1.2, 1.5], dtype=torch.float64), "bond_graph": torch.tensor([0, 0, 0]),
                  "fragment": torch.zeros(5, dtype=i32), "graph_counts": torch.tensor([[4, 3, 4, 1, 4, 0], [1, 0, 0, 1, 1, 0]], dtype=i32)},
        "rings": {"atom_ring_min": torch.zeros(5, dtype=u8), "graph_counts": torch.zeros(2, 13, dtype=i32)},
        "aromatic": {"aromatic_atom": torch.zeros(5, dtype=torch.bool), "in_closure": torch.zeros(5, dtype=torch.bool),
                     "aromatic_bond": torch.zeros(3, dtype=torch.bool), "bond_type": torch.tensor([1, 2, 1], dtype=u8),
                     "graph_counts": torch.zeros(2, 10, dtype=i32)},
        "valence": {"implicit_h": torch.zeros(5, dtype=u8), "atom_flags": torch.zeros(5, dtype=u8), "bond_kekule": torch.tensor([1, 2, 1], dtype=u8),
                    "graph_counts": torch.zeros(2, 22, dtype=i32)},
        "groups": {"atom_group": torch.tensor([0, 0, 0, -1, -2], dtype=i32), "atom_class": torch.tensor([1, 1, 1, 254, 255], dtype=u8),
                   "graph_counts": torch.tensor([amide, [1, 0] + [-1] * 30 + [1]], dtype=i32)}}

    def fake(name, wants):
        def run(batch, x, c, lig_batch, mode, **deps):
            calls.append((name, tuple(sorted(k for k, v in deps.items() if v is not None))))
            assert all(deps[k] is made[k] for k in deps if deps[k] is not None) and set(deps) <= set(wants)
            return made[name]
        return run

    return {"batch_bonds": fake("bonds", ()), "batch_rings": fake("rings", ("bonds",)), "batch_aromatic": fake("aromatic", ("bonds", "rings")),
            "batch_valence": fake("valence", ("bonds", "aromatic")), "batch_groups": fake("groups", ("bonds", "aromatic"))}


GROUP_FIELDS = ("atom_group", "atom_class", "groups", "n_groups", "fg_counts", "groups_status")


def test_groups_alone_computes_its_dependencies_once_and_writes_none(monkeypatch, tmp_path, capsys):
    assert sample_reports.LATE == ("groups",) and sample_reports.EXTRA == ("interactions",) and sample_reports.ORDER[-1] == "valence"
    assert sample_reports.needs("groups", "add_aromatic") == ("bonds", "aromatic") and sample_reports.needs("groups", "basic") == ("bonds",)
    calls = []
    for name, fn in fake_reports(calls).items():
        monkeypatch.setattr(G, name, fn)
    state = (torch.zeros(5, 3), torch.zeros(5, dtype=torch.long), torch.tensor([0, 0, 0, 0, 1]))
    r = SampleReports(("groups",))
    ev = r.evaluate(torch.device("cpu"), state, {}, 2, "add_aromatic")
    assert calls == [("bonds", ()), ("rings", ("bonds",)), ("aromatic", ("bonds", "rings")), ("groups", ("aromatic", "bonds"))]
    assert sorted(ev) == ["groups"] and sorted(r.seconds) == ["groups"] and r.seconds["groups"] > 0.0
    # with the 8-type vocabulary there are no aromatic flags: the bond list only
    del calls[:]
    SampleReports(("groups",)).evaluate(torch.device("cpu"), state, {}, 2, "basic")
    assert calls == [("bonds", ()), ("groups", ("bonds",))]
    # beside every other flag it comes last, and everything is still made once
    del calls[:]
    every = SampleReports(("groups", "valence", "aromatic", "rings", "bonds", "sdf"))
    ev_all = every.evaluate(torch.device("cpu"), state, {}, 2, "add_aromatic")
    assert [n for n, _ in calls] == ["bonds", "rings", "aromatic", "valence", "groups"] and list(every.seconds)[-1] == "groups"
    assert list(ev_all) == ["bonds", "rings", "aromatic", "valence", "groups"]

    smp = [{"pos": torch.zeros(4, 3), "atom": [7, 6, 8, 6]}, {"pos": torch.zeros(1, 3), "atom": [6]}]
    r.annotate(smp, ev)
    assert all(sorted(s) == sorted(("pos", "atom") + GROUP_FIELDS) for s in smp)
    s0, s1 = smp
    assert s0["atom_group"].tolist() == [0, 0, 0, -1] and s0["atom_class"].tolist() == [1, 1, 1, 254] and s0["groups"] == ["NC=O"]
    assert s0["n_groups"] == 1 and s0["groups_status"] == 0 and s0["fg_counts"].tolist() == [0, 1] + [0] * 24
    assert s0["fg_counts"].dtype == torch.int64 and s0["fg_counts"].shape == (26,)
    assert s1["groups"] == [] and s1["groups_status"] == 1 and s1["n_groups"] == -1 and s1["atom_group"].tolist() == [-2]
    rec = r.pocket_counts(ev, 0, 2)
    assert list(rec) == ["groups"] and rec["groups"] == G.summarise_groups(ev["groups"]["graph_counts"])["counts"]
    assert rec["groups"]["n_mol_over_limit"] == 1 and rec["groups"]["n_fg_1"] == 1
    assert list(every.pocket_counts(ev_all, 0, 2))[-1] == "groups"
    r.finish(str(tmp_path), 0, torch.device("cpu"))
    with open(tmp_path / "groups_summary.json") as f:
        assert f.read() == json.dumps(G.summarise_groups(ev["groups"]["graph_counts"]), indent=1, sort_keys=True)
    assert os.listdir(tmp_path) == ["groups_summary.json"]
    line = capsys.readouterr().out
    assert line.startswith("groups: groups_per_mol 1.0000, named_group_ratio 1.0000, mol_with_named_group_ratio 1.0000, group_atom_ratio 0.7500")
    assert "most frequent: NC=O 1, c1ccccc1 0, O=CO 0" in line and "1 of 2 molecules evaluated, n_mol_over_limit 1" in line


def test_groups_reference_joins_the_summary(monkeypatch, tmp_path):
    for name, fn in fake_reports([]).items():
        monkeypatch.setattr(G, name, fn)
    ref = reference_fixture()
    paths = [str(tmp_path / "ref.npz"), str(tmp_path / "ref.pt")]
    np.savez(paths[0], ratio=[ref["ratio"][k] for k in N], distribution=[ref["distribution"][k] for k in N])
    torch.save({"ratio": ref["ratio"], "distribution": ref["distribution"]}, paths[1])
    state = (torch.zeros(5, 3), torch.zeros(5, dtype=torch.long), torch.tensor([0, 0, 0, 0, 1]))
    summaries = []
    for k, path in enumerate(paths):
        r = SampleReports(("groups",), groups_reference=path)
        ev = r.evaluate(torch.device("cpu"), state, {}, 2, "basic")
        r.pocket_counts(ev, 0, 2)
        out = tmp_path / f"out{k}"
        out.mkdir()
        r.finish(str(out), 0, torch.device("cpu"))
        with open(out / "groups_summary.json") as f:
            summaries.append(json.load(f))
    want = G.summarise_groups(ev["groups"]["graph_counts"])
    want.update(G.groups_against(want, ref))
    assert summaries[0] == summaries[1] == json.loads(json.dumps(want)) and summaries[0]["MAE_fg"] > 0 and summaries[0]["JSD_fg"] > 0


def test_a_run_without_the_flag_adds_no_key(monkeypatch, tmp_path):
    calls = []
    for name, fn in fake_reports(calls).items():
        monkeypatch.setattr(G, name, fn)
    state = (torch.zeros(5, 3), torch.zeros(5, dtype=torch.long), torch.tensor([0, 0, 0, 0, 1]))
    r = SampleReports(("bonds",))
    ev = r.evaluate(torch.device("cpu"), state, {}, 2, "add_aromatic")
    smp = [{"pos": torch.zeros(4, 3), "atom": [7, 6, 8, 6]}, {"pos": torch.zeros(1, 3), "atom": [6]}]
    r.annotate(smp, ev)
    assert calls == [("bonds", ())] and list(ev) == ["bonds"] and "groups" not in r.seconds
    assert not set(GROUP_FIELDS) & set(smp[0]) and list(r.pocket_counts(ev, 0, 2)) == ["bonds"]
    r.finish(str(tmp_path), 0, torch.device("cpu"))
    assert os.listdir(tmp_path) == ["bonds_summary.json"]
    assert SampleReports(()).evaluate(torch.device("cpu"), state, {}, 2, "add_aromatic") == {}


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    idx, b = torch.tensor([[0], [1]], dtype=torch.int32), torch.zeros(2, dtype=torch.long)
    bonds = {"bond_index": idx, "bond_order": torch.ones(1, dtype=torch.uint8), "graph_counts": torch.zeros(1, 6, dtype=torch.int32)}
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.ligand_groups(torch.full((2,), 6), b, 1, bonds)
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.batch_groups({"num_graphs": 1}, torch.zeros(2, 3), torch.ones(2, dtype=torch.long), b, "basic", bonds=bonds)


def test_sample_cli_refusals():
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    with pytest.raises(SystemExit, match="--groups runs on the GPU"):
        sample_cli.main(["--config", cfg, "--device", "cpu", "--groups", "--random_init", "--synthetic", "1"])
    with pytest.raises(SystemExit, match="--groups_reference needs --groups"):
        sample_cli.main(["--config", cfg, "--device", "cpu", "--groups_reference", "nowhere.npz", "--random_init", "--synthetic", "1"])


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_ligand_groups", "cbgx_ligand_groups_templates")


def test_entries_are_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH, sources
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _native.EXPORTS and hasattr(lib, name)
    assert len(_native.EXPORTS[ENTRIES[0]][1]) == 13 and len(_native.EXPORTS[ENTRIES[1]][1]) == 4
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ENTRIES:
            assert f" {name}\n" in sym, (path, name)
    for xcheck in (False, True):
        assert any(os.path.basename(p) == "groups.hip" for p in sources(xcheck))
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    assert f"#define CBGX_GROUPS_GRAPH_COLS {len(G.GROUP_GRAPH_COLUMNS)} " in hdr
    for name, value in (("MAX_ATOMS", G.MAX_GROUP_ATOMS), ("CLASSES", G.GROUP_CLASSES), ("MAX_TEMPLATE_ATOMS", G.MAX_GROUP_TEMPLATE_ATOMS),
                        ("MAX_TEMPLATE_BONDS", G.MAX_GROUP_TEMPLATE_BONDS), ("NO_GROUP", G.GROUP_NO_GROUP),
                        ("TOO_MANY_ATOMS", G.GROUPS_TOO_MANY_ATOMS), ("BAD_BONDS", G.GROUPS_BAD_BONDS), ("NO_AROMATIC", G.GROUPS_NO_AROMATIC)):
        assert f"#define CBGX_GROUPS_{name} {value}\n" in hdr, name
    assert (G.MAX_GROUP_ATOMS, G.GROUP_CLASSES, G.MAX_GROUP_TEMPLATE_ATOMS, G.GROUP_OTHER, G.GROUP_NO_GROUP) == \
        (GM.MAX_ATOMS, GM.CLASSES, GM.MAX_TEMPLATE_ATOMS, GM.OTHER, GM.NO_GROUP) == (256, 25, 10, 25, 254)
    assert (GM.TOO_MANY_ATOMS, GM.BAD_BONDS, GM.NO_AROMATIC) == (G.GROUPS_TOO_MANY_ATOMS, G.GROUPS_BAD_BONDS, G.GROUPS_NO_AROMATIC) == (1, 4, 8)
    for name in N:
        assert name in hdr, name
    assert lib.cbgx_ligand_groups_templates(None, None, None, None) == -1 and b"NULL" in lib.cbgx_last_error()


ONE = ctypes.c_void_p(16)       # a pointer that is never dereferenced: argument checks come first
POINTERS = ("z", "bond_ptr", "bond_index", "bond_order", "bond_aromatic", "atom_group", "atom_class", "graph_out")


def _groups(lig_ptr, n_lig, B, n_bonds, **kw):
    lp = np.asarray([] if lig_ptr is None else lig_ptr, np.int32)
    lptr = ctypes.c_void_p(lp.ctypes.data) if lig_ptr is not None else None
    a = {k: kw.get(k, ONE) for k in POINTERS}
    return _native.lib().cbgx_ligand_groups(a["z"], lptr, n_lig, B, a["bond_ptr"], a["bond_index"], a["bond_order"], a["bond_aromatic"],
                                            n_bonds, a["atom_group"], a["atom_class"], a["graph_out"], None)


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    ok = [0, 2, 4]
    bad = [_groups(ok, 4, -1, 3), _groups(ok, -1, 2, 3), _groups(ok, 4, 2, -1)]
    assert bad == [-1] * 3 and b"negative" in lib.cbgx_last_error()
    for name in POINTERS:
        if name != "bond_aromatic":
            assert _groups(ok, 4, 2, 3, **{name: None}) == -1 and b"NULL" in lib.cbgx_last_error(), name
    assert _groups(None, 4, 2, 3) == -1 and b"NULL" in lib.cbgx_last_error()
    # B == 0: nothing to do, nothing is dereferenced
    assert _groups(None, 0, 0, 0, **{k: None for k in POINTERS}) == 0
    assert _groups(None, 7, 0, 5, bond_ptr=None, graph_out=None) == 0
    # bond_aromatic may always be NULL, the two per-bond arrays without bonds.  What then refuses these calls is host memory: the first
    # array in argument order that the device cannot read is named
    z = np.full(4, 6, np.uint8)
    zp = ctypes.c_void_p(z.ctypes.data)
    for kw in ({"bond_aromatic": None}, {"bond_index": None, "bond_order": None, "bond_aromatic": None}):
        assert _groups(ok, 4, 2, 0 if "bond_index" in kw else 3, z=zp, **kw) == -1
        msg = lib.cbgx_last_error().decode()
        assert "NULL" not in msg and "z_lig is not memory the device can read" in msg
    # sizes are never refused here: a graph over the limit is reported in its status
    assert _groups([0, 3, 1000], 1000, 2, 0, z=zp, bond_index=None, bond_order=None) == -1
    assert "not memory the device can read" in lib.cbgx_last_error().decode()
