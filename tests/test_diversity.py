"""The fingerprint, hash and per-pocket diversity definitions (include/cbgx.h, cbgx_ligand_fingerprints / cbgx_group_diversity) in their
plain-Python model (tests/diversity_model.py), and the host side of the report: pinned values, invariance under relabelling, the stated
limits of the hash, rounding and ties, totals and summaries, the report plumbing on stand-ins for the device entries, refusals and the C
ABI.  No GPU."""
import ctypes
import json
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from cbgbench_amd import _native, geometry as G, sample_reports
from cbgbench_amd.sample_reports import SampleReports
from tests import diversity_model as DM
from tests import rings_model as RM
from tests.test_valence import molecule_like, ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- cases: (n, [(i, j, type)] sorted with i < j, z, atom_ring_min) ------------------------------------------------------------------------
def case(z, bonds, ring_min=None):
    """``bonds`` [(a, b, type)] in any order and orientation; atom_ring_min from the ring model when not given"""
    rows = sorted((min(a, b), max(a, b), t) for a, b, t in bonds)
    assert len({(i, j) for i, j, _ in rows}) == len(rows)
    if ring_min is None:
        ring_min = RM.graph_rings(len(z), [(i, j) for i, j, _ in rows])[2]
    return len(z), rows, list(z), list(ring_min)


def typed(pairs, t):
    return [(a, b, t) for a, b in pairs]


def permuted(c, perm):
    """atom a becomes perm[a]; the list is sorted again, so its order is shuffled with it"""
    n, rows, z, ring_min = c
    new_z, new_ring = [0] * n, [0] * n
    for a in range(n):
        new_z[perm[a]], new_ring[perm[a]] = z[a], ring_min[a]
    return n, sorted((min(perm[i], perm[j]), max(perm[i], perm[j]), t) for i, j, t in rows), new_z, new_ring


def collate(cases):
    """-> (z, lig_ptr, n_lig, bond_ptr, bond_index, bond_type, atom_ring_min): the arguments of DM.batch_fingerprints and of the entry"""
    lig_ptr = np.concatenate([[0], np.cumsum([c[0] for c in cases])]).astype(np.int32)
    n_lig = int(lig_ptr[-1])
    idx = np.array([(lig_ptr[g] + i, lig_ptr[g] + j) for g, c in enumerate(cases) for i, j, _ in c[1]], np.int32).reshape(-1, 2).T.copy()
    bond_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx[0], minlength=n_lig))]).astype(np.int32)
    return (np.array([v for c in cases for v in c[2]], np.uint8), lig_ptr, n_lig, bond_ptr, idx,
            np.array([t for c in cases for _, _, t in c[1]], np.uint8), np.array([v for c in cases for v in c[3]], np.uint8))


def one(c):
    """(fp, hash, n_bits, n_rounds) of one case"""
    return DM.fingerprint(c[2], c[1], c[3])


DECALIN = ring(6) + [(5, 6), (6, 7), (7, 8), (8, 9), (9, 4)]
HAND = {
    "benzene": case([6] * 6, typed(ring(6), 4)),
    "toluene": case([6] * 7, typed(ring(6), 4) + [(0, 6, 1)]),
    "pyridine": case([7] + [6] * 5, typed(ring(6), 4)),
    "cyclohexane": case([6] * 6, typed(ring(6), 1)),
    "two_cyclopropanes": case([6] * 6, typed(ring(3) + ring(3, 3), 1)),
    "decalin": case([6] * 10, typed(DECALIN, 1)),
    "bicyclopentyl": case([6] * 10, typed(ring(5) + ring(5, 5) + [(0, 5)], 1)),
    "phenol": case([6] * 6 + [8], typed(ring(6), 4) + [(0, 6, 1)]),
    "acetamide": case([6, 6, 8, 7], [(0, 1, 1), (1, 2, 2), (1, 3, 1)]),
    "acetonitrile": case([6, 6, 7], [(0, 1, 1), (1, 2, 3)]),
    "naphthalene": case([6] * 10, typed(DECALIN, 4)),
    "water": case([8], []),
    "two_atoms": case([6, 8], [(0, 1, 2)]),
    "unknown_element": case([6, 5], [(0, 1, 1)]),
}


def from_valence_case(c):
    n, pairs, z, order, aromatic = c
    return case(z, [(i, j, 4 if a else o) for (i, j), o, a in zip(pairs, order, aromatic)])


def seeded(count=40, seed=11):
    rng = random.Random(seed)
    return [from_valence_case(molecule_like(rng)) for _ in range(count)]


# ---- the pinned values of the definition ------------------------------------------------------------------------------------------------------
def test_pinned_hashes_bits_and_similarities():
    assert DM.mix(0) == 0 and DM.mix(1) == 0x5692161D100B05E5          # the splitmix64 finaliser itself
    fps = {k: one(HAND[k]) for k in ("benzene", "toluene", "pyridine", "cyclohexane")}
    assert HAND["toluene"][3] == [6] * 6 + [0] and HAND["cyclohexane"][3] == [6] * 6
    assert fps["benzene"][1:] == (0xDF3D2164081C0C2E, 3, 6)
    assert fps["toluene"][1:] == (0x704E731148F194FD, 11, 7)
    assert fps["pyridine"][1:] == (0xAE9FCE6A27F6280E, 9, 6)
    assert fps["cyclohexane"][1] == 0x351BDBD9CA516C9C
    assert DM.tanimoto_micro(fps["benzene"][0], fps["pyridine"][0]) == 333333
    assert DM.tanimoto_micro(fps["benzene"][0], fps["toluene"][0]) == 272727
    assert one(HAND["water"])[2:] == (3, 2) and one(HAND["two_atoms"])[3] == 2


def test_invariance_under_atom_permutations_with_shuffled_bond_order():
    rng = random.Random(5)
    for k, c in enumerate(list(HAND.values()) + seeded()):
        want = one(c)
        for _ in range(3):
            perm = rng.sample(range(c[0]), c[0])
            p = permuted(c, perm)
            shuffled = (p[0], rng.sample(p[1], len(p[1])), p[2], p[3])       # the model takes the bonds in any order
            assert one(p) == want and one(shuffled) == want, k
    hashes = {one(c)[1] for c in seeded()}
    assert len(hashes) == 40                                                 # and it tells the seeded molecules apart


def test_the_ring_term_and_the_stated_blind_spot():
    names = ("cyclohexane", "two_cyclopropanes", "decalin", "bicyclopentyl")
    assert len({one(HAND[k])[1] for k in names}) == 4
    without = {k: one(HAND[k][:3] + ([0] * HAND[k][0],))[1] for k in names}
    assert without["cyclohexane"] == without["two_cyclopropanes"] and without["decalin"] == without["bicyclopentyl"]
    assert without["cyclohexane"] != without["decalin"]
    # the documented limit: rings above 9 atoms have no ring term to tell them apart
    c20, c10 = case([6] * 20, typed(ring(20), 1)), case([6] * 20, typed(ring(10) + ring(10, 10), 1))
    assert c20[3] == c10[3] == [0] * 20 and one(c20)[:2] == one(c10)[:2]
    c9, c18 = case([6] * 18, typed(ring(9) + ring(9, 9), 1)), case([6] * 18, typed(ring(18), 1))
    assert one(c9)[1] != one(c18)[1]


def test_tanimoto_rounding_at_exact_halves():
    def rows(inter, only_a, only_b):
        a, b = [0] * 32, [0] * 32
        for k in range(inter + only_a + only_b):
            bit = 37 * k % 1024
            if k < inter + only_a:
                a[bit >> 5] |= 1 << (bit & 31)
            if k < inter or k >= inter + only_a:
                b[bit >> 5] |= 1 << (bit & 31)
        return a, b

    # inter / uni = 1 / 64 = 0.015625 exactly: 15625 millionths; 1 / 128 = 7812.5 rounds half up; 3 / 128 = 23437.5 too
    for inter, uni, want in ((1, 64, 15625), (1, 128, 7813), (3, 128, 23438), (1, 3, 333333), (2, 3, 666667), (0, 5, 0), (7, 7, 1000000)):
        a, b = rows(inter, (uni - inter) // 2, uni - inter - (uni - inter) // 2)
        assert DM.tanimoto_micro(a, b) == want == DM.tanimoto_micro(b, a)
        assert G.tanimoto_micro(a, b) == want
        signed = lambda w: torch.tensor(np.array(w, np.uint32).view(np.int32))
        assert G.tanimoto_micro(signed(a), signed(b)) == want == G.tanimoto_micro(np.array(a, np.uint32), b)
    assert DM.tanimoto_micro([0] * 32, [0] * 32) == 0 == G.tanimoto_micro([0] * 32, [0] * 32)
    with pytest.raises(ValueError):
        G.tanimoto_micro([0] * 31, [0] * 32)
    assert G.mol_hash_int(torch.tensor(-1, dtype=torch.int64)) == 2 ** 64 - 1 and G.mol_hash_int(np.int64(5)) == 5


def model_batch(cases):
    return DM.batch_fingerprints(*collate(cases))


def test_ties_go_to_the_smallest_index():
    b, t, p = HAND["benzene"], HAND["toluene"], HAND["pyridine"]
    fp, h, out = model_batch([t, b, p, b, t, b])
    pair_sim, first, nearest, micro, group = DM.group_diversity(fp, h, out[:, 4], [0, 6])
    assert first.tolist() == [0, 1, 2, 1, 0, 1]                         # a duplicate that is not adjacent
    assert nearest.tolist() == [4, 3, 1, 1, 0, 1] and micro.tolist() == [1000000, 1000000, 333333, 1000000, 1000000, 1000000]
    assert group[0].tolist() == [6, 6, 3, 15, int(pair_sim.sum()), 1000000, 0] and len(pair_sim) == 15
    assert pair_sim[:5].tolist() == [272727, DM.tanimoto_micro(fp[0], fp[2]), 272727, 1000000, 272727]
    # two pyridines at the same distance from benzene: the first is its nearest
    fp, h, out = model_batch([b, p, p])
    _, first, nearest, _, group = DM.group_diversity(fp, h, out[:, 4], [0, 3])
    assert nearest.tolist() == [1, 2, 1] and first.tolist() == [0, 1, 1] and group[0, 2] == 2


def test_a_group_with_members_that_were_not_evaluated():
    big = case([6] * 257, typed([(a, a + 1) for a in range(256)], 1), [0] * 257)
    empty = case([], [])
    cases = [HAND["benzene"], big, HAND["benzene"], empty, HAND["pyridine"]]
    fp, h, out = model_batch(cases)
    assert out[:, 4].tolist() == [0, DM.TOO_MANY_ATOMS, 0, DM.EMPTY, 0] and out[1].tolist() == [257, 256, -1, -1, 1]
    assert not fp[1].any() and h[1] == 0 and out[3].tolist() == [0, 0, -1, -1, 16]
    pair_sim, first, nearest, micro, group = DM.group_diversity(fp, h, out[:, 4], [0, 5])
    assert pair_sim.tolist() == [-1, 1000000, -1, 333333, -1, -1, -1, -1, 333333, -1]
    assert first.tolist() == [0, -1, 0, -1, 4] and nearest.tolist() == [2, -1, 0, -1, 0] and micro.tolist() == [1000000, -1, 1000000, -1, 333333]
    assert group[0].tolist() == [5, 3, 2, 3, 1666666, 1000000, 0]
    # one evaluated molecule has no neighbour; none at all has nothing
    _, first, nearest, micro, group = DM.group_diversity(fp, h, out[:, 4], [0, 2, 2, 4, 5])
    assert first.tolist() == [0, -1, 0, -1, 0] and nearest.tolist() == [-1] * 5 and micro.tolist() == [-1] * 5
    assert group.tolist() == [[2, 1, 1, 0, 0, -1, 0], [0, 0, 0, 0, 0, -1, 0], [2, 1, 1, 0, 0, -1, 0], [1, 1, 1, 0, 0, -1, 0]]
    m = G.similarity_matrix(pair_sim, [s == 0 for s in out[:, 4]])
    assert m.dtype == torch.int32 and torch.equal(m, m.T) and m.diagonal().tolist() == [1000000, -1, 1000000, -1, 1000000]
    assert (m[1] == -1).all() and (m[:, 3] == -1).all() and m[0, 2] == 1000000 and m[2, 4] == 333333


def test_status_bits_of_the_fingerprint_model():
    cases = [HAND["toluene"], HAND["acetamide"], HAND["naphthalene"]]
    args = list(collate(cases))
    clean = DM.batch_fingerprints(*args)
    assert (clean[2][:, 4] == 0).all() and clean[2][:, 3].tolist() == [7, 4, 10]
    for where, value, want in ((7 + 1, 255, DM.NO_TYPES), (7 + 1, 0, DM.BAD_BONDS), (7 + 1, 5, DM.BAD_BONDS)):
        a = list(args)
        a[5] = a[5].copy()
        a[5][where] = value
        got = DM.batch_fingerprints(*a)
        assert got[2][:, 4].tolist() == [0, want, 0] and not got[0][1].any() and got[1][1] == 0
        assert np.array_equal(got[0][[0, 2]], clean[0][[0, 2]])
    a = list(args)
    a[6] = a[6].copy()
    a[6][8] = 255
    assert DM.batch_fingerprints(*a)[2][:, 4].tolist() == [0, DM.NO_TYPES, 0]


# ---- totals and summaries ---------------------------------------------------------------------------------------------------------------------
ROWS = np.array([[4, 4, 2, 6, 3000000, 1000000, 0],        # two pairs of twins
                 [3, 3, 1, 3, 3000000, 1000000, 0],        # collapsed
                 [2, 1, 1, 0, 0, -1, 0],                   # one evaluated molecule: no pair
                 [1025, -1, -1, -1, -1, -1, 1],            # over the limit
                 [3, 3, 3, 3, 1000001, 400000, 4]], np.int64)


def test_totals_summaries_and_split_ranks():
    assert G.diversity_counts(ROWS[0]) == {"n_mol": 4, "n_mol_evaluated": 4, "n_unique": 2, "n_pairs": 6, "sim_micro_sum": 3000000,
                                           "diversity_micro": 500000}
    assert G.diversity_counts(ROWS[4])["diversity_micro"] == 1000000 - (1000001 + 1) // 3 == DM.diversity_micro(1000001, 3)
    assert G.diversity_counts(ROWS[2])["diversity_micro"] == -1
    assert G.diversity_counts(ROWS[3]) == {"n_mol": 1025, "n_mol_evaluated": 0, "n_unique": 0, "n_pairs": 0, "sim_micro_sum": 0,
                                           "diversity_micro": -1}
    totals = G.diversity_totals(ROWS)
    c = dict(zip(G.DIVERSITY_COUNT_KEYS, totals))
    assert c == {"n_pockets": 5, "n_mol": 1037, "n_mol_evaluated": 11, "n_mol_over_limit": 1026, "n_unique": 7, "n_pairs": 12,
                 "sim_micro_sum": 7000001, "n_pockets_with_pair": 3, "diversity_micro_sum": 500000 + 0 + 666666,
                 "n_pockets_with_two": 3, "n_collapsed_pockets": 1}
    assert all(isinstance(v, int) for v in totals)
    s = G.summarise_diversity_totals(totals)
    assert s == G.summarise_diversity(torch.from_numpy(ROWS)) and s["counts"] == c and s["n_mol_over_limit"] == 1026
    assert s["unique_mol_ratio"] == 7 / 11 and s["duplicate_mol_ratio"] == 4 / 11 and s["mean_pair_similarity"] == 7000001 / 12e6
    assert s["mean_pocket_diversity"] == 1166666 / 3e6 and s["collapsed_pocket_ratio"] == 1 / 3
    assert set(s) == set(G.DIVERSITY_RATIOS) | {"n_mol_over_limit", "counts"}
    # pockets split over "ranks": the same integers, whatever the split
    for cut in range(6):
        parts = [G.diversity_totals(ROWS[:cut]), G.diversity_totals(ROWS[cut:])]
        assert [a + b for a, b in zip(*parts)] == totals
    nothing = G.summarise_diversity(np.zeros((0, 7)))
    assert all(math.isnan(nothing[k]) for k in G.DIVERSITY_RATIOS) and nothing["counts"]["n_pockets"] == 0
    lonely = G.summarise_diversity(ROWS[2:3])
    assert lonely["unique_mol_ratio"] == 1.0 and all(math.isnan(lonely[k]) for k in G.DIVERSITY_RATIOS[2:])
    assert G.group_pair_ptr([0, 4, 4, 7, 8], 8) == [0, 6, 6, 9, 9] == DM.pair_ptr_of([0, 4, 4, 7, 8], 8).tolist()
    assert G.group_pair_ptr([-3, 2, 1, 99], 5) == [0, 1, 1, 7] == DM.pair_ptr_of([-3, 2, 1, 99], 5).tolist()


# ---- the reports' host side -------------------------------------------------------------------------------------------------------------------
DIVERSITY_FIELDS = ("fingerprint", "mol_hash", "duplicate_of", "nearest_sample", "nearest_similarity", "diversity_status")


def fake_reports(calls, group_ptrs):
    """stand-ins for geometry.batch_*: they count their calls and check what they are handed; ``batch_diversity`` answers with the
    model's numbers for toluene, benzene, a molecule over the limit and benzene, as CPU tensors"""
    big = case([6] * 257, typed([(a, a + 1) for a in range(256)], 1), [0] * 257)
    fp, h, out = model_batch([HAND["toluene"], HAND["benzene"], big, HAND["benzene"]])
    made = {"bonds": {"graph_counts": torch.zeros(4, 6, dtype=torch.int32)}, "rings": {"graph_counts": torch.zeros(4, 13, dtype=torch.int32)},
            "aromatic": {"graph_counts": torch.zeros(4, 10, dtype=torch.int32)}}

    def fake(name, wants):
        def run(batch, x, c, lig_batch, mode, *args, **deps):
            calls.append((name, tuple(sorted(k for k, v in deps.items() if v is not None))))
            assert all(deps[k] is made[k] for k in deps if deps[k] is not None) and set(deps) <= set(wants)
            if name != "diversity":
                return made[name]
            (group_ptr,) = args
            group_ptrs.append(group_ptr)
            pair_sim, first, nearest, micro, group = DM.group_diversity(fp, h, out[:, 4], group_ptr)
            t = torch.from_numpy
            return {"fingerprint": t(fp.view(np.int32)), "mol_hash": t(h.view(np.int64)), "graph_counts": t(out), "pair_sim": t(pair_sim),
                    "pair_ptr": t(DM.pair_ptr_of(group_ptr, 4)), "group_ptr": torch.tensor(group_ptr, dtype=torch.int32),
                    "first_same": t(first), "nearest": t(nearest), "nearest_micro": t(micro), "group_counts": t(group)}
        return run

    return {"batch_bonds": fake("bonds", ()), "batch_rings": fake("rings", ("bonds",)), "batch_aromatic": fake("aromatic", ("bonds", "rings")),
            "batch_diversity": fake("diversity", ("bonds", "rings", "aromatic"))}


def test_across_needs_and_the_report_on_stand_ins(monkeypatch, tmp_path, capsys):
    assert sample_reports.ACROSS == ("diversity",) and sample_reports.LATE == ("groups",) and sample_reports.EXTRA == ("interactions",)
    assert sample_reports.NEEDS["diversity"] == ("bonds", "rings", "aromatic")
    assert sample_reports.needs("diversity", "add_aromatic") == ("bonds", "rings", "aromatic")
    assert sample_reports.needs("diversity", "basic") == ("bonds", "rings")
    calls, ptrs = [], []
    for name, fn in fake_reports(calls, ptrs).items():
        monkeypatch.setattr(G, name, fn)
    state = (torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), torch.tensor([0, 1, 2, 3]))
    r = SampleReports(("diversity",))
    with pytest.raises(ValueError, match="group_ptr"):
        r.evaluate(torch.device("cpu"), state, {}, 4, "add_aromatic")
    assert calls == []
    ev = r.evaluate(torch.device("cpu"), state, {}, 4, "add_aromatic", group_ptr=[0, 3, 4])
    assert calls == [("bonds", ()), ("rings", ("bonds",)), ("aromatic", ("bonds", "rings")), ("diversity", ("aromatic", "bonds", "rings"))]
    assert ptrs == [[0, 3, 4]] and sorted(ev) == ["diversity"] and sorted(r.seconds) == ["diversity"] and r.seconds["diversity"] > 0.0
    del calls[:]
    SampleReports(("diversity",)).evaluate(torch.device("cpu"), state, {}, 4, "basic", group_ptr=[0, 3, 4])
    assert calls == [("bonds", ()), ("rings", ("bonds",)), ("diversity", ("bonds", "rings"))]
    # the other reports ignore the grouping, with and without it
    del calls[:]
    assert list(SampleReports(("rings",)).evaluate(torch.device("cpu"), state, {}, 4, "basic", group_ptr=[0, 4])) == ["rings"]
    assert list(SampleReports(("rings",)).evaluate(torch.device("cpu"), state, {}, 4, "basic")) == ["rings"]
    assert list(SampleReports(("diversity", "rings")).seconds) == ["rings", "diversity"]

    smp = [{"atom": [6] * 7}, {"atom": [6] * 6}, {"atom": [6] * 257}, {"atom": [6] * 6}]
    r.annotate(smp, ev)
    assert all(sorted(s) == sorted(("atom",) + DIVERSITY_FIELDS) for s in smp)
    assert [s["duplicate_of"] for s in smp] == [0, 1, -1, 0] and [s["nearest_sample"] for s in smp] == [1, 0, -1, -1]
    assert smp[0]["nearest_similarity"] == 0.272727 and math.isnan(smp[2]["nearest_similarity"]) and math.isnan(smp[3]["nearest_similarity"])
    assert [s["diversity_status"] for s in smp] == [0, 0, 1, 0]
    assert smp[1]["mol_hash"] == smp[3]["mol_hash"] == 0xDF3D2164081C0C2E and smp[0]["mol_hash"] == 0x704E731148F194FD and smp[2]["mol_hash"] == 0
    assert smp[0]["fingerprint"].dtype == torch.int32 and smp[0]["fingerprint"].shape == (32,)
    assert G.tanimoto_micro(smp[0]["fingerprint"], smp[3]["fingerprint"]) == 272727      # across pockets: the host helper
    rec0, rec1 = r.pocket_counts(ev, 0, 3), r.pocket_counts(ev, 3, 4)
    assert list(rec0) == ["similarity_micro", "diversity"]
    assert rec0["similarity_micro"].tolist() == [[1000000, 272727, -1], [272727, 1000000, -1], [-1, -1, -1]]
    assert rec0["diversity"] == {"n_mol": 3, "n_mol_evaluated": 2, "n_unique": 2, "n_pairs": 1, "sim_micro_sum": 272727, "diversity_micro": 727273}
    assert rec1["similarity_micro"].tolist() == [[1000000]] and rec1["diversity"]["diversity_micro"] == -1
    with pytest.raises(ValueError, match="no group"):
        r.pocket_counts(ev, 0, 2)
    r.finish(str(tmp_path), 0, torch.device("cpu"))
    want = G.summarise_diversity(ev["diversity"]["group_counts"])
    with open(tmp_path / "diversity_summary.json") as f:
        assert f.read() == json.dumps(want, indent=1, sort_keys=True)
    assert os.listdir(tmp_path) == ["diversity_summary.json"] and want["counts"]["n_mol_over_limit"] == 1
    line = capsys.readouterr().out
    assert line.startswith("diversity: unique_mol_ratio 1.0000, duplicate_mol_ratio 0.0000, mean_pair_similarity 0.2727, mean_pocket_diversity 0.7273")
    assert "3 of 4 molecules evaluated in 2 pockets" in line and "not an isomorphism test" in line and "not RDKit's" in line


def test_a_run_without_the_flag_adds_no_key(monkeypatch, tmp_path):
    calls = []
    for name, fn in fake_reports(calls, []).items():
        monkeypatch.setattr(G, name, fn)
    state = (torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), torch.tensor([0, 1, 2, 3]))
    r = SampleReports(("rings",))
    ev = r.evaluate(torch.device("cpu"), state, {}, 4, "basic", group_ptr=[0, 4])
    assert [n for n, _ in calls] == ["bonds", "rings"] and "diversity" not in r.seconds and list(ev) == ["rings"]
    r.finish(str(tmp_path), 0, torch.device("cpu"))
    assert os.listdir(tmp_path) == ["rings_summary.json"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    idx, b = torch.tensor([[0], [1]], dtype=torch.int32), torch.zeros(2, dtype=torch.long)
    bonds = {"bond_index": idx, "bond_order": torch.ones(1, dtype=torch.uint8), "graph_counts": torch.zeros(1, 6, dtype=torch.int32)}
    rings = {"atom_ring_min": torch.zeros(2, dtype=torch.uint8)}
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.ligand_fingerprints(torch.full((2,), 6), b, 1, bonds, rings)
    fps = {"fingerprint": torch.zeros(1, 32, dtype=torch.int32), "mol_hash": torch.zeros(1, dtype=torch.int64),
           "graph_counts": torch.zeros(1, 5, dtype=torch.int32)}
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.group_diversity(fps, [0, 1])
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.batch_diversity({"num_graphs": 1}, torch.zeros(2, 3), torch.ones(2, dtype=torch.long), b, "basic", [0, 1], bonds=bonds, rings=rings)


def test_sample_cli_refusal_on_the_cpu():
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    with pytest.raises(SystemExit, match=r"--diversity runs on the GPU \(cbgx_ligand_fingerprints / cbgx_group_diversity have no CPU fallback\)"):
        sample_cli.main(["--config", cfg, "--device", "cpu", "--diversity", "--random_init", "--synthetic", "1"])


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_ligand_fingerprints", "cbgx_group_diversity")


def test_entries_are_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH, sources
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _native.EXPORTS and hasattr(lib, name)
    assert len(_native.EXPORTS[ENTRIES[0]][1]) == 13 and len(_native.EXPORTS[ENTRIES[1]][1]) == 14
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ENTRIES:
            assert f" {name}\n" in sym, (path, name)
    for xcheck in (False, True):
        assert any(os.path.basename(p) == "diversity.hip" for p in sources(xcheck))
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    assert f"#define CBGX_FINGERPRINT_GRAPH_COLS {len(G.FINGERPRINT_GRAPH_COLUMNS)} " in hdr
    assert f"#define CBGX_DIVERSITY_GROUP_COLS {len(G.DIVERSITY_GROUP_COLUMNS)} " in hdr
    for name, value in (("FINGERPRINT_MAX_ATOMS", G.MAX_FINGERPRINT_ATOMS), ("FINGERPRINT_BITS", G.FINGERPRINT_BITS),
                        ("FINGERPRINT_WORDS", G.FINGERPRINT_WORDS), ("FINGERPRINT_TOO_MANY_ATOMS", G.FINGERPRINT_TOO_MANY_ATOMS),
                        ("FINGERPRINT_BAD_BONDS", G.FINGERPRINT_BAD_BONDS), ("FINGERPRINT_NO_TYPES", G.FINGERPRINT_NO_TYPES),
                        ("FINGERPRINT_EMPTY", G.FINGERPRINT_EMPTY), ("DIVERSITY_MAX_GROUP", G.MAX_DIVERSITY_GROUP),
                        ("DIVERSITY_TOO_MANY_GRAPHS", G.DIVERSITY_TOO_MANY_GRAPHS), ("DIVERSITY_BAD_GROUPS", G.DIVERSITY_BAD_GROUPS)):
        assert f"#define CBGX_{name} {value}\n" in hdr, name
    assert (G.MAX_FINGERPRINT_ATOMS, G.FINGERPRINT_BITS, G.FINGERPRINT_WORDS, G.MAX_DIVERSITY_GROUP, len(G.FINGERPRINT_GRAPH_COLUMNS),
            len(G.DIVERSITY_GROUP_COLUMNS)) == (DM.MAX_ATOMS, DM.BITS, DM.WORDS, DM.MAX_GROUP, DM.COLS, DM.GROUP_COLS) == (256, 1024, 32, 1024, 5, 7)
    assert (DM.TOO_MANY_ATOMS, DM.BAD_BONDS, DM.NO_TYPES, DM.EMPTY) == (1, 4, 8, 16) == \
        (G.FINGERPRINT_TOO_MANY_ATOMS, G.FINGERPRINT_BAD_BONDS, G.FINGERPRINT_NO_TYPES, G.FINGERPRINT_EMPTY)
    assert (DM.TOO_MANY_GRAPHS, DM.BAD_GROUPS) == (G.DIVERSITY_TOO_MANY_GRAPHS, G.DIVERSITY_BAD_GROUPS) == (1, 4)
    for text in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "NOT a proof of isomorphism", "RDKFingerprint"):
        assert text in hdr, text


ONE = ctypes.c_void_p(16)       # a pointer that is never dereferenced: argument checks come first
FP_POINTERS = ("z", "bond_ptr", "bond_index", "bond_type", "ring", "fp", "mol_hash", "graph_out")
DV_POINTERS = ("fp", "mol_hash", "status", "group_ptr", "pair_ptr", "pair_sim", "first_same", "nearest", "nearest_micro", "group_out")


def _fingerprints(lig_ptr, n_lig, B, n_bonds, **kw):
    lp = np.asarray([] if lig_ptr is None else lig_ptr, np.int32)
    lptr = ctypes.c_void_p(lp.ctypes.data) if lig_ptr is not None else None
    a = {k: kw.get(k, ONE) for k in FP_POINTERS}
    return _native.lib().cbgx_ligand_fingerprints(a["z"], lptr, n_lig, B, a["bond_ptr"], a["bond_index"], a["bond_type"], a["ring"], n_bonds,
                                                  a["fp"], a["mol_hash"], a["graph_out"], None)


def _diversity(B, P, n_pairs, **kw):
    a = {k: kw.get(k, ONE) for k in DV_POINTERS}
    return _native.lib().cbgx_group_diversity(a["fp"], a["mol_hash"], a["status"], a["group_ptr"], a["pair_ptr"], B, P, n_pairs, a["pair_sim"],
                                              a["first_same"], a["nearest"], a["nearest_micro"], a["group_out"], None)


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    ok = [0, 2, 4]
    assert [_fingerprints(ok, 4, -1, 3), _fingerprints(ok, -1, 2, 3), _fingerprints(ok, 4, 2, -1)] == [-1] * 3
    assert b"negative" in lib.cbgx_last_error()
    for name in FP_POINTERS:
        assert _fingerprints(ok, 4, 2, 3, **{name: None}) == -1 and b"NULL" in lib.cbgx_last_error(), name
    assert _fingerprints(None, 4, 2, 3) == -1 and b"NULL" in lib.cbgx_last_error()
    # B == 0: nothing to do, nothing is dereferenced
    assert _fingerprints(None, 0, 0, 0, **{k: None for k in FP_POINTERS}) == 0
    assert _fingerprints(None, 7, 0, 5, bond_ptr=None, fp=None, graph_out=None) == 0
    # the two per-bond arrays may be NULL without bonds.  What then refuses the call is host memory: the first array in argument order
    # that the device cannot read is named
    z = np.full(4, 6, np.uint8)
    zp = ctypes.c_void_p(z.ctypes.data)
    for kw, nb in (({}, 3), ({"bond_index": None, "bond_type": None}, 0)):
        assert _fingerprints(ok, 4, 2, nb, z=zp, **kw) == -1
        msg = lib.cbgx_last_error().decode()
        assert "NULL" not in msg and "z_lig is not memory the device can read" in msg
    assert _fingerprints([0, 3, 1000], 1000, 2, 0, z=zp, bond_index=None, bond_type=None) == -1      # sizes are never refused here
    assert "not memory the device can read" in lib.cbgx_last_error().decode()

    assert [_diversity(-1, 1, 0), _diversity(2, -1, 1), _diversity(2, 1, -1)] == [-1] * 3 and b"negative" in lib.cbgx_last_error()
    for name in DV_POINTERS:
        assert _diversity(2, 1, 1, **{name: None}) == -1 and b"NULL" in lib.cbgx_last_error(), name
    # P == 0: nothing to do, nothing is dereferenced; pair_sim may be NULL without pairs, the per-graph arrays without graphs
    assert _diversity(0, 0, 0, **{k: None for k in DV_POINTERS}) == 0 and _diversity(5, 0, 3, group_ptr=None, group_out=None) == 0
    fp = np.zeros((2, 32), np.uint32)
    assert fp.ctypes.data % 16 == 0
    fpp = ctypes.c_void_p(fp.ctypes.data)
    assert _diversity(2, 1, 0, fp=fpp, pair_sim=None) == -1
    msg = lib.cbgx_last_error().decode()
    assert "NULL" not in msg and "fp is not memory the device can read" in msg
    gp = np.zeros(2, np.int32)
    assert _diversity(0, 1, 0, group_ptr=ctypes.c_void_p(gp.ctypes.data), **{k: None for k in DV_POINTERS if k not in ("group_ptr", "pair_ptr", "group_out")}) == -1
    assert "group_ptr is not memory the device can read" in lib.cbgx_last_error().decode()
    assert _diversity(2, 1, 1, fp=ctypes.c_void_p(fp.ctypes.data + 4)) == -1 and b"aligned" in lib.cbgx_last_error()
