"""Aromatic atoms and bonds of the table-bond graph (cbgbench_amd/geometry.py: ligand_aromatic, summarise_aromatic, the four-order type
codes, sdf_record; csrc/aromatic.hip), host side: the plain-Python model (tests/aromatic_model.py) against ``networkx.chordless_cycles``
and against hand-computed cases, its independence of the visiting order, its status rows, ``summarise_aromatic`` against hand counts, the
type codes and their strings, the SDF writer against a fixed-width reader, the C ABI of the entry without a device, and the driver's
refusals.  The kernel itself is compared with the model in tests/test_gpu_aromatic.py."""
import ctypes
import os
import random
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import torch

from cbgbench_amd import _native, geometry as G
from tests import aromatic_model as AM, rings_model as RM
from tests.test_rings import NAMED, complete, cyc, norm, seeded_random, triangle_strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C56 against networkx ------------------------------------------------------------------------------------------------------------
def truth_cycles(n, pairs):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(pairs)
    return sorted(tuple(sorted(c)) for c in nx.chordless_cycles(g, length_bound=6) if len(c) in (5, 6))


def model_cycles(n, pairs):
    cycles = AM.chordless_cycles56(n, pairs)
    for c in cycles:                 # a cycle indeed, from its smallest atom, towards the smaller neighbour
        edges = set(pairs)
        assert all((min(a, b), max(a, b)) in edges for a, b in zip(c, c[1:] + c[:1])) and c[0] == min(c) and c[1] < c[-1], c
    return sorted(tuple(sorted(c)) for c in cycles)


@pytest.mark.parametrize("name", list(NAMED))
def test_model_cycles_equal_networkx_on_named_graphs(name):
    assert model_cycles(*NAMED[name]) == truth_cycles(*NAMED[name])


def test_model_cycles_equal_networkx_on_seeded_random_graphs():
    sizes = set()
    for n, pairs in seeded_random(300):
        got = model_cycles(n, pairs)
        assert got == truth_cycles(n, pairs), (n, pairs)
        sizes |= {len(c) for c in got}
    assert sizes == {5, 6}
    # a chordless cycle is determined by its atoms, so comparing atom sets loses nothing
    assert len(set(model_cycles(*NAMED["dodecahedron"]))) == 12 and model_cycles(*NAMED["naphthalene"]) == [(0, 1, 2, 3, 4, 5),
                                                                                                           (0, 1, 6, 7, 8, 9)]
    assert sorted(len(c) for c in model_cycles(*NAMED["norbornane"])) == [5, 5, 6]


# ---- hand-computed cases -------------------------------------------------------------------------------------------------------------
ANTHRACENE = norm(14, cyc(6) + [(5, 6), (6, 7), (7, 8), (8, 9), (9, 4)] + [(8, 10), (10, 11), (11, 12), (12, 13), (13, 7)])
BIPHENYL = norm(12, cyc(6) + cyc(6, 6) + [(0, 6)])
BICYCLO_220 = norm(6, cyc(6) + [(0, 3)])


def _flags(n, on):
    return [a in on for a in range(n)]


#        name: (graph, z, flags, (n_cycles56, n_aromatic_cycles, n_closure, n_aromatic_atoms, n_aromatic_bonds, n_unsupported))
HAND = {
    "benzene_all": (norm(6, cyc(6)), [6] * 6, _flags(6, range(6)), (1, 1, 6, 6, 6, 0)),
    "benzene_alternating": (norm(6, cyc(6)), [6] * 6, _flags(6, (0, 2, 4)), (1, 1, 6, 6, 6, 0)),                    # R3
    "benzene_two": (norm(6, cyc(6)), [6] * 6, _flags(6, (0, 1)), (1, 0, 2, 0, 0, 2)),
    "pyridine_carbons": (norm(6, cyc(6)), [7] + [6] * 5, _flags(6, range(1, 6)), (1, 1, 6, 6, 6, 0)),
    "pyridine_next_to_n": (norm(6, cyc(6)), [7] + [6] * 5, _flags(6, (1, 5)), (1, 0, 3, 0, 0, 2)),                  # R2 fires, R3 does not
    "pentazole_ring": (norm(5, cyc(5)), [7] * 5, _flags(5, ()), (1, 1, 5, 5, 5, 0)),                                # the carbon-free quirk
    "biphenyl": (BIPHENYL, [6] * 12, _flags(12, range(12)), (2, 2, 12, 12, 12, 0)),                                 # the link is not aromatic
    # ring A flagged, one outer atom of B, one outer atom of C: C fires only because B fired
    "anthracene_cascade": (ANTHRACENE, [6] * 14, _flags(14, (0, 1, 2, 3, 4, 5, 6, 10)), (3, 3, 14, 14, 16, 0)),
    "anthracene_no_cascade": (ANTHRACENE, [6] * 14, _flags(14, (0, 1, 2, 3, 4, 5, 10)), (3, 1, 7, 6, 6, 1)),
    "ring_7": (norm(7, cyc(7)), [6] * 7, _flags(7, range(7)), (0, 0, 7, 0, 0, 7)),
    "bicyclo_220_hexane": (BICYCLO_220, [6] * 6, _flags(6, (0, 1, 2)), (0, 0, 3, 0, 0, 3)),                         # the perimeter has a chord
}


def ring_min_of(n, pairs):
    return RM.graph_rings(n, pairs)[2]


@pytest.mark.parametrize("name", list(HAND))
def test_hand_computed_cases(name):
    (n, pairs), z, flags, want = HAND[name]
    row, in_f, on_atom, on_bond = AM.graph_aromatic(n, pairs, z, flags, ring_min_of(n, pairs))
    assert row[:2] == [n, len(pairs)] and row[4] == sum(flags)
    assert (row[2], row[3], row[5], row[6], row[7], row[8]) == want
    assert sum(in_f) == want[2] and sum(on_atom) == want[3] and sum(on_bond) == want[4]
    assert all(f or not a for f, a in zip(in_f, on_atom))          # an aromatic atom is in F


def test_biphenyl_link_and_single_pass():
    (n, pairs), z, flags, _ = HAND["biphenyl"]
    _, _, _, on_bond = AM.graph_aromatic(n, pairs, z, flags, ring_min_of(n, pairs))
    assert len(pairs) == 13 and [e for e, a in zip(pairs, on_bond) if not a] == [(0, 6)]
    # anthracene: one application of R3 to the input flags reaches ring B and not ring C
    (n, pairs), z, flags, _ = HAND["anthracene_cascade"]
    once = set(a for a in range(n) if flags[a])
    for c in AM.chordless_cycles56(n, pairs):
        if 2 * sum(flags[a] for a in c) >= len(c):
            once |= set(c)
    assert len(once) == 11 and sum(AM.graph_aromatic(n, pairs, z, flags, ring_min_of(n, pairs))[1]) == 14


def test_r2_guard():
    # C - O - C with both carbons flagged, the oxygen on no ring: it does not join F; nor with ring_min 255; on a ring it does
    chain = (3, [(0, 1), (1, 2)])
    for ring_min in ([0, 0, 0], [0, 255, 0], [0, 2, 0], [0, 10, 0]):
        assert AM.graph_aromatic(*chain, [6, 8, 6], [True, False, True], ring_min)[0][5] == 2, ring_min
    for ring_min in ([0, 3, 0], [0, 9, 0]):
        assert AM.graph_aromatic(*chain, [6, 8, 6], [True, False, True], ring_min)[0][5] == 3, ring_min
    # a carbon or a sulfur in the same place does not join; a nitrogen does; one flagged neighbour is not enough
    ring = norm(7, cyc(7))
    for z1, joins in ((6, False), (16, False), (7, True), (8, True)):
        z = [6, z1] + [6] * 5
        assert AM.graph_aromatic(*ring, z, _flags(7, (0, 2)), [7] * 7)[0][5] == 2 + joins, z1
    assert AM.graph_aromatic(*ring, [6, 7] + [6] * 5, _flags(7, (0,)), [7] * 7)[0][5] == 1


# ---- the result does not depend on the order of visits ----------------------------------------------------------------------------------
def assignment(n, seed):
    """a seeded element and flag assignment of n atoms"""
    rng = random.Random(seed)
    return [rng.choice([6, 6, 6, 6, 7, 8, 16]) for _ in range(n)], [rng.random() < 0.35 for _ in range(n)]


def test_order_freedom():
    cases = [(g, z, f) for g, z, f, _ in HAND.values()]
    for k, name in enumerate(NAMED):
        cases.append((NAMED[name],) + assignment(NAMED[name][0], 100 + k))
    for k, graph in enumerate(seeded_random(60, seed=11)):
        cases.append((graph,) + assignment(graph[0], 200 + k))
    fired = 0
    for (n, pairs), z, flags in cases:
        rmin = ring_min_of(n, pairs)
        first = AM.graph_aromatic(n, pairs, z, flags, rmin)
        fired += first[0][5] > first[0][4]
        for order in ("reversed", random.Random(5), random.Random(6)):
            assert AM.graph_aromatic(n, pairs, z, flags, rmin, order=order) == first, (n, pairs, order)
    assert fired > 10


# ---- status rows ------------------------------------------------------------------------------------------------------------------------
def one(n, pairs, bond_ptr=None, ring_min=None, z=None, flags=None):
    idx = np.array(pairs, np.int64).reshape(-1, 2).T
    if bond_ptr is None:
        bond_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx[0], minlength=n))])
    ring_min = [0] * n if ring_min is None else ring_min
    atom, bond, out = AM.batch_aromatic([6] * n if z is None else z, [1] * n if flags is None else flags, ring_min, [0, n], n, bond_ptr, idx)
    return atom.tolist(), bond.tolist(), out[0].tolist()


def test_model_limits_and_status():
    atom, bond, row = one(*norm(256, cyc(256)))
    assert row == [256, 256, 0, 0, 256, 256, 0, 0, 256, 0] and set(atom) == {1} and set(bond) == {0}
    atom, bond, row = one(*norm(257, cyc(257)))
    assert row == [257, 257] + [-1] * 7 + [AM.TOO_MANY_ATOMS] and set(atom) == {255} and set(bond) == {255}
    n, pairs = triangle_strip(130)                       # 257 bonds = n + 127: evaluated
    atom, bond, row = one(n, pairs)
    assert row == [130, 257, 0, 0, 130, 130, 0, 0, 130, 0]
    n, pairs = triangle_strip(131)                       # 259 bonds = n + 128
    atom, bond, row = one(n, pairs)
    assert row == [131, 259] + [-1] * 7 + [AM.TOO_MANY_CYCLES] and set(atom) == {255} and set(bond) == {255}
    assert one(*complete(17))[2] == [17, 136, 0, 0, 17, 17, 0, 0, 17, 0]
    assert one(*complete(18))[2] == [18, 153] + [-1] * 7 + [AM.TOO_MANY_CYCLES]
    for bad in ([(0, 1), (2, 1)], [(0, 1), (1, 3)], [(0, 2), (0, 1)], [(0, 1), (0, 1)], [(0, 1), (1, 1)], [(-7, 1), (1, 2)]):
        assert one(3, bad, bond_ptr=[0, 1, 2, 2])[2] == [3, 2] + [-1] * 7 + [AM.BAD_BONDS], bad
    assert one(3, [(0, 1), (1, 2)], bond_ptr=[0, 2, 1, 2])[2][-1] == AM.BAD_BONDS                   # non-monotone inside the graph
    assert one(3, [(0, 1), (1, 2)], bond_ptr=[-3, 1, 2, 2])[2][-1] == AM.BAD_BONDS                  # outside the list
    assert one(3, [(0, 1), (1, 2)], bond_ptr=[0, 1, 2, 9])[2][-1] == AM.BAD_BONDS
    atom, bond, row = one(*norm(6, cyc(6)), ring_min=[6, 6, 255, 6, 6, 6])
    assert row == [6, 6] + [-1] * 7 + [AM.NO_RINGS] and set(atom) == {255} and set(bond) == {255}
    assert one(*norm(257, cyc(257)), ring_min=[255] * 257)[2][-1] == AM.TOO_MANY_ATOMS | AM.NO_RINGS
    assert one(0, [])[2] == [0] * 10 and one(3, [], flags=[0, 1, 0])[2] == [3, 0, 0, 0, 1, 1, 0, 0, 1, 0]
    atom, bond, row = one(*norm(6, cyc(6)), ring_min=[6] * 6, flags=[1, 0, 7, 0, 1, 0])             # any non-zero byte is a flag
    assert row == [6, 6, 1, 1, 3, 6, 6, 6, 0, 0] and atom == [3] * 6 and bond == [1] * 6
    assert (AM.MAX_ATOMS, AM.MAX_CYCLES, AM.COLS, AM.COLUMNS) == (G.MAX_AROMATIC_ATOMS, G.MAX_AROMATIC_CYCLES,
                                                                  len(G.AROMATIC_GRAPH_COLUMNS), G.AROMATIC_GRAPH_COLUMNS)
    assert (AM.TOO_MANY_ATOMS, AM.TOO_MANY_CYCLES, AM.BAD_BONDS, AM.NO_RINGS) == (
        G.AROMATIC_TOO_MANY_ATOMS, G.AROMATIC_TOO_MANY_CYCLES, G.AROMATIC_BAD_BONDS, G.AROMATIC_NO_RINGS) == (1, 2, 4, 8)


# ---- summaries ------------------------------------------------------------------------------------------------------------------------
def test_summarise_aromatic_against_hand_computed_counts():
    #      n_atoms n_bonds c56 arom flagged closure ar_atoms ar_bonds unsupported status
    gc = [[20, 22, 3, 2, 9, 11, 10, 11, 1, 0],
          [10, 9, 0, 0, 2, 2, 0, 0, 2, 0],
          [300, 310, -1, -1, -1, -1, -1, -1, -1, 1],
          [30, 33, 2, 0, 0, 0, 0, 0, 0, 0],
          [12, 12, 1, 1, 6, 6, 6, 6, 0, 0],
          [8, 8, -1, -1, -1, -1, -1, -1, -1, 8]]
    s = G.summarise_aromatic(gc)
    c = s["counts"]
    assert tuple(c) == G.AROMATIC_COUNT_KEYS and set(s) == set(G.AROMATIC_RATIOS) | {"counts"}
    assert [c[k] for k in G.AROMATIC_COUNT_KEYS] == [6, 4, 2, 72, 76, 6, 3, 17, 19, 16, 17, 3, 2]
    assert s["aromatic_mol_ratio"] == 2 / 4 and s["aromatic_rings_per_mol"] == 3 / 4 and s["aromatic_cycle_share"] == 3 / 6
    assert s["aromatic_atom_ratio"] == 16 / 72 and s["aromatic_bond_ratio"] == 17 / 76 and s["unsupported_flag_ratio"] == 3 / 17
    whole = G.aromatic_totals(gc)
    parts = [a + b for a, b in zip(G.aromatic_totals(gc[:2]), G.aromatic_totals(gc[2:]))]
    assert whole == parts and G.summarise_aromatic_totals(parts) == s
    assert G.summarise_aromatic(torch.tensor(gc, dtype=torch.int32)) == s
    for nothing in (np.zeros((0, 10), np.int32), [gc[2]]):
        e = G.summarise_aromatic(nothing)
        assert e["counts"]["n_mol_evaluated"] == 0 and all(np.isnan(e[k]) for k in G.AROMATIC_RATIOS)
    assert G.summarise_aromatic([gc[2], gc[5]])["counts"]["n_mol_over_limit"] == 2


# ---- four-order type codes ----------------------------------------------------------------------------------------------------------------
def test_four_order_type_codes_round_trip():
    assert G.n_type_codes() == (G.N_BOND_TYPES, G.N_ANGLE_TYPES) == (192, 4608) and G.n_type_codes(4) == (256, 8192)
    assert G.N_ANGLE_TYPES_4 - 1 <= np.iinfo(np.int16).max
    seen = set()
    for t in range(1, 5):
        for lo in range(8):
            for hi in range(lo, 8):
                code = G.bond_type_code(hi, t, lo, n_orders=4)
                assert code == ((t - 1) * 8 + lo) * 8 + hi and 0 <= code < 256
                text = G.bond_type_string(code)
                assert text == f"{G._ELEMENTS[lo]}{'-=#:'[t - 1]}{G._ELEMENTS[hi]}"
                assert G._parse_type(text, 4) == ("bond_length", text)
                assert G._parse_type((G._ELEMENTS[hi], G._ELEMENTS[lo], t), 4) == ("bond_length", text)
                if t < 4:
                    assert code == G.bond_type_code(lo, t, hi) and G._parse_type(text) == ("bond_length", text)
                seen.add(code)
    assert len(seen) == 4 * 36
    rng, seen = random.Random(3), set()
    for _ in range(4000):
        c1, cc, c2, t1, t2 = rng.randrange(8), rng.randrange(8), rng.randrange(8), rng.randint(1, 4), rng.randint(1, 4)
        code = G.angle_type_code(c1, t1, cc, t2, c2, n_orders=4)
        (a, ta), (b, tb) = sorted([(c1, t1), (c2, t2)])
        assert code == (((a * 4 + (ta - 1)) * 8 + cc) * 4 + (tb - 1)) * 8 + b and 0 <= code < 8192
        assert code == G.angle_type_code(c2, t2, cc, t1, c1, n_orders=4)
        text = G.angle_type_string(code, 4)
        assert text == f"{G._ELEMENTS[a]}{'-=#:'[ta - 1]}{G._ELEMENTS[cc]}{'-=#:'[tb - 1]}{G._ELEMENTS[b]}"
        assert G._parse_type(text, 4) == ("bond_angle", text)
        flipped = f"{G._ELEMENTS[b]}{'-=#:'[tb - 1]}{G._ELEMENTS[cc]}{'-=#:'[ta - 1]}{G._ELEMENTS[a]}"
        assert G._parse_type(flipped, 4) == ("bond_angle", text)
        assert G._parse_type((G._ELEMENTS[c1], t1, G._ELEMENTS[cc], t2, G._ELEMENTS[c2]), 4) == ("bond_angle", text)
        if t1 < 4 and t2 < 4:      # the three-order strings are the same strings
            assert G.angle_type_string(G.angle_type_code(c1, t1, cc, t2, c2)) == text and G._parse_type(text) == ("bond_angle", text)
        seen.add(code)
    assert len(seen) > 2000


def test_aromatic_keys_parse_with_four_orders_and_not_by_default():
    reason = "aromatic bond type: table bonds have orders 1, 2, 3 only"
    for key, kind, canon in (("6:6", "bond_length", "6:6"), ("6?6", "bond_length", "6:6"), ((6, 6, 4), "bond_length", "6:6"),
                             ((6, 7, 4), "bond_length", "6:7"), ((7, 6, 4), "bond_length", "6:7"), ("6:6:6", "bond_angle", "6:6:6"),
                             ((6, 4, 6, 4, 6), "bond_angle", "6:6:6"), ("8=6:6", "bond_angle", "6:6=8"), ("7:6-6", "bond_angle", "6-6:7")):
        assert G._parse_type(key, 4) == (kind, canon), key
        assert G._parse_type(key) == (None, reason) and G._parse_type(key, n_orders=3) == (None, reason), key
    assert G._parse_type("6-6", 4) == G._parse_type("6-6") == ("bond_length", "6-6")
    assert G._parse_type((6, 6, 5), 4) == (None, "unknown bond order") and G._parse_type("5:6", 4)[0] is None
    with pytest.raises(ValueError):
        G._parse_type("6:6", 5)
    # the totals: the default is today's length, the four-order vector is longer by the new rows
    n_pair, n_bond, n_angle = G.DISTRIBUTION_BINS
    assert G.distribution_totals_length() == G.distribution_totals_length(n_orders=3) == 6 + 2 * n_pair + 192 * n_bond + 4608 * n_angle
    assert G.distribution_totals_length(n_orders=4) == 6 + 2 * n_pair + 256 * n_bond + 8192 * n_angle
    # a job's summary with the aromatic type: the key is evaluated
    totals = np.zeros(G.distribution_totals_length(n_orders=4), np.int64)
    bond0 = 6 + 2 * n_pair
    code = G.bond_type_code(1, 4, 1, n_orders=4)
    totals[bond0 + code * n_bond + 58:bond0 + code * n_bond + 62] = [1, 5, 3, 1]
    angle0 = bond0 + 256 * n_bond
    acode = G.angle_type_code(1, 4, 1, 4, 1, n_orders=4)
    totals[angle0 + acode * n_angle + 60] = 7
    summary = G.summarise_distribution_totals(totals, n_orders=4)
    assert list(summary["bond_length"]) == ["6:6"] and summary["bond_length"]["6:6"]["count"] == 10
    assert list(summary["bond_angle"]) == ["6:6:6"] and summary["bond_angle"]["6:6:6"]["count"] == 7
    ref = np.zeros(n_bond)
    ref[58:62] = [1, 5, 3, 1]
    aref = np.zeros(n_angle)
    aref[60] = 1
    out = G.jsd_against(summary, {(6, 6, 4): ref, "6:6": ref, "6:6:6": aref, (6, 7, 4): ref}, n_orders=4)
    assert out["JSD_6?6"] == pytest.approx(0.0, abs=1e-7) and out["JSD_6:6"] == pytest.approx(0.0, abs=1e-7)
    assert out["JSD_6:6:6"] == pytest.approx(0.0, abs=1e-7)
    assert out["JSD_6?7"] is None and out["not_evaluated"] == {"JSD_6?7": "no such type among the samples"}
    with pytest.raises(ValueError):
        G.summarise_distribution_totals(totals)                    # a four-order vector is not a three-order one
    three = G.summarise_distribution_totals(np.zeros(G.distribution_totals_length(), np.int64))
    assert G.jsd_against(three, {(6, 6, 4): ref})["not_evaluated"] == {"JSD_6?6": reason}


# ---- SDF ----------------------------------------------------------------------------------------------------------------------------------
def read_sdf(text):
    """fixed-width V2000 reader: [(name, pos [n, 3], symbols [n], bonds [(i, j, type)])]"""
    records = []
    blocks = text.split("$$$$\n")
    assert blocks[-1] == ""
    for block in blocks[:-1]:
        lines = block.split("\n")
        assert lines[-1] == "" and lines[-2] == "M  END"
        counts = lines[3]
        assert counts[33:39] == " V2000"
        n, m = int(counts[0:3]), int(counts[3:6])
        assert len(lines) == 4 + n + m + 2
        pos = [[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in lines[4:4 + n]]
        assert all(l[30] == " " for l in lines[4:4 + n])
        symbols = [l[31:34].strip() for l in lines[4:4 + n]]
        bonds = [(int(l[0:3]) - 1, int(l[3:6]) - 1, int(l[6:9])) for l in lines[4 + n:4 + n + m]]
        assert all(l[9:12] == "  0" for l in lines[4 + n:4 + n + m])
        records.append((lines[0], np.array(pos).reshape(-1, 3), symbols, bonds))
    return records


def test_sdf_record_reads_back():
    rng = np.random.default_rng(4)
    pos = rng.normal(0, 30, (8, 3))
    pos[0] = [-123.45678, 0.00004, 99.99995]
    z = [1, 6, 7, 8, 9, 15, 16, 17]
    idx = np.array([[0, 1, 1, 2, 6], [1, 2, 7, 3, 7]])
    types = [1, 2, 3, 4, 4]
    text = G.sdf_record("mol_a", pos, z, idx, types) + G.sdf_record("mol_b", torch.from_numpy(pos[:2]), torch.tensor(z[:2]),
                                                                    torch.tensor(idx[:, :1]), torch.tensor([1], dtype=torch.uint8))
    (name_a, pos_a, sym_a, bonds_a), (name_b, pos_b, sym_b, bonds_b) = read_sdf(text)
    assert name_a == "mol_a" and name_b == "mol_b"
    assert np.abs(pos_a - pos).max() <= 0.5e-4 + 1e-12 and np.abs(pos_b - pos[:2]).max() <= 0.5e-4 + 1e-12
    assert sym_a == ["H", "C", "N", "O", "F", "P", "S", "Cl"] and sym_b == ["H", "C"]
    assert bonds_a == [(0, 1, 1), (1, 2, 2), (1, 7, 3), (2, 3, 4), (6, 7, 4)] and bonds_b == [(0, 1, 1)]
    empty, = read_sdf(G.sdf_record("none", np.zeros((0, 3)), [], np.zeros((2, 0), int), []))
    assert empty[1].shape == (0, 3) and empty[2] == [] and empty[3] == []
    # 999 of each fit, 1000 do not; unknown elements and types are refused
    big = np.zeros((1000, 3))
    chain = np.array([np.arange(999), np.arange(1, 1000)])
    rec, = read_sdf(G.sdf_record("big", big[:999], [6] * 999, chain[:, :998], [1] * 998))
    assert len(rec[2]) == 999 and len(rec[3]) == 998 and rec[3][-1] == (997, 998, 1)
    with pytest.raises(ValueError, match="999"):
        G.sdf_record("big", big, [6] * 1000, chain[:, :10], [1] * 10)
    ring = np.array([np.arange(999), (np.arange(999) + 1) % 999])
    ring = np.concatenate([np.sort(ring, 0), [[0], [2]]], 1)
    with pytest.raises(ValueError, match="999"):
        G.sdf_record("big", big[:999], [6] * 999, ring, [1] * 1000)
    for z_bad in (0, 5, 34, 255):
        with pytest.raises(ValueError, match="element"):
            G.sdf_record("x", big[:2], [6, z_bad], [[0], [1]], [1])
    for t_bad in (0, 5, 255):
        with pytest.raises(ValueError, match="bond type"):
            G.sdf_record("x", big[:2], [6, 6], [[0], [1]], [t_bad])


# ---- the Python entries without a device ----------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    idx, b = torch.tensor([[0], [1]], dtype=torch.int32), torch.zeros(2, dtype=torch.long)
    bonds = {"bond_index": idx, "bond_order": torch.ones(1, dtype=torch.uint8), "graph_counts": torch.zeros(1, 6, dtype=torch.int32)}
    rings = {"atom_ring_min": torch.zeros(2, dtype=torch.uint8)}
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.ligand_aromatic(torch.full((2,), 6), torch.ones(2, dtype=torch.bool), b, 1, bonds, rings)
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.batch_aromatic({"num_graphs": 1}, torch.zeros(2, 3), torch.full((2,), 2), b, "add_aromatic", bonds=bonds, rings=rings)
    with pytest.raises(_native.NativeError):
        G.batch_aromatic({"num_graphs": 1}, torch.zeros(2, 3), torch.full((2,), 2), b, "add_aromatic")
    with pytest.raises(ValueError, match="no aromatic atom types"):
        G.batch_aromatic({"num_graphs": 1}, torch.zeros(2, 3), torch.ones(2, dtype=torch.long), b, "basic", bonds=bonds, rings=rings)


def test_sample_cli_aromatic_needs_the_gpu_and_add_aromatic(tmp_path):
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    with pytest.raises(SystemExit, match="--aromatic runs on the GPU"):
        sample_cli.main(["--config", cfg, "--device", "cpu", "--aromatic", "--random_init", "--synthetic", "1"])
    with pytest.raises(SystemExit, match="--sdf takes its bonds from the GPU"):
        sample_cli.main(["--config", cfg, "--device", "cpu", "--sdf", "--random_init", "--synthetic", "1"])
    # the same config with the 8-type vocabulary: refused before any model is built, whatever the device
    text = open(cfg).read()
    assert text.count("mode: add_aromatic") == 1
    basic = tmp_path / "targetdiff_T20_basic.yml"
    basic.write_text(text.replace("mode: add_aromatic", "mode: basic").replace("!include common/",
                                                                               "!include " + os.path.join(ROOT, "tests", "fixtures", "common") + "/"))
    with pytest.raises(SystemExit, match="mode 'add_aromatic', not 'basic'"):
        sample_cli.main(["--config", str(basic), "--device", "cpu", "--aromatic", "--random_init", "--synthetic", "1",
                         "--out_root", str(tmp_path)])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
ENTRY = "cbgx_ligand_aromatic"


def test_entry_is_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH, sources
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    assert re.search(r"\bint " + ENTRY + r"\(", hdr) and ENTRY in _native.EXPORTS and hasattr(lib, ENTRY)
    assert len(_native.EXPORTS[ENTRY][1]) == 13
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        assert f" {ENTRY}\n" in sym, path
    for xcheck in (False, True):
        assert any(os.path.basename(p) == "aromatic.hip" for p in sources(xcheck))
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    assert f"#define CBGX_AROMATIC_GRAPH_COLS {len(G.AROMATIC_GRAPH_COLUMNS)} " in hdr
    for name, value in (("MAX_ATOMS", G.MAX_AROMATIC_ATOMS), ("MAX_CYCLES", G.MAX_AROMATIC_CYCLES),
                        ("TOO_MANY_ATOMS", G.AROMATIC_TOO_MANY_ATOMS), ("TOO_MANY_CYCLES", G.AROMATIC_TOO_MANY_CYCLES),
                        ("BAD_BONDS", G.AROMATIC_BAD_BONDS), ("NO_RINGS", G.AROMATIC_NO_RINGS)):
        assert f"#define CBGX_AROMATIC_{name} {value}\n" in hdr, name
    assert f"#define CBGX_AROMATIC_BOND_TYPES {G.N_BOND_TYPES_4} " in hdr and f"#define CBGX_AROMATIC_ANGLE_TYPES {G.N_ANGLE_TYPES_4} " in hdr
    assert (G.MAX_AROMATIC_ATOMS, G.MAX_AROMATIC_CYCLES) == (G.MAX_RING_ATOMS, G.MAX_RING_CYCLES)


ONE = ctypes.c_void_p(16)       # a pointer that is never dereferenced: argument checks come first


def _aromatic(lig_ptr, n_lig, B, n_bonds, **kw):
    lp = np.asarray([] if lig_ptr is None else lig_ptr, np.int32)
    lptr = ctypes.c_void_p(lp.ctypes.data) if lig_ptr is not None else None
    a = {k: kw.get(k, ONE) for k in ("z", "flag", "ring_min", "bond_ptr", "bond_index", "atom_out", "bond_aromatic", "graph_out")}
    return _native.lib().cbgx_ligand_aromatic(a["z"], a["flag"], a["ring_min"], lptr, n_lig, B, a["bond_ptr"], a["bond_index"], n_bonds,
                                              a["atom_out"], a["bond_aromatic"], a["graph_out"], None)


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    ok = [0, 2, 4]
    bad = [_aromatic(ok, 4, -1, 3), _aromatic(ok, -1, 2, 3), _aromatic(ok, 4, 2, -1)]
    assert bad == [-1] * 3 and b"negative" in lib.cbgx_last_error()
    for name in ("z", "flag", "ring_min", "bond_ptr", "bond_index", "atom_out", "bond_aromatic", "graph_out"):
        assert _aromatic(ok, 4, 2, 3, **{name: None}) == -1 and b"NULL" in lib.cbgx_last_error(), name
    assert _aromatic(None, 4, 2, 3) == -1 and b"NULL" in lib.cbgx_last_error()
    # B == 0: nothing to do, nothing is dereferenced
    nothing = {k: None for k in ("z", "flag", "ring_min", "bond_ptr", "bond_index", "atom_out", "bond_aromatic", "graph_out")}
    assert _aromatic(None, 0, 0, 0, **nothing) == 0
    assert _aromatic(None, 7, 0, 5, bond_ptr=None, graph_out=None) == 0
    # no bonds: bond_index and bond_aromatic may be NULL.  What then refuses this call is the host memory lig_ptr points to
    assert _aromatic(ok, 4, 2, 0, bond_index=None, bond_aromatic=None) == -1
    msg = lib.cbgx_last_error().decode()
    assert "NULL" not in msg and "lig_ptr" in msg
    # sizes are never refused here: a graph over a limit is reported in its status
    assert _aromatic([0, 3, 1000], 1000, 2, 0, bond_index=None, bond_aromatic=None) == -1 and "lig_ptr" in lib.cbgx_last_error().decode()
