"""The host half of sample_cli's reports (cbgbench_amd/sample_reports.py) alone: per-sample fields, per-pocket counts, SDF text and the
job summaries from hand-written report dicts of CPU tensors.  No GPU, no library.  One batch of four graphs with 3, 0, 1 and 4 atoms (an
empty graph and a single atom in the middle): graph 0 is a chain 0-1-2, graph 3 a 4-ring with one double bond, which neither the ring nor
the aromatic report evaluated.  Every expectation below is written out by hand."""
import json

import numpy as np
import torch

from cbgbench_amd import geometry as G
from cbgbench_amd.sample_reports import SampleReports, ranges

NAN = float("nan")
ALL = ("geometry", "bonds", "rings", "aromatic", "distributions", "sdf")
# global atom rows: graph 0 = 0 1 2, graph 2 = 3, graph 3 = 4 5 6 7; global bond rows: graph 0 = 0 1, graph 3 = 2 3 4 5
C_C, C_DOUBLE_C, C_AROMATIC_C, C_C_C = 9, 73, 201, 1057         # '6-6', '6=6', '6:6', '6-6-6' in the four-order type codes


def reports():
    i32, u8 = torch.int32, torch.uint8
    return {
        "geometry": {"nr_bonds": torch.tensor([1, 2, 1, 0, 2, 2, 3, 3], dtype=i32), "flags": torch.tensor([1, 0, 3, 4, 1, 1, 1, 1], dtype=u8),
                     "graph_counts": torch.tensor([[3, 2, 0, 1, 0, 0], [0, 0, 1, 0, 0, 2], [1, 0, 0, 0, 1, 0], [4, 4, 1, 0, 0, 0]], dtype=i32)},
        "bonds": {"bond_index": torch.tensor([[0, 1, 4, 4, 5, 6], [1, 2, 5, 7, 6, 7]], dtype=i32),
                  "bond_order": torch.tensor([1, 1, 1, 1, 2, 1], dtype=u8),
                  "bond_length": torch.tensor([1.5, 1.4, 1.51, 1.52, 1.33, 1.53], dtype=torch.float64),
                  "bond_graph": torch.tensor([0, 0, 3, 3, 3, 3]), "fragment": torch.tensor([0, 0, 0, 0, 0, 0, 0, 0], dtype=i32),
                  "graph_counts": torch.tensor([[3, 2, 2, 1, 3, 0], [0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 0], [4, 4, 5, 1, 4, 1]], dtype=i32)},
        "rings": {"atom_ring_min": torch.tensor([0, 0, 0, 0, 255, 255, 255, 255], dtype=u8),
                  "graph_counts": torch.tensor([[3, 2] + [0] * 11, [0] * 13, [1] + [0] * 12, [4, 4] + [-1] * 10 + [2]], dtype=i32)},
        "aromatic": {"aromatic_atom": torch.tensor([True, True, True, False, False, False, False, False]),
                     "in_closure": torch.tensor([True, True, True, False, False, False, False, False]),
                     "aromatic_bond": torch.tensor([True, False, False, False, False, False]),
                     "bond_type": torch.tensor([4, 1, 255, 255, 255, 255], dtype=u8),
                     "graph_counts": torch.tensor([[3, 2, 1, 1, 2, 3, 3, 1, 0, 0], [0] * 10, [1] + [0] * 9, [4, 4] + [-1] * 7 + [8]], dtype=i32)},
        "distributions": {"angle_index": torch.tensor([[0, 4, 5], [1, 5, 6], [2, 6, 7]], dtype=i32),
                          "angle_cos": torch.tensor([0.0, -1.0, 1.0], dtype=torch.float64),
                          "angle_bin": torch.tensor([45, 89, 0], dtype=u8), "angle_type": torch.tensor([10, 20, 30], dtype=torch.int16),
                          "angle_graph": torch.tensor([0, 3, 3]),
                          "graph_counts": torch.tensor([[3, 2, 1, 0, 0], [0] * 5, [1, 0, 0, 0, 0], [4, 4, 2, 0, 0]], dtype=i32),
                          "pair_hist": pair_hist(), "bond_bin": torch.tensor([50, 60, 80, 80, 40, 80], dtype=u8),
                          "bond_type": torch.tensor([C_AROMATIC_C, C_C, C_C, C_C, C_DOUBLE_C, C_C], dtype=torch.int16),
                          "bond_hist_index": torch.tensor([[0, 0, 3, 3], [C_C, C_AROMATIC_C, C_C, C_DOUBLE_C], [60, 50, 80, 40]], dtype=i32),
                          "bond_hist_count": torch.tensor([1, 1, 3, 1], dtype=i32),
                          "angle_hist_index": torch.tensor([[0, 3, 3], [C_C_C, C_C_C, C_C_C], [45, 0, 89]], dtype=i32),
                          "angle_hist_count": torch.tensor([1, 1, 1], dtype=i32)}}


def pair_hist():
    h = torch.zeros(4, 2, 101, dtype=torch.int32)
    h[0, 0, 13], h[0, 0, 25], h[0, 1, 70] = 2, 1, 1
    h[3, 0, 12], h[3, 0, 17] = 4, 2
    return h


def samples():
    """what split_samples leaves of a sample, as far as the reports read it; the single atom is selenium, which no SDF record takes"""
    atoms = ([6, 6, 6], [], [34], [6, 6, 6, 6])
    return [{"pos": torch.arange(3.0 * len(a)).reshape(-1, 3) + 0.25 * g, "atom": list(a)} for g, a in enumerate(atoms)]


def hist(n, cells):
    out = [0] * n
    for k, v in cells.items():
        out[k] = v
    return out


def same(t, dtype, values):
    want = torch.tensor(values, dtype=dtype)
    return t.dtype == dtype and t.shape == want.shape and torch.equal(t, want)


def test_ranges():
    assert ranges(torch.tensor([3, 0, 1, 4], dtype=torch.int32)) == [(0, 3), (3, 3), (3, 4), (4, 8)]
    assert ranges(torch.tensor([], dtype=torch.int32)) == []


def test_annotate_per_sample_fields():
    smp = samples()
    SampleReports(ALL).annotate(smp, reports())
    s0, s1, s2, s3 = smp
    i32, u8, i64, f64 = torch.int32, torch.uint8, torch.int64, torch.float64
    # geometry
    assert [same(s["nr_bonds"], i32, v) for s, v in zip(smp, ([1, 2, 1], [], [0], [2, 2, 3, 3]))] == [True] * 4
    assert [s["atom_stable"].tolist() for s in smp] == [[True, False, True], [], [False], [True] * 4]
    assert [s["inter_clash"].tolist() for s in smp] == [[False, False, True], [], [False], [False] * 4]
    assert [s["intra_clash_table_bonds"].tolist() for s in smp] == [[False] * 3, [], [True], [False] * 4]
    assert all(s[k].dtype == torch.bool for s in smp for k in ("atom_stable", "inter_clash", "intra_clash_table_bonds"))
    assert [s["mol_stable"] for s in smp] == [False, True, False, True]
    # bonds: rows become ligand-local
    assert same(s0["bond_index"], i32, [[0, 1], [1, 2]]) and same(s3["bond_index"], i32, [[0, 0, 1, 2], [1, 3, 2, 3]])
    assert all(s["bond_index"].dtype == i32 and tuple(s["bond_index"].shape) == (2, 0) for s in (s1, s2))
    assert [same(s["bond_order"], u8, v) for s, v in zip(smp, ([1, 1], [], [], [1, 1, 2, 1]))] == [True] * 4
    assert [same(s["bond_length"], f64, v) for s, v in zip(smp, ([1.5, 1.4], [], [], [1.51, 1.52, 1.33, 1.53]))] == [True] * 4
    assert [same(s["fragment"], i32, v) for s, v in zip(smp, ([0, 0, 0], [], [0], [0, 0, 0, 0]))] == [True] * 4
    assert [s["n_fragments"] for s in smp] == [1, 0, 1, 1] and [s["connected"] for s in smp] == [True, False, True, True]
    # rings: graph 3 was not evaluated
    assert [same(s["ring_sizes"], i64, v) for s, v in zip(smp, ([0] * 7, [0] * 7, [0] * 7, [-1] * 7))] == [True] * 4
    assert [same(s["atom_ring_min"], u8, v) for s, v in zip(smp, ([0, 0, 0], [], [0], [255] * 4))] == [True] * 4
    assert [s["n_rings_larger"] for s in smp] == [0, 0, 0, -1] and [s["ring_status"] for s in smp] == [0, 0, 0, 2]
    # aromatic: aligned with the bond list; graph 3 was not evaluated
    assert [s["aromatic_atom"].tolist() for s in smp] == [[True] * 3, [], [False], [False] * 4]
    assert [s["aromatic_bond"].tolist() for s in smp] == [[True, False], [], [], [False] * 4]
    assert all(s[k].dtype == torch.bool for s in smp for k in ("aromatic_atom", "aromatic_bond"))
    assert [same(s["bond_type"], u8, v) for s, v in zip(smp, ([4, 1], [], [], [255] * 4))] == [True] * 4
    assert [s["n_aromatic_rings"] for s in smp] == [1, 0, 0, -1] and [s["aromatic_status"] for s in smp] == [0, 0, 0, 8]
    # distributions: three angles, one in graph 0 and two in graph 3
    assert same(s0["angle_index"], i32, [[0], [1], [2]]) and same(s3["angle_index"], i32, [[0, 1], [1, 2], [2, 3]])
    assert all(s["angle_index"].dtype == i32 and tuple(s["angle_index"].shape) == (3, 0) for s in (s1, s2))
    assert [same(s["angle_cos"], f64, v) for s, v in zip(smp, ([0.0], [], [], [-1.0, 1.0]))] == [True] * 4
    assert [same(s["angle_deg"], f64, v) for s, v in zip(smp, ([90.0], [], [], [180.0, 0.0]))] == [True] * 4
    assert [same(s["angle_type"], torch.int16, v) for s, v in zip(smp, ([10], [], [], [20, 30]))] == [True] * 4
    assert [s["distribution_status"] for s in smp] == [0, 0, 0, 0]
    # the fields are copies: the batch's tensors can go
    rep = reports()
    smp = samples()
    SampleReports(ALL).annotate(smp, rep)
    rep["bonds"]["bond_order"].fill_(9), rep["rings"]["atom_ring_min"].fill_(9), rep["aromatic"]["bond_type"].fill_(9)
    assert smp[3]["bond_order"].tolist() == [1, 1, 2, 1] and smp[3]["atom_ring_min"].tolist() == [255] * 4
    assert smp[0]["bond_type"].tolist() == [4, 1]


def test_a_dependency_is_used_and_not_written():
    smp = samples()
    SampleReports(("aromatic", "sdf")).annotate(smp, {k: v for k, v in reports().items() if k in ("aromatic", "bonds")})
    assert all(sorted(s) == sorted(["pos", "atom", "aromatic_atom", "aromatic_bond", "bond_type", "n_aromatic_rings", "aromatic_status"])
               for s in smp)
    smp = samples()
    SampleReports(("sdf",)).annotate(smp, {"bonds": reports()["bonds"]})
    assert all(sorted(s) == ["atom", "pos"] for s in smp)


def test_pocket_counts():
    rep, r = reports(), SampleReports(ALL)
    first, second = r.pocket_counts(rep, 0, 2), r.pocket_counts(rep, 2, 4)           # num_samples = 2
    assert list(first) == list(second) == ["distributions", "aromatic", "rings", "bonds", "geometry"]     # the order they are saved in
    assert first["geometry"] == {"n_mol": 2, "n_atoms": 3, "n_stable": 2, "n_mol_stable": 1, "n_inter_clash_atoms": 1,
                                 "n_intra_clash_atoms": 0, "n_clash_mol": 1, "n_protein_atoms_without_radius": 2}
    assert second["geometry"] == {"n_mol": 2, "n_atoms": 5, "n_stable": 4, "n_mol_stable": 1, "n_inter_clash_atoms": 0,
                                  "n_intra_clash_atoms": 1, "n_clash_mol": 0, "n_protein_atoms_without_radius": 0}
    assert first["bonds"] == {"n_mol": 2, "n_atoms": 3, "n_bonds": 2, "n_connected_mol": 1, "n_largest_fragment_atoms": 3, "n_fragments": 1,
                              "n_cycles": 0}
    assert second["bonds"] == {"n_mol": 2, "n_atoms": 5, "n_bonds": 4, "n_connected_mol": 2, "n_largest_fragment_atoms": 5,
                               "n_fragments": 2, "n_cycles": 1}
    no_rings = {k: 0 for k in G.RING_COUNT_KEYS}
    assert first["rings"] == {**no_rings, "n_mol": 2, "n_mol_evaluated": 2, "n_atoms": 3}
    assert second["rings"] == {**no_rings, "n_mol": 2, "n_mol_evaluated": 1, "n_mol_over_limit": 1, "n_atoms": 1}
    assert first["aromatic"] == {"n_mol": 2, "n_mol_evaluated": 2, "n_mol_over_limit": 0, "n_atoms": 3, "n_bonds": 2, "n_cycles56": 1,
                                 "n_aromatic_cycles": 1, "n_flagged": 2, "n_closure": 3, "n_aromatic_atoms": 3, "n_aromatic_bonds": 1,
                                 "n_unsupported": 0, "n_aromatic_mol": 1}
    assert second["aromatic"] == {**{k: 0 for k in G.AROMATIC_COUNT_KEYS}, "n_mol": 2, "n_mol_evaluated": 1, "n_mol_over_limit": 1,
                                  "n_atoms": 1}
    assert first["distributions"] == {
        "counts": {"n_mol": 2, "n_mol_over_limit": 0, "n_atoms": 3, "n_bonds": 2, "n_angles": 1, "n_degenerate_angles": 0},
        "pair_hist": [hist(101, {13: 2, 25: 1}), hist(101, {70: 1})],
        "bond_hist": {"6-6": hist(120, {60: 1}), "6:6": hist(120, {50: 1})}, "angle_hist": {"6-6-6": hist(91, {45: 1})}}
    assert second["distributions"] == {
        "counts": {"n_mol": 2, "n_mol_over_limit": 0, "n_atoms": 5, "n_bonds": 4, "n_angles": 2, "n_degenerate_angles": 0},
        "pair_hist": [hist(101, {12: 4, 17: 2}), hist(101, {})],
        "bond_hist": {"6-6": hist(120, {80: 3}), "6=6": hist(120, {40: 1})}, "angle_hist": {"6-6-6": hist(91, {0: 1, 89: 1})}}
    # without --aromatic the histograms are keyed by the three orders: the same dict is then one of another vocabulary
    assert SampleReports(("distributions",)).n_orders == 3 and r.n_orders == 4


def test_sdf_text():
    rep, smp, r = reports(), samples(), SampleReports(("aromatic", "sdf"))
    files = [r.pocket_files(f"pocket_{pid:05d}", smp[g0:g0 + 2], rep, g0) for pid, g0 in ((7, 0), (8, 2))]
    assert [[name for name, _ in f] for f in files] == [["pocket_00007.sdf"], ["pocket_00008.sdf"]]
    chain, empty = files[0][0][1].split("$$$$\n")[:2]
    assert files[0][0][1].count("$$$$\n") == 2 and files[1][0][1].count("$$$$\n") == 1        # selenium is left out of its file
    assert (r.sdf_written, r.sdf_left_out) == (3, 1)
    lines = chain.split("\n")
    assert lines[0] == "pocket_00007_sample_0" and lines[3] == "  3  2  0  0  0  0  0  0  0  0999 V2000"
    assert lines[4] == "    0.0000    1.0000    2.0000 C   0  0  0  0  0  0  0  0  0  0  0  0"
    assert lines[7:10] == ["  1  2  4  0", "  2  3  1  0", "M  END"]                # the aromatic report's types
    lines = empty.split("\n")
    assert lines[0] == "pocket_00007_sample_1" and lines[3] == "  0  0  0  0  0  0  0  0  0  0999 V2000" and lines[4] == "M  END"
    lines = files[1][0][1].split("\n")
    assert lines[0] == "pocket_00008_sample_1" and lines[3] == "  4  4  0  0  0  0  0  0  0  0999 V2000"
    assert lines[8:13] == ["  1  2  1  0", "  1  4  1  0", "  2  3  2  0", "  3  4  1  0", "M  END"]   # not evaluated: the bond orders
    # without --aromatic every record carries the orders; without --sdf there is no file
    plain = SampleReports(("sdf",)).pocket_files("pocket_00007", smp[0:2], {"bonds": rep["bonds"]}, 0)[0][1].split("\n")
    assert plain[7:9] == ["  1  2  1  0", "  2  3  1  0"]
    assert SampleReports(("bonds",)).pocket_files("pocket_00007", smp[0:2], rep, 0) == []


def test_finish_on_one_rank(tmp_path, capsys):
    rep, r = reports(), SampleReports(ALL)
    for g0 in (0, 2):
        r.pocket_files("p", samples()[g0:g0 + 2], rep, g0)
        r.pocket_counts(rep, g0, g0 + 2)
    r.finish(str(tmp_path), 0, torch.device("cpu"))
    want = {"geometry": G.summarise(rep["geometry"]["graph_counts"]), "bonds": G.summarise_bonds(rep["bonds"]["graph_counts"]),
            "rings": G.summarise_rings(rep["rings"]["graph_counts"]), "aromatic": G.summarise_aromatic(rep["aromatic"]["graph_counts"]),
            "distributions": G.summarise_distributions(rep["distributions"], n_orders=4)}
    for name, summary in want.items():
        with open(tmp_path / f"{name}_summary.json") as f:
            assert f.read() == json.dumps(summary, indent=1, sort_keys=True), name
    assert want["bonds"]["counts"]["n_bonds"] == 6 and want["distributions"]["counts"]["n_angles"] == 3
    printed = capsys.readouterr().out.split("\n")
    assert [line.split(":")[0] for line in printed[:6]] == ["geometry", "bonds", "rings", "distributions", "aromatic", "sdf"]
    assert printed[1] == ("bonds: connected_mol_ratio 0.7500, largest_fragment_atom_ratio 1.0000, fragments_per_mol 0.7500, "
                          "cycles_per_mol 0.2500, bonds_per_atom 0.7500 (4 molecules, 6 bonds)")
    assert printed[3] == "distributions: 4 molecules, 6 bonds, 3 angles, All_12A modal bin centre 1.394 A, n_mol_over_limit 0"
    assert printed[4].endswith("(3 of 4 molecules evaluated, 1 aromatic rings)")
    assert printed[5].startswith("sdf: 3 records written, 1 samples left out")
    # another rank writes and prints nothing
    r.finish(str(tmp_path / "none"), 1, torch.device("cpu"))
    assert not (tmp_path / "none").exists() and capsys.readouterr().out == ""
