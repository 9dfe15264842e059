"""Distributions of sampled ligands (cbgbench_amd/geometry.py, include/cbgx.h cbgx_ligand_pair_hist / cbgx_ligand_angles) without a GPU:
the numpy model of the definition (tests/distributions_model.py) against the reference's pair-length and bond-length profiles bit for
bit and against the arccos route for the angles, lattice cases with bins derived by hand, the type codes, the summaries and the
Jensen-Shannon distance, and the C ABI's argument checks."""
import ctypes
import importlib
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from cbgbench_amd import _native, geometry as G
from tests import bonds_model as BM
from tests import distributions_model as DM
from tests import geometry_model as GM
from tests.test_geometry import molecules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.fixture(scope="module")
def ref_length():
    """the reference's eval_bond_length, imported through its tree on sys.path with an empty stand-in for repo.utils.molecule.constants
    (its only import there is RDKit); sys.path and sys.modules are put back"""
    if not os.path.exists(os.path.join(REF, "repo", "tools", "geometry", "eval_bond_length.py")):
        pytest.skip("needs the reference tree at " + REF)
    before = set(sys.modules)
    sys.path.insert(0, REF)
    sys.modules["repo.utils.molecule.constants"] = types.ModuleType("repo.utils.molecule.constants")
    try:
        try:
            return importlib.import_module("repo.tools.geometry.eval_bond_length")
        except ImportError as e:
            pytest.skip(f"the reference's eval_bond_length.py does not import here: {e}")
    finally:
        sys.path.remove(REF)
        for name in set(sys.modules) - before:
            if name == "repo" or name.startswith("repo."):
                del sys.modules[name]


@pytest.fixture(scope="module")
def mols():
    return [(x, z) for x, z, _, _ in molecules()]


# ---- the model against the reference -------------------------------------------------------------------------------------------------
def test_pair_profiles_equal_the_reference_bit_for_bit(ref_length, mols):
    ea, ec = G.default_pair_edges()
    counts = sum(DM.pair_hist(x, z, ea, ec).astype(np.int64) for x, z in mols)
    pooled = []
    for x, z in mols:
        pooled += ref_length.pair_distance_from_pos_v(x.astype(np.float64), z)
    profile = ref_length.get_pair_length_profile(pooled)
    assert np.array_equal(ea, np.linspace(0, 12, 100)) and np.array_equal(ec, np.linspace(0, 2, 100))
    for f, key in enumerate(G.PAIR_FAMILIES):
        assert profile[key].shape == (101,) and np.array_equal(counts[f] / counts[f].sum(), profile[key]), key
    # the input reaches what it should: a full and a sparse family, and pairs beyond the cutoff
    assert counts[0].sum() == 23556 and counts[1].sum() == 849 and len(pooled) - counts[0].sum() == 19
    assert (counts[0] > 0).sum() == 99 and (counts[1] > 0).sum() == 83


def test_bond_length_profiles_equal_the_reference(ref_length, mols):
    edges = G.default_bond_edges()
    assert np.array_equal(edges, ref_length.DISTANCE_BINS) and len(edges) == 119
    listed, mine = [], {}
    for x, z in mols:
        b = BM.graph_bonds(x, z)
        code = GM._codes(z, GM.tables()["elements"])
        types_, bins = DM.bond_types(b["bond_index"], b["bond_order"], code), DM.bond_bins(b["bond_length"], edges)
        for (i, j), o, d, t, k in zip(b["bond_index"].T.tolist(), b["bond_order"].tolist(), b["bond_length"].tolist(), types_.tolist(),
                                      bins.tolist()):
            listed.append(((int(z[j]), int(z[i]), o), d))          # (either order of the atoms: the reference sorts them)
            mine.setdefault(t, np.zeros(120, np.int64))[k] += 1
    profile = ref_length.get_bond_length_profile(listed)
    assert {ref_length._bond_type_str(k) for k in profile} == {G.bond_type_string(t) for t in mine} and len(mine) > 20
    for t, h in mine.items():
        a1, o, a2 = re.fullmatch(r"(\d+)([-=#])(\d+)", G.bond_type_string(t)).groups()
        assert np.array_equal(h / h.sum(), profile[(int(a1), int(a2), "-=#".index(o) + 1)]), G.bond_type_string(t)
    assert {o for (_, _, o), _ in listed} == {1, 2, 3}


def test_angle_bins_equal_the_arccos_route(mols):
    cos_edges, edges_deg = G.default_cos_edges(), np.arange(0, 180, 2)
    n_angles, n_degenerate, n_guarded, kinds = 0, 0, 0, set()
    for x, z in mols:
        r = DM.graph_angles(x, z, cos_edges)
        assert r["counts"][4] == 0
        ok = r["angle_bin"] != DM.DEGENERATE
        theta = np.degrees(np.arccos(r["angle_cos"][ok]))
        clear = np.abs(theta[:, None] - edges_deg[None, :]).min(1) > 1e-9
        assert np.array_equal(r["angle_bin"][ok][clear], np.searchsorted(edges_deg, theta[clear]))
        n_angles, n_degenerate, n_guarded = n_angles + len(ok), n_degenerate + int((~ok).sum()), n_guarded + int((~clear).sum())
        kinds |= set(r["angle_type"].tolist())
        a, c, b = r["angle_index"].astype(np.int64)
        assert (a < b).all() and np.array_equal(np.lexsort((b, a, c)), np.arange(len(a)))      # (c, a, b) order
    # the guard leaves nothing out on this input.  504 canonical types; the reference, which appends every angle under both
    # orientations, would list 931 (77 of the 504 read the same from either end)
    both = {f(t) for t in kinds for f in (lambda t: (t // 576, t // 192 % 3, t // 24 % 8, t // 8 % 3, t % 8),
                                          lambda t: (t % 8, t // 8 % 3, t // 24 % 8, t // 192 % 3, t // 576))}
    assert n_guarded == 0 and n_degenerate == 0 and n_angles == 27699 and len(kinds) == 504 and len(both) == 931


# ---- lattice cases, bins by hand -----------------------------------------------------------------------------------------------------
def lattice():
    """carbons on exact coordinates (also a graph of the GPU test):
      0 - 3   a centre with partners at +x, -x, +y, 1.5 A away: one angle of 180 and two of 90 degrees
      4 - 7   the FCC points (0,0,0), (1,1,0), (1,0,1), (0,1,1) (+ 20 in x): a regular tetrahedron of edge sqrt(2), twelve angles of 60
      8 - 10  two coincident atoms and a third 1.5 A away: two degenerate angles and one of 0 degrees
      11 - 13 an atom 4 A above atom 0 (All edge 33 exactly), one 12 A from it (excluded), one 2 A from that (the CC cutoff exactly)"""
    x = [[0, 0, 0], [1.5, 0, 0], [-1.5, 0, 0], [0, 1.5, 0],
         [20, 0, 0], [21, 1, 0], [21, 0, 1], [20, 1, 1],
         [0, 20, 0], [0, 20, 0], [1.5, 20, 0],
         [0, 0, 4], [0, 12, 4], [0, 14, 4]]
    return np.array(x, np.float32), np.full(len(x), 6)


def test_lattice_angles():
    x, z = lattice()
    ce = G.default_cos_edges()
    # hand-derived bins = the number of edges 0, 2, ..., 178 strictly less than the angle: 180 -> 90, 90 -> 45, 60 -> 30, 0 -> 0
    assert ce[0] == 1.0 and ce[30] == 0.5 and ce[45] == 0.0 and ce[60] == -0.5 and len(ce) == 90 and (np.diff(ce) < 0).all()
    r = DM.graph_angles(x[:4], z[:4], ce)
    assert r["angle_index"].T.tolist() == [[1, 0, 2], [1, 0, 3], [2, 0, 3]]
    assert r["angle_cos"].tolist() == [-1.0, 0.0, 0.0] and r["angle_bin"].tolist() == [90, 45, 45]
    r = DM.graph_angles(x[4:8], z[4:8], ce)
    assert r["angle_index"].shape == (3, 12) and (r["angle_cos"] == 0.5).all() and (r["angle_bin"] == 30).all()
    r = DM.graph_angles(x[8:11], z[8:11], ce)
    assert r["angle_index"].T.tolist() == [[1, 0, 2], [0, 1, 2], [0, 2, 1]]
    assert np.isnan(r["angle_cos"][:2]).all() and r["angle_cos"][2] == 1.0 and r["angle_bin"].tolist() == [255, 255, 0]
    assert r["counts"].tolist() == [3, 3, 3, 2, 0]
    whole = DM.graph_angles(x, z, ce)
    assert whole["counts"].tolist() == [14, 12, 18, 2, 0]
    assert set(whole["angle_type"].tolist()) == {G.angle_type_code(1, 1, 1, 1, 1), G.angle_type_code(1, 3, 1, 1, 1)}


def test_lattice_pair_distances():
    ea, ec = G.default_pair_edges()
    assert ea[0] == 0.0 and ea[33] == 4.0 and ea[99] == 12.0 and ec[99] == 2.0
    at = lambda *pts: (np.array(pts, np.float32), np.full(len(pts), 6))
    one = lambda h: [(f, int(b)) for f, b in zip(*np.nonzero(h))]
    assert one(DM.pair_hist(*at([0, 0, 0], [0, 0, 0]), ea, ec)) == [(0, 0), (1, 0)]           # distance 0: no edge is less
    assert one(DM.pair_hist(*at([0, 0, 0], [0, 0, 4]), ea, ec)) == [(0, 33)]                  # exactly edge 33: 33 edges are less
    assert one(DM.pair_hist(*at([0, 0, 4], [0, 12, 4]), ea, ec)) == []                        # exactly the last edge: excluded
    assert one(DM.pair_hist(*at([0, 12, 4], [0, 14, 4]), ea, ec)) == [(0, 17)]                # 2 A: in All (16.5 steps), not in CC
    x, z = lattice()
    h = DM.pair_hist(x, z, ea, ec)
    assert h.shape == (2, 101) and h[0].sum() == int((GM.distances(x, x)[np.triu_indices(14, 1)] < 12).sum()) < 91 and h[0, 0] == 1 and h[0, 33] == 1 and h[1, 0] == 1
    z2 = z.copy()
    z2[0] = 34                                                                                 # unknown element: in All, not in CC
    h2 = DM.pair_hist(x, z2, ea, ec)
    assert np.array_equal(h2[0], h[0]) and h2[1].sum() == h[1].sum() - int((GM.distances(x[:1], x[1:]) < 2).sum())


def test_an_over_limit_graph_has_a_status_and_no_angles():
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 0.5, size=(40, 3)).astype(np.float32)
    r = DM.graph_angles(x, np.full(40, 6), G.default_cos_edges())
    assert r["counts"].tolist() == [40, 780, 0, 0, DM.TOO_MANY] and r["angle_index"].shape == (3, 0)
    assert 40 * (39 * 38 // 2) == 29640 > G.MAX_ANGLES_PER_GRAPH


# ---- type codes ----------------------------------------------------------------------------------------------------------------------
def test_type_codes_and_strings():
    assert GM.tables()["elements"].tolist() == list(G._ELEMENTS)
    # O=C-C seen from either end is one code, and the double bond stays with the oxygen
    assert G.angle_type_code(3, 2, 1, 1, 1) == G.angle_type_code(1, 1, 1, 2, 3)
    assert G.angle_type_string(G.angle_type_code(3, 2, 1, 1, 1)) == "6-6=8"
    assert G.angle_type_code(1, 2, 1, 1, 1) == G.angle_type_code(1, 1, 1, 2, 1) and G.angle_type_string(G.angle_type_code(1, 2, 1, 1, 1)) == "6-6=6"
    seen = set()
    for ca in range(8):
        for oa in (1, 2, 3):
            for cc in range(8):
                for ob in (1, 2, 3):
                    for cb in range(8):
                        t = G.angle_type_code(ca, oa, cc, ob, cb)
                        assert 0 <= t < G.N_ANGLE_TYPES and t == G.angle_type_code(cb, ob, cc, oa, ca)
                        assert int(DM.angle_types([ca], [oa], [cc], [ob], [cb])[0]) == t
                        kind, canon = G._parse_type(G.angle_type_string(t))
                        assert kind == "bond_angle" and canon == G.angle_type_string(t)
                        e = G._ELEMENTS
                        assert G._parse_type((e[ca], oa, e[cc], ob, e[cb])) == ("bond_angle", canon)
                        seen.add(t)
    assert len(seen) == 8 * (24 * 25 // 2)                                                     # unordered end pairs x centres
    for a in range(8):
        for o in (1, 2, 3):
            for b in range(8):
                t = G.bond_type_code(a, o, b)
                assert 0 <= t < G.N_BOND_TYPES and t == G.bond_type_code(b, o, a) and t // 8 % 8 <= t % 8
                lo, hi = sorted((G._ELEMENTS[a], G._ELEMENTS[b]))
                assert G.bond_type_string(t) == f"{lo}{'-=#'[o - 1]}{hi}" and G._parse_type(G.bond_type_string(t)) == ("bond_length", G.bond_type_string(t))
    assert G._parse_type((8, 6, 2)) == ("bond_length", "6=8") and G._parse_type("8=6") == ("bond_length", "6=8")
    assert G._parse_type("6:6")[0] is None and G._parse_type((6, 6, 4))[0] is None and G._parse_type("6-35")[0] is None
    assert G._parse_type("CC_2A") == ("pair_length", "CC_2A")


# ---- summaries and the Jensen-Shannon distance ---------------------------------------------------------------------------------------
def _hand_made():
    """two graphs: a propene-like O=C-C with its one angle, and a collapsed graph over the angle limit"""
    pair = np.zeros((2, 2, 101), np.int32)
    pair[0, 0, [10, 12, 20]] = 1
    pair[0, 1, 75] = 1
    pair[1, 0, 3] = 700
    pair[1, 0, 4] = 80
    pair[1, 1, 30] = 780
    cc1, co2 = G.bond_type_code(1, 1, 1), G.bond_type_code(1, 2, 3)
    return {"graph_counts": np.array([[3, 2, 1, 0, 0], [40, 780, 0, 0, 1]], np.int32), "pair_hist": pair,
            "bond_hist_index": np.array([[0, 0, 1, 1], [cc1, co2, cc1, cc1], [84, 22, 0, 1]], np.int32),
            "bond_hist_count": np.array([1, 1, 500, 280], np.int32),
            "angle_hist_index": np.array([[0], [G.angle_type_code(3, 2, 1, 1, 1)], [60]], np.int32),
            "angle_hist_count": np.array([1], np.int32)}


def test_summaries_against_hand_computed_counts():
    d = _hand_made()
    totals = G.distribution_totals(d)
    assert totals.dtype == np.int64 and totals.shape == (G.distribution_totals_length(),) == (6 + 202 + 192 * 120 + 4608 * 91,)
    c = G.distribution_counts(totals)
    assert c["counts"] == {"n_mol": 2, "n_mol_over_limit": 1, "n_atoms": 43, "n_bonds": 782, "n_angles": 1, "n_degenerate_angles": 0}
    assert sorted(c["bond_hist"]) == ["6-6", "6=8"] and sorted(c["angle_hist"]) == ["6-6=8"]
    assert c["bond_hist"]["6-6"][:2] == [500, 280] and c["bond_hist"]["6-6"][84] == 1 and sum(c["bond_hist"]["6-6"]) == 781
    assert c["angle_hist"]["6-6=8"][60] == 1 and sum(c["angle_hist"]["6-6=8"]) == 1
    assert np.array(c["pair_hist"]).shape == (2, 101) and c["pair_hist"][0][3] == 700 and c["pair_hist"][1][30] == 780
    s = G.summarise_distributions(d)
    assert set(s) == {"counts", "pair_length", "bond_length", "bond_angle"} and s["counts"] == c["counts"]
    assert s["pair_length"]["All_12A"]["count"] == 783 and s["pair_length"]["All_12A"]["distribution"][3] == 700 / 783
    assert s["pair_length"]["CC_2A"]["count"] == 781 and s["pair_length"]["CC_2A"]["distribution"][75] == 1 / 781
    assert s["bond_length"]["6-6"]["count"] == 781 and s["bond_length"]["6-6"]["distribution"][1] == 280 / 781
    assert s["bond_length"]["6=8"] == {"count": 1, "distribution": [0.0] * 22 + [1.0] + [0.0] * 97}
    assert s["bond_angle"]["6-6=8"] == {"count": 1, "distribution": [0.0] * 60 + [1.0] + [0.0] * 30}
    # per-pocket slices add up to the whole: what sample_cli sums over pockets and ranks
    parts = G.distribution_totals(d, graphs=(0, 1)) + G.distribution_totals(d, graphs=(1, 2))
    assert np.array_equal(parts, totals)
    first = G.distribution_counts(G.distribution_totals(d, graphs=(0, 1)))
    assert first["counts"]["n_mol_over_limit"] == 0 and first["bond_hist"]["6-6"][84] == 1 and sum(first["bond_hist"]["6-6"]) == 1
    assert G.summarise_distributions({k: torch.from_numpy(v) for k, v in d.items()}) == s
    # nothing at all: no types, and ratios over nothing are nan
    empty = G.summarise_distribution_totals(np.zeros(G.distribution_totals_length(), np.int64))
    assert empty["bond_length"] == {} and empty["bond_angle"] == {} and empty["counts"]["n_mol"] == 0
    assert all(np.isnan(empty["pair_length"][k]["distribution"]).all() and empty["pair_length"][k]["count"] == 0 for k in G.PAIR_FAMILIES)
    with pytest.raises(ValueError):
        G.distribution_counts(totals[:-1])


def test_distribution_jsd_equals_scipy():
    from scipy.spatial.distance import jensenshannon
    rng = np.random.default_rng(11)
    for n in (2, 6, 91, 101, 120):
        for _ in range(20):
            p, q = rng.uniform(size=n), rng.uniform(size=n)
            p[rng.uniform(size=n) < 0.3] = 0.0                      # bins only one side fills, and bins neither fills
            q[rng.uniform(size=n) < 0.3] = 0.0
            p[0], q[0] = 1.0, 0.5
            assert abs(G.distribution_jsd(p, q) - jensenshannon(p, q)) <= 1e-15, n
            assert abs(G.distribution_jsd(5 * p, q) - jensenshannon(p, q)) <= 1e-15
    assert G.distribution_jsd([1, 0], [1, 0]) == 0.0 and abs(G.distribution_jsd([1, 0], [0, 1]) - np.sqrt(np.log(2))) <= 1e-15
    assert np.isnan(G.distribution_jsd([0, 0], [1, 0]))
    six = rng.uniform(size=6)
    assert abs(G.distribution_jsd(six, six[::-1]) - G.ring_jsd(six, six[::-1])) <= 1e-15
    with pytest.raises(ValueError):
        G.distribution_jsd([1, 2], [1, 2, 3])


def test_jsd_against():
    s = G.summarise_distributions(_hand_made())
    rng = np.random.default_rng(3)
    ref = {"All_12A": rng.uniform(size=101), "8=6-6": rng.uniform(size=91), (6, 1, 6, 2, 8): rng.uniform(size=91),
           "6-6": rng.uniform(size=120), (8, 6, 2): rng.uniform(size=120), (6, 6, 4): rng.uniform(size=120), "6:6-6": rng.uniform(size=91),
           "7-7": rng.uniform(size=120)}
    out = G.jsd_against(s, ref)
    assert set(out) == {"JSD_All_12A", "JSD_8=6-6", "JSD_6-6=8", "JSD_6-6", "JSD_8=6", "JSD_6?6", "JSD_6:6-6", "JSD_7-7", "not_evaluated"}
    angle = s["bond_angle"]["6-6=8"]["distribution"]
    assert out["JSD_8=6-6"] == G.distribution_jsd(angle, ref["8=6-6"]) and out["JSD_6-6=8"] == G.distribution_jsd(angle, ref[(6, 1, 6, 2, 8)])
    assert out["JSD_All_12A"] == G.distribution_jsd(s["pair_length"]["All_12A"]["distribution"], ref["All_12A"])
    assert out["JSD_8=6"] == G.distribution_jsd(s["bond_length"]["6=8"]["distribution"], ref[(8, 6, 2)]) > 0
    assert out["JSD_6?6"] is None and out["JSD_6:6-6"] is None and out["JSD_7-7"] is None
    assert "aromatic" in out["not_evaluated"]["JSD_6?6"] and "aromatic" in out["not_evaluated"]["JSD_6:6-6"]
    assert "no such type" in out["not_evaluated"]["JSD_7-7"] and set(out["not_evaluated"]) == {"JSD_6?6", "JSD_6:6-6", "JSD_7-7"}
    with pytest.raises(ValueError, match="bins"):
        G.jsd_against(s, {"6-6": np.ones(7)})


# ---- no CPU path ---------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    x, z, b = torch.zeros(3, 3), torch.tensor([6, 6, 6]), torch.zeros(3, dtype=torch.long)
    bonds = {"bond_index": torch.tensor([[0, 0], [1, 2]], dtype=torch.int32), "bond_order": torch.ones(2, dtype=torch.uint8)}
    with pytest.raises(_native.NativeError):
        G.ligand_angles(x, z, b, 1, bonds)
    with pytest.raises(_native.NativeError):
        G.ligand_pair_hist(x, z, b, 1)
    with pytest.raises(_native.NativeError):
        G.batch_distributions({"num_graphs": 1}, x, torch.ones(3, dtype=torch.long), b, "basic")


def test_sample_cli_distributions_needs_the_gpu():
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    with pytest.raises(SystemExit, match="--distributions runs on the GPU"):
        sample_cli.main(["--config", cfg, "--device", "cpu", "--distributions", "--random_init", "--synthetic", "1"])


def test_edges_are_checked():
    assert len(G.default_cos_edges()) == 90 and len(G.default_bond_edges()) == 119
    with pytest.raises(ValueError, match="increasing"):
        G._edges([0.0, 1.0, 1.0], "edges_all", 255)
    with pytest.raises(ValueError, match="decreasing"):
        G._edges([1.0, 0.5, 0.75], "cos_edges", 254, decreasing=True)
    with pytest.raises(ValueError, match="at most 254"):
        G._edges(np.linspace(1, -1, 255), "cos_edges", 254, decreasing=True)
    assert G._edges(np.linspace(0, 1, 255), "edges_all", 255).shape == (255,)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_ligand_pair_hist", "cbgx_ligand_angles")


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
        assert "distributions.hip" in [os.path.basename(s) for s in sources(xcheck)]
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    for name, value in (("PAIR_HIST_MAX_EDGES", G.MAX_PAIR_EDGES), ("ANGLES_MAX_EDGES", G.MAX_ANGLE_EDGES),
                        ("ANGLES_MAX_PER_GRAPH", G.MAX_ANGLES_PER_GRAPH), ("ANGLE_BIN_DEGENERATE", G.ANGLE_BIN_DEGENERATE),
                        ("ANGLE_TYPES", G.N_ANGLE_TYPES), ("DISTRIBUTIONS_TOO_MANY_ANGLES", G.DISTRIBUTIONS_TOO_MANY_ANGLES)):
        assert re.search(rf"#define CBGX_{name} {value}\b", hdr), name


ONE = ctypes.c_void_p(16)          # a pointer that is never dereferenced: the argument checks come first


def _pair(lig_ptr=(0, 2, 4), n_lig=4, B=2, x=ONE, z=ONE, ea=ONE, n_ea=100, ec=ONE, n_ec=100, out=ONE):
    lp = None if lig_ptr is None else np.asarray(lig_ptr, np.int32)
    return _native.lib().cbgx_ligand_pair_hist(x, z, None if lp is None else ctypes.c_void_p(lp.ctypes.data), n_lig, B, ea, n_ea, ec, n_ec,
                                               out, None)


def _angles(lig_ptr=(0, 2, 4), n_lig=4, B=2, x=ONE, z=ONE, adj_ptr=ONE, adj_nbr=ONE, adj_order=ONE, n_adj=6, angle_ptr=ONE, n_angles=3,
            ce=ONE, n_ce=90, index=ONE, cos=ONE, bins=ONE, types_=ONE):
    lp = None if lig_ptr is None else np.asarray(lig_ptr, np.int32)
    return _native.lib().cbgx_ligand_angles(x, z, None if lp is None else ctypes.c_void_p(lp.ctypes.data), n_lig, B, adj_ptr, adj_nbr,
                                            adj_order, n_adj, angle_ptr, n_angles, ce, n_ce, index, cos, bins, types_, None)


def test_argument_errors_are_returned_without_a_gpu():
    err = lambda: _native.lib().cbgx_last_error().decode()
    bad = [_pair(B=-1), _pair(n_lig=-1), _pair(n_ea=-1), _pair(n_ec=-1), _pair(lig_ptr=None), _pair(x=None), _pair(z=None), _pair(ea=None),
           _pair(ec=None), _pair(out=None), _pair(n_ea=256), _pair(n_ec=256)]
    assert bad == [-1] * len(bad), bad
    assert _pair(n_ec=-1) == -1 and "negative" in err()
    assert _pair(out=None) == -1 and "NULL" in err()
    assert _pair(n_ea=256) == -1 and "256" in err() and "255" in err()
    # a family without edges needs no array; no graphs: nothing to do, no launch, no error
    assert _pair(ea=None, n_ea=0) == -1 and "lig_ptr" in err()           # (past the checks: what refuses it is the host lig_ptr)
    assert _pair(n_ea=255, n_ec=255) == -1 and "lig_ptr" in err()
    assert _pair(lig_ptr=None, B=0, out=None) == 0 and _pair(lig_ptr=None, n_lig=0, B=0, x=None, z=None, ea=None, n_ea=0, ec=None, n_ec=0,
                                                            out=None) == 0
    assert _pair(lig_ptr=(0, 3, 1028, 1030), n_lig=1030, B=3) == -1 and "graph 1" in err() and "1025" in err()

    bad = [_angles(B=-1), _angles(n_lig=-1), _angles(n_adj=-1), _angles(n_angles=-1), _angles(n_ce=-1), _angles(lig_ptr=None),
           _angles(x=None), _angles(z=None), _angles(adj_ptr=None), _angles(adj_nbr=None), _angles(adj_order=None), _angles(angle_ptr=None),
           _angles(ce=None), _angles(index=None), _angles(cos=None), _angles(bins=None), _angles(types_=None), _angles(n_ce=255)]
    assert bad == [-1] * len(bad), bad
    assert _angles(n_adj=-1) == -1 and "negative" in err()
    assert _angles(types_=None) == -1 and "NULL" in err()
    assert _angles(n_ce=255) == -1 and "255" in err() and "254" in err()
    assert _angles(n_ce=254) == -1 and "lig_ptr" in err()
    assert _angles(lig_ptr=(0, 3, 1028, 1030), n_lig=1030, B=3) == -1 and "graph 1" in err() and "1025" in err()
    # no graphs or no angles: nothing to do, whatever else is NULL
    assert _angles(lig_ptr=None, B=0, adj_ptr=None, angle_ptr=None) == 0
    assert _angles(n_angles=0, index=None, cos=None, bins=None, types_=None) == 0
    assert _angles(n_adj=0, adj_nbr=None, adj_order=None, n_angles=0, index=None, cos=None, bins=None, types_=None, ce=None, n_ce=0) == 0
