"""The comparison with a pocket's native ligand (include/cbgx.h, cbgx_pocket_contacts / cbgx_native_compare) in its numpy / Python-int
model (tests/native_model.py), and the host side of the report: contacts at the threshold, rounding, every status bit, groups of 0 and
1, the reference's formulas, totals over split ranks, the report plumbing on stand-ins for the device entries, refusals and the C ABI.
No GPU."""
import ctypes
import importlib.util
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cbgbench_amd import _native, geometry as G, sample_reports
from cbgbench_amd.sample_reports import SampleReports
from oracle.ref_shim import REFERENCE_ROOT
from tests import native_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")


# ---- contacts ------------------------------------------------------------------------------------------------------------------------------------
def test_contacts_at_the_threshold_on_the_integer_lattice():
    # one carbon at the origin; pocket atoms on the lattice, where d2 is exact in any order
    x_rec = np.array([[4, 0, 0], [4, 0, 2.0 ** -20 * 3], [0, 4, 0], [2, 2, 3], [2, 2, 2], [0, 0, -4], [4, 0, 0], [-5, 0, 0]], np.float32)
    z_rec = np.array([6, 6, 7, 8, 6, 16, 1, 6], np.uint8)       # the second (4, 0, 0) is a hydrogen
    assert float(NM.dist2(x_rec[1], [0, 0, 0])) == 16.0 + 9 * 2.0 ** -40 > 16.0 and float(NM.dist2(x_rec[3], [0, 0, 0])) == 17.0
    rec, lig, cen, out = NM.pocket_contacts([[0, 0, 0]], [6], [0, 1], x_rec, z_rec, [0, 8], 1)
    assert rec.tolist() == [1, 0, 1, 0, 1, 1, 0, 0] and lig.tolist() == [1] and cen.tolist() == [[0, 0, 0]]
    assert out.tolist() == [[1, 1, 8, 4, 1, 0]]
    # a hydrogen ligand atom beside it touches nothing and does not move the centroid; a ligand of hydrogens is empty
    rec, lig, cen, out = NM.pocket_contacts([[0, 0, 0], [-5, 0, 1]], [6, 1], [0, 2], x_rec, z_rec, [0, 8], 1)
    assert rec.tolist() == [1, 0, 1, 0, 1, 1, 0, 0] and lig.tolist() == [1, 0] and cen.tolist() == [[0, 0, 0]] and out[0, :2].tolist() == [2, 1]
    rec, lig, cen, out = NM.pocket_contacts([[0, 0, 0], [-5, 0, 1]], [1, 1], [0, 2], x_rec, z_rec, [0, 8], 1)
    assert not rec.any() and not lig.any() and np.isnan(cen).all() and out.tolist() == [[2, 0, 8, 0, 0, NM.EMPTY]]
    # empty ligand, empty pocket, both; rows of no graph are not written
    rec, lig, cen, out = NM.pocket_contacts([[0, 0, 0]], [6], [0, 0, 1, 1], x_rec, z_rec, [0, 8, 8, 8], 3)
    assert out.tolist() == [[0, 0, 8, 0, 0, NM.EMPTY], [1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, NM.EMPTY]]
    assert not rec.any() and lig.tolist() == [0] and np.isnan(cen[0]).all() and cen[1].tolist() == [0, 0, 0] and np.isnan(cen[2]).all()
    rec, lig, _, _ = NM.pocket_contacts([[0, 0, 0], [1, 0, 0]], [6, 6], [0, 1], x_rec, z_rec, [2, 5], 1)
    assert rec.tolist() == [255, 255, 1, 0, 1, 255, 255, 255] and lig.tolist() == [1, 255]
    # another cutoff; a NaN one is no contact
    assert NM.pocket_contacts([[0, 0, 0]], [6], [0, 1], x_rec, z_rec, [0, 8], 1, cutoff2=17.0)[0].tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    assert not NM.pocket_contacts([[0, 0, 0]], [6], [0, 1], x_rec, z_rec, [0, 8], 1, cutoff2=float("nan"))[0].any()


def test_the_centroid_is_the_sequential_sum_in_atom_order():
    # one float64 addition after the other: the order shows where a sum is not exact
    x = np.array([[2.0 ** 60, 1, 0], [1, 2.0 ** 60, 0], [-2.0 ** 60, 0, 0], [0, -2.0 ** 60, 3]], np.float32)
    _, _, cen, _ = NM.pocket_contacts(x, [6] * 4, [0, 4], np.zeros((0, 3)), [], [0, 0], 1)
    assert cen.tolist() == [[0.0, 0.0, 0.75]]          # (2^60 + 1) rounds to 2^60: the small terms are lost in this order
    _, _, cen, _ = NM.pocket_contacts(x[[0, 2, 1, 3]], [6] * 4, [0, 4], np.zeros((0, 3)), [], [0, 0], 1)
    assert cen.tolist() == [[0.25, 0.0, 0.75]]
    _, _, cen, _ = NM.pocket_contacts([[1, 2, 3], [0, 0, 1], [2, 0, 0]], [6, 1, 8], [0, 3], np.zeros((0, 3)), [], [0, 0], 1)
    assert cen.tolist() == [[1.5, 1.0, 1.5]]


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------------
def words(bits):
    row = np.zeros(32, np.uint32)
    for b in bits:
        row[b >> 5] |= np.uint32(1 << (b & 31))
    return row


def compare(samples, natives, group_ptr):
    """samples / natives: dicts(fp bits, hash, fp_status, contacts bytes, centroid, contacts_status)"""
    def side(rows):
        ptr = np.concatenate([[0], np.cumsum([len(r["contact"]) for r in rows])]).astype(np.int32)
        return (np.stack([words(r["bits"]) for r in rows]) if rows else np.zeros((0, 32), np.uint32),
                np.array([r["hash"] for r in rows], np.uint64), np.array([r.get("fp_status", 0) for r in rows], np.int32),
                np.array([b for r in rows for b in r["contact"]], np.uint8), ptr,
                np.array([r.get("centroid", (0, 0, 0)) for r in rows], np.float64).reshape(-1, 3),
                np.array([r.get("contacts_status", 0) for r in rows], np.int32))
    return NM.native_compare(*side(samples), *side(natives), np.asarray(group_ptr, np.int32))


def test_rounding_at_exact_halves_and_with_union_zero():
    assert [NM.micro(1, 2), NM.micro(1, 3), NM.micro(2, 3), NM.micro(0, 5), NM.micro(7, 7), NM.micro(0, 0)] == [500000, 333333, 666667, 0, 1000000, 0]
    # union 64: 1 / 64 = 0.015625 exactly: no half.  union 128 = 2^7: k 10^6 / 128 = k 7812.5: a half for odd k, rounded up
    assert NM.micro(1, 128) == 7813 and NM.micro(3, 128) == 23438 and NM.micro(2, 128) == 15625
    assert all(NM.micro(c, u) == G.tanimoto_micro(words(range(c)), words(range(u))) for c, u in ((1, 128), (3, 128), (1, 3), (0, 0), (5, 5)))
    nat = {"bits": range(128), "hash": 5, "contact": [1] * 128 + [0] * 2, "centroid": (1, 2, 3)}
    rows = [{"bits": [0], "hash": 5, "contact": [1] + [0] * 129, "centroid": (1, 2, 3)},
            {"bits": [0, 1, 2], "hash": 6, "contact": [1] * 3 + [0] * 127, "centroid": (4, 6, 3)},
            {"bits": range(128), "hash": 5, "contact": [1] * 128 + [0, 0], "centroid": (1, 2, 3.5)}]
    out, d2, grp = compare(rows, [nat], [0, 3])
    assert out.tolist() == [[7813, 1, 1, 128, 7813, 0], [23438, 0, 3, 128, 23438, 0], [1000000, 1, 128, 128, 1000000, 0]]
    assert d2.tolist() == [0.0, 25.0, 0.25] and grp.tolist() == [[3, 3, 2, 1031251, 1000000, 3, 1031251, 1000000, 0]]
    # neither has a bit, neither touches an atom: 0, not a division by zero
    out, d2, grp = compare([{"bits": [], "hash": 0, "contact": [0, 0]}], [{"bits": [], "hash": 0, "contact": [0, 0]}], [0, 1])
    assert out.tolist() == [[0, 1, 0, 0, 0, 0]] and grp.tolist() == [[1, 1, 1, 0, 0, 1, 0, 0, 0]]


def test_every_status_bit_and_groups_of_zero_and_one():
    nat = [{"bits": [1, 2], "hash": 9, "contact": [1, 0, 1]},
           {"bits": [1, 2], "hash": 9, "contact": [1, 1], "fp_status": 8, "centroid": (0, 0, 1)},
           {"bits": [3], "hash": 1, "contact": [], "contacts_status": NM.EMPTY, "centroid": (np.nan,) * 3}]
    rows = [{"bits": [1, 2], "hash": 9, "contact": [1, 1, 1]},                                  # pocket 0
            {"bits": [1], "hash": 9, "contact": [0, 0, 1], "fp_status": 1},                      # ... not evaluated
            {"bits": [1], "hash": 2, "contact": [0, 1], "contacts_status": NM.EMPTY},            # ... another pocket length, no centroid
            {"bits": [2], "hash": 9, "contact": [0, 1]},                                          # pocket 1: native not evaluated
            {"bits": [2], "hash": 9, "contact": [0, 1], "fp_status": 16}]                         # ... and neither is the sample
    out, d2, grp = compare(rows, nat, [0, 3, 5, 5])
    assert out.tolist() == [[1000000, 1, 2, 3, 666667, 0], [-1, -1, 1, 2, 500000, NM.SAMPLE_NOT_EVALUATED],
                            [500000, 0, -1, -1, -1, NM.POCKET_MISMATCH], [-1, -1, 1, 2, 500000, NM.NATIVE_NOT_EVALUATED],
                            [-1, -1, 1, 2, 500000, NM.NATIVE_NOT_EVALUATED | NM.SAMPLE_NOT_EVALUATED]]
    assert d2[:2].tolist() == [0.0, 0.0] and math.isnan(d2[2]) and d2[3:].tolist() == [1.0, 1.0]
    assert grp.tolist() == [[3, 2, 1, 1500000, 1000000, 2, 1166667, 666667, 0], [2, 0, 0, 0, -1, 2, 1000000, 500000, NM.NATIVE_NOT_EVALUATED],
                            [0, 0, 0, 0, -1, 0, 0, -1, 0]]
    # a native without a centroid: NaN for its samples; malformed group_ptr: clamped, evaluated and reported; a graph in no group keeps
    # what was there
    out, d2, grp = compare(rows[:1], [nat[2]], [-4, 1])
    assert out.tolist() == [[0, 0, -1, -1, -1, NM.POCKET_MISMATCH]] and math.isnan(d2[0]) and grp[0, [0, -1]].tolist() == [1, NM.BAD_GROUPS]
    out, d2, grp = compare(rows[:2] + [rows[0]], [nat[0], nat[0]], [2, 1, 9])
    assert grp[:, 0].tolist() == [0, 2] and grp[:, -1].tolist() == [NM.BAD_GROUPS, NM.BAD_GROUPS]
    assert out[0].tolist() == [-1] * 6 and out[2].tolist() == [1000000, 1, 2, 3, 666667, 0]
    out, d2, grp = compare(rows[:2], [nat[0]], [1, 2])
    assert out[0].tolist() == [-1] * 6 and np.array([d2[0]]).view(np.int64)[0] == -1 and grp.tolist() == [[1, 0, 0, 0, -1, 1, 500000, 500000, 0]]


# ---- the reference's formulas -----------------------------------------------------------------------------------------------------------------
def reference_metrics():
    path = os.path.join(REFERENCE_ROOT, "evaluate_scripts", "cal_chem_results.py")
    if not os.path.exists(path):
        pytest.skip("needs the reference tree")
    spec = importlib.util.spec_from_file_location("cal_chem_results", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.calculate_vina_metrics


def test_native_pocket_metrics_restate_calculate_vina_metrics(capsys):
    ref_fn = reference_metrics()
    rng = np.random.default_rng(20261021)
    eps = 2.0 ** -52
    cases = [(rng.integers(-9000000, 2000000, n).tolist(), rng.integers(1, 40, n).tolist(), int(rng.integers(-9000000, -1)))
             for n in (1, 2, 10, 200)]
    cases.append(([-5000000] * 7, [20] * 7, -5000000))                  # all equal to the native: vina < ref is strict
    cases.append(([-5000000, -5000001], [20, 21], -5000000))
    for micro, heavy, nat in cases:
        mine = G.native_pocket_metrics(micro, heavy, nat)
        result = [{"vina": {"score_only": {"affinity": m / 1e6}}, "num_atoms": n} for m, n in zip(micro, heavy)]
        gap, imp, mean, le = ref_fn(result, {"vina": {"score_only": {"affinity": nat / 1e6}}}, "score_only")
        # the same float64 expressions on the same inputs.  A mean of n terms t_i, each a value of one subtraction and one division (or
        # one division) of exactly given inputs, summed in any order and divided once: the first-order bound of the error of each
        # side is (2 + (n - 1) + 1 [+ 1 for the factor 100]) eps max |t_i|; the two sides differ by at most twice that
        n, vina, ref = len(micro), np.array(micro) / 1e6, nat / 1e6
        bound = lambda t, extra=0: 2 * (n + 2 + extra) * eps * float(np.max(np.abs(t)))
        assert mine["skipped"] == G.NATIVE_EVALUATED and mine["n_scored"] == n
        assert abs(mine["binding_gap"] - gap) <= bound((vina - ref) / ref * 100, 1)
        assert abs(mine["improved_ratio"] * 100 - imp) <= 2 * eps * 100 and mine["n_improved"] == int((vina < ref).sum())
        assert abs(mine["mean_score"] - mean) <= bound(vina) and abs(mine["ligand_efficiency"] - le) <= bound(vina / np.array(heavy))
        for k in ("binding_gap", "improved_ratio", "mean_score", "ligand_efficiency"):      # half up, whole millionths
            assert mine[k + "_micro"] == math.floor(mine[k] * 1e6 + 0.5) and isinstance(mine[k + "_micro"], int)
    assert G.native_pocket_metrics(*cases[4])["improved_ratio"] == 0.0 and G.native_pocket_metrics(*cases[5])["improved_ratio"] == 0.5
    # a positive native score: the reference returns None; a native score of zero: not skipped, and divided by as there
    assert ref_fn([{"vina": {"k": {"affinity": -1.0}}, "num_atoms": 3}], {"vina": {"k": {"affinity": 1e-6}}}, "k") is None
    assert G.native_pocket_metrics([-1000000], [3], 1)["skipped"] == G.NATIVE_POSITIVE_NATIVE
    with np.errstate(divide="ignore", invalid="ignore"):
        want = ref_fn([{"vina": {"k": {"affinity": v}}, "num_atoms": 4} for v in (-1.0, -2.0)], {"vina": {"k": {"affinity": 0.0}}}, "k")
        both = ref_fn([{"vina": {"k": {"affinity": v}}, "num_atoms": 4} for v in (-1.0, 0.0)], {"vina": {"k": {"affinity": 0.0}}}, "k")
    mine, nan = G.native_pocket_metrics([-1000000, -2000000], [4, 4], 0), G.native_pocket_metrics([-1000000, 0], [4, 4], 0)
    assert mine["skipped"] == G.NATIVE_EVALUATED and mine["binding_gap"] == want[0] == -math.inf and mine["binding_gap_micro"] is None
    assert (mine["improved_ratio"] * 100, mine["mean_score"], mine["ligand_efficiency"]) == tuple(want[1:]) == (100.0, -1.5, -0.375)
    assert math.isnan(nan["binding_gap"]) and math.isnan(both[0]) and nan["improved_ratio"] * 100 == both[1] == 50.0
    capsys.readouterr()


def test_native_pocket_metrics_without_the_reference():
    m = G.native_pocket_metrics([-6000000, None, -2000000, -4000000, -9000000], [10, 10, 20, 40, 0], -4000000)
    assert m["skipped"] == G.NATIVE_EVALUATED and m["n_scored"] == 3 and m["n_improved"] == 1 and m["native_score_micro"] == -4000000
    assert m["binding_gap"] == 0.0 and m["improved_ratio"] == 1 / 3 and m["mean_score"] == -4.0
    assert m["ligand_efficiency"] == (-0.6 + -0.1 + -0.1) / 3
    assert (m["binding_gap_micro"], m["improved_ratio_micro"], m["mean_score_micro"], m["ligand_efficiency_micro"]) == (0, 333333, -4000000, -266667)
    assert G._half_up_micro(0.0000005) == 1 and G._half_up_micro(-0.0000005) == 0 and G._half_up_micro(-0.0000015) == -1
    for args, why in ((([-1], [3], None), G.NATIVE_NO_NATIVE_SCORE), (([-1], [3], 1), G.NATIVE_POSITIVE_NATIVE),
                      (([None, -5], [3, 0], -7), G.NATIVE_NO_SAMPLE), (([], [], -7), G.NATIVE_NO_SAMPLE)):
        m = G.native_pocket_metrics(*args)
        assert m["skipped"] == why and math.isnan(m["binding_gap"]) and m["mean_score_micro"] is None and m["n_improved"] == 0


# ---- totals ---------------------------------------------------------------------------------------------------------------------------------------
def pockets_for_totals():
    rng = np.random.default_rng(7)
    out = []
    for k in range(9):
        n = int(rng.integers(0, 6))
        micro = [None if rng.random() < 0.2 else int(v) for v in rng.integers(-8000000, 1000000, n)]
        nat = [None, 250000, 0][k] if k < 3 else int(rng.integers(-8000000, -1000000))
        n_fp = int(rng.integers(0, n + 1))
        n_same = int(rng.integers(0, n_fp + 1))
        row = [n, n_fp, n_same, 400000 * n_fp, 900000 if n_fp else -1, n, 123457 * n, 500000 if n else -1, 0]
        out.append(G.native_pocket_counts(row, G.native_pocket_metrics(micro, rng.integers(1, 30, n).tolist(), nat)))
    return out


def test_totals_split_over_ranks_sum_to_the_whole():
    pockets = pockets_for_totals()
    assert all(tuple(p) == G.NATIVE_POCKET_KEYS for p in pockets)
    totals = G.native_totals(pockets)
    assert all(isinstance(v, int) for v in totals) and len(totals) == len(G.NATIVE_COUNT_KEYS)
    for cuts in [(c,) for c in range(10)] + [(a, b) for a in range(10) for b in range(a, 10)]:
        edges = (0,) + cuts + (9,)
        parts = [G.native_totals(pockets[a:b]) for a, b in zip(edges[:-1], edges[1:])]
        assert [sum(col) for col in zip(*parts)] == totals
    c = dict(zip(G.NATIVE_COUNT_KEYS, totals))
    assert c["n_pockets"] == 9 and c["n_pockets_native_not_evaluated"] >= 1 and c["n_pockets_positive_native"] >= 1
    assert c["n_pockets_evaluated"] + c["n_pockets_positive_native"] + c["n_pockets_native_not_evaluated"] + c["n_pockets_no_sample"] == 9
    s = G.summarise_native_totals(totals)
    assert s == G.summarise_native(pockets) and s["counts"] == c
    assert set(s) == set(G.NATIVE_RATIOS) | {"n_pockets_positive_native", "n_pockets_native_not_evaluated", "n_pockets_no_sample", "counts"}
    good = [p for p in pockets if p["skipped"] == G.NATIVE_EVALUATED]
    assert s["mean_score"] == sum(p["mean_score_micro"] for p in good) / (1e6 * len(good))
    assert s["improved_mol_ratio"] == sum(p["improved_ratio_micro"] for p in good) / (1e6 * len(good))
    gaps = [p["binding_gap_micro"] for p in good if p["binding_gap_micro"] is not None]
    assert s["mean_binding_gap"] == sum(gaps) / (1e6 * len(gaps)) and c["n_pockets_with_gap"] == len(gaps)
    assert s["rediscovered_mol_ratio"] == c["n_same_hash"] / c["n_fp_compared"] and s["mean_native_similarity"] == 0.4
    assert s["mean_contact_jaccard"] == 0.123457
    nothing = G.summarise_native([])
    assert all(math.isnan(nothing[k]) for k in G.NATIVE_RATIOS) and nothing["counts"]["n_pockets"] == 0


# ---- the report's host side -------------------------------------------------------------------------------------------------------------------
NATIVE_FIELDS = ("native_similarity", "native_same_hash", "native_contact_jaccard", "native_contact_common", "native_contact_union",
                 "native_centroid_distance", "score_minus_native", "better_than_native", "ligand_efficiency", "native_status")
DEPS = ("bonds", "rings", "aromatic", "valence", "interactions", "diversity")


def interaction_rows(scores, status=None):
    """graph_counts [n, 13] and graph_terms [n, 5] whose ``interaction_scores`` are ``scores`` up to rounding (no rotatable bond)"""
    gc = np.zeros((len(scores), 13), np.int32)
    gc[:, -1] = status if status is not None else 0
    terms = np.zeros((len(scores), 5), np.float64)
    terms[:, 0] = np.array(scores) / G.INTERACTION_WEIGHTS[0]
    return torch.from_numpy(gc), torch.from_numpy(terms)


def fake_reports(calls):
    """stand-ins for geometry.batch_*: they record (report, number of graphs, the dependencies they were handed) and check that the
    dependencies are the objects made for the same state; ``batch_native`` answers with the model's numbers for three samples in two
    pockets (2 + 1) and their natives, as CPU tensors"""
    made = {}

    def fake(name):
        def run(batch, x, c, lig_batch, mode, *args, **deps):
            n = int(batch["num_graphs"])
            calls.append((name, n, tuple(sorted(k for k, v in deps.items() if v is not None))))
            assert all(v is made[k, n] for k, v in deps.items() if v is not None)
            if name == "native":
                group_ptr, theirs = args
                assert group_ptr == [0, 2, 3] and all(theirs[k] is made[k, 2] for k in deps) and theirs["x"].shape == (2, 3)
                made[name, n] = native_answer(group_ptr)
            else:
                cols = {"bonds": 6, "rings": 13, "aromatic": 10, "valence": 22, "geometry": 6}.get(name, 1)
                made[name, n] = {"graph_counts": torch.zeros(n, cols, dtype=torch.int32), "flags": torch.zeros(x.shape[0], dtype=torch.uint8),
                                 "nr_bonds": torch.zeros(x.shape[0], dtype=torch.int32), "atom_ring_min": torch.zeros(x.shape[0], dtype=torch.uint8)}
            return made[name, n]
        return run
    return {"batch_" + name: fake(name) for name in DEPS + ("native", "geometry")}


def native_answer(group_ptr):
    nat = [{"bits": range(128), "hash": 5, "contact": [1, 1, 0, 0], "centroid": (0, 0, 0)},
           {"bits": [7], "hash": 8, "contact": [0, 1, 1], "centroid": (1, 1, 1)}]
    rows = [{"bits": range(128), "hash": 5, "contact": [1, 1, 0, 0], "centroid": (0, 0, 0)},
            {"bits": [0], "hash": 6, "contact": [0, 1, 1, 0], "centroid": (3, 4, 0), "fp_status": 1},
            {"bits": [7, 8], "hash": 9, "contact": [0, 0, 1], "centroid": (1, 1, 3)}]
    out, d2, grp = compare(rows, nat, group_ptr)
    t = torch.from_numpy
    counts, terms = interaction_rows([-5.0, -7.5, -1.0], [0, 0, 8])
    nat_counts, nat_terms = interaction_rows([-5.0, -2.0])
    nat_counts[0, 10] = 3
    contact_counts = torch.tensor([[9, 8, 4, 2, 3, 0], [12, 10, 4, 2, 2, 0], [5, 5, 3, 1, 1, 0]], dtype=torch.int32)
    return {"sample_counts": t(out), "centroid_d2": t(d2), "group_counts": t(grp), "group_ptr": torch.tensor(group_ptr, dtype=torch.int32),
            "contact_counts": contact_counts, "interaction_counts": counts, "interaction_terms": terms,
            "native_contact_counts": torch.tensor([[8, 8, 4, 2, 4, 0], [3, 3, 3, 2, 2, 0]], dtype=torch.int32),
            "native_interaction_counts": nat_counts, "native_interaction_terms": nat_terms}


def pocket():
    return {k: torch.zeros(0) for k in ("protein_pos", "protein_element", "protein_element_batch", "protein_aa_type", "protein_atom_feature")}


def stand_in_native():
    return {"x": torch.zeros(2, 3), "c": torch.zeros(2, dtype=torch.long), "lig_batch": torch.tensor([0, 1]), "batch": pocket()}


def test_against_needs_and_the_report_on_stand_ins(monkeypatch, tmp_path, capsys):
    assert sample_reports.AGAINST == ("native",) and sample_reports.ACROSS == ("diversity",) and sample_reports.LATE == ("groups",)
    assert sample_reports.ORDER == ("geometry", "bonds", "rings", "aromatic", "distributions", "valence")
    assert sample_reports.needs("native", "add_aromatic") == sample_reports.NEEDS["native"] == DEPS
    assert sample_reports.needs("native", "basic") == ("bonds", "rings", "valence", "interactions", "diversity")
    assert [rep.name for rep in G.COUNT_REPORTS] == ["geometry", "bonds", "rings", "aromatic", "valence"]
    calls = []
    for name, fn in fake_reports(calls).items():
        monkeypatch.setattr(G, name, fn)
    state = (torch.zeros(3, 3), torch.zeros(3, dtype=torch.long), torch.tensor([0, 1, 2]))
    r = SampleReports(("native",))
    with pytest.raises(ValueError, match="group_ptr"):
        r.evaluate(torch.device("cpu"), state, pocket(), 3, "add_aromatic", native=stand_in_native())
    with pytest.raises(ValueError, match="needs native"):
        r.evaluate(torch.device("cpu"), state, pocket(), 3, "add_aromatic", group_ptr=[0, 2, 3])
    assert calls == []
    ev = r.evaluate(torch.device("cpu"), state, pocket(), 3, "add_aromatic", group_ptr=[0, 2, 3], native=stand_in_native())
    chain = [("bonds", ()), ("rings", ("bonds",)), ("aromatic", ("bonds", "rings")), ("valence", ("aromatic", "bonds")),
             ("interactions", ("bonds", "valence")), ("diversity", ("aromatic", "bonds", "rings"))]
    # the samples' dependencies, the native ligands' by the same functions, then the comparison
    assert calls == [(n, 3, d) for n, d in chain] + [(n, 2, d) for n, d in chain] + [("native", 3, tuple(sorted(DEPS)))]
    assert sorted(ev) == ["native", "native_reports"] and ev["native_reports"] == {} and list(r.seconds) == ["native"] and r.seconds["native"] > 0.0
    del calls[:]
    r2 = SampleReports(("geometry", "native", "rings"))
    ev2 = r2.evaluate(torch.device("cpu"), state, pocket(), 3, "basic", group_ptr=[0, 2, 3], native=stand_in_native())
    assert list(r2.seconds) == ["geometry", "rings", "native"] and sorted(ev2["native_reports"]) == ["geometry", "rings"]
    assert [c[:2] for c in calls] == [("geometry", 3), ("bonds", 3), ("rings", 3), ("valence", 3), ("interactions", 3), ("diversity", 3),
                                      ("bonds", 2), ("rings", 2), ("valence", 2), ("interactions", 2), ("diversity", 2), ("native", 3),
                                      ("geometry", 2)]

    smp = [{"atom": [6]}, {"atom": [6]}, {"atom": [6]}]
    r.annotate(smp, ev)
    assert all(sorted(s) == sorted(("atom",) + NATIVE_FIELDS) for s in smp)
    assert [s["native_similarity"] for s in smp[::2]] == [1.0, 0.5] and math.isnan(smp[1]["native_similarity"])
    assert [s["native_same_hash"] for s in smp] == [True, None, False]
    assert [s["native_contact_jaccard"] for s in smp] == [1.0, 0.333333, 0.5] and [s["native_contact_common"] for s in smp] == [2, 1, 1]
    assert [s["native_contact_union"] for s in smp] == [2, 3, 2] and [s["native_centroid_distance"] for s in smp] == [0.0, 5.0, 2.0]
    assert [s["score_minus_native"] for s in smp[:2]] == [0.0, -2.5] and math.isnan(smp[2]["score_minus_native"])
    assert [s["better_than_native"] for s in smp] == [False, True, None]
    assert [s["ligand_efficiency"] for s in smp[:2]] == [-5.0 / 8, -0.75] and math.isnan(smp[2]["ligand_efficiency"])
    assert [s["native_status"] for s in smp] == [0, NM.SAMPLE_NOT_EVALUATED, 0]
    natives = r.annotate_native([{"atom": [6]}, {"atom": [8]}], ev)
    assert natives == [{"atom": [6], "score": -5.0, "score_micro": -5000000, "n_contact_atoms": 3, "n_pocket_contact_atoms": 2},
                       {"atom": [8], "score": -2.0, "score_micro": -2000000, "n_contact_atoms": 0, "n_pocket_contact_atoms": 2}]
    natives2 = r2.annotate_native([{"atom": [6]}, {"atom": [8]}], ev2)
    assert sorted(natives2[0]) == sorted(["atom", "score", "score_micro", "n_contact_atoms", "n_pocket_contact_atoms", "nr_bonds", "atom_stable", "inter_clash",
                                          "intra_clash_table_bonds", "mol_stable", "ring_sizes", "n_rings_larger", "atom_ring_min", "ring_status"])
    rec0, rec1 = r.pocket_counts(ev, 0, 2), r.pocket_counts(ev, 2, 3)
    assert list(rec0) == ["native_comparison"] and tuple(rec0["native_comparison"]) == G.NATIVE_POCKET_KEYS
    assert rec0["native_comparison"] == {
        "n_mol": 2, "n_fp_compared": 1, "n_same_hash": 1, "sim_micro_sum": 1000000, "sim_micro_max": 1000000, "n_contact_compared": 2,
        "contact_micro_sum": 1333333, "contact_micro_max": 1000000, "status": 0, "skipped": 0, "n_scored": 2, "n_improved": 1,
        "native_score_micro": -5000000, "binding_gap_micro": 25000000, "improved_ratio_micro": 500000, "mean_score_micro": -6250000,
        "ligand_efficiency_micro": -687500}
    assert rec1["native_comparison"]["skipped"] == G.NATIVE_NO_SAMPLE and rec1["native_comparison"]["native_score_micro"] == -2000000
    with pytest.raises(ValueError, match="no group"):
        r.pocket_counts(ev, 0, 1)
    r.finish(str(tmp_path), 0, torch.device("cpu"))
    want = G.summarise_native([rec0["native_comparison"], rec1["native_comparison"]])
    with open(tmp_path / "native_summary.json") as f:
        assert f.read() == json.dumps(want, indent=1, sort_keys=True)
    assert os.listdir(tmp_path) == ["native_summary.json"] and want["counts"]["n_pockets_no_sample"] == 1
    assert want["improved_mol_ratio"] == 0.5 and want["mean_binding_gap"] == 25.0 and want["mean_native_score"] == -5.0
    line = capsys.readouterr().out
    assert line.startswith("native: improved_mol_ratio 0.5000, mean_binding_gap 25.0000, mean_score -6.2500, mean_native_score -5.0000")
    assert "1 of 2 pockets evaluated" in line and "not the Vina program" in line and "not RDKit's" in line


def test_a_run_without_the_flag_adds_no_key(monkeypatch, tmp_path):
    calls = []
    for name, fn in fake_reports(calls).items():
        monkeypatch.setattr(G, name, fn)
    state = (torch.zeros(3, 3), torch.zeros(3, dtype=torch.long), torch.tensor([0, 1, 2]))
    r = SampleReports(("rings",))
    ev = r.evaluate(torch.device("cpu"), state, {}, 3, "basic", group_ptr=[0, 2, 3], native=stand_in_native())
    assert [c[:2] for c in calls] == [("bonds", 3), ("rings", 3)] and "native" not in r.seconds and list(ev) == ["rings"]
    smp = [{"atom": [6]}]
    r.annotate(smp * 3, ev)
    assert not set(smp[0]) & set(NATIVE_FIELDS) and list(r.pocket_counts(ev, 0, 2)) == ["rings"]
    r.finish(str(tmp_path), 0, torch.device("cpu"))
    assert os.listdir(tmp_path) == ["rings_summary.json"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    x, z, b = torch.zeros(2, 3), torch.full((2,), 6), torch.zeros(2, dtype=torch.long)
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.pocket_contacts(x, z, b, x, z, b, 1)
    fps = {"fingerprint": torch.zeros(1, 32, dtype=torch.int32), "mol_hash": torch.zeros(1, dtype=torch.int64),
           "graph_counts": torch.zeros(1, 5, dtype=torch.int32)}
    con = {"rec_contact": torch.zeros(2, dtype=torch.uint8), "rec_ptr": torch.tensor([0, 2], dtype=torch.int32),
           "centroid": torch.zeros(1, 3, dtype=torch.float64), "graph_counts": torch.zeros(1, 6, dtype=torch.int32)}
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        G.native_compare(fps, con, fps, con, [0, 1])


def pockets_file(tmp_path, **change):
    rng = np.random.default_rng(3)
    raw = []
    for k in range(2):
        n = 30 + k
        feat = np.zeros((n, 27), np.float32)
        feat[:, 0] = 1
        raw.append({"protein_pos": rng.normal(size=(n, 3)).astype(np.float32) * 6, "protein_atom_feature": feat,
                    "protein_aa_type": rng.integers(0, 20, n), "ligand_pos": rng.normal(size=(5, 3)).astype(np.float32),
                    "ligand_atom_type": rng.integers(0, 13, 5)})
    for key, value in change.items():
        if value is None:
            del raw[1][key]
        else:
            raw[1][key] = value
    path = str(tmp_path / "pockets.pt")
    torch.save(raw, path)
    return path


def test_sample_cli_refusals(tmp_path, monkeypatch):
    from cbgbench_amd import sample_cli
    with pytest.raises(SystemExit, match=r"--native runs on the GPU \(cbgx_pocket_contacts / cbgx_native_compare have no CPU fallback\)"):
        sample_cli.main(["--config", CFG, "--device", "cpu", "--native", "--random_init", "--pockets", pockets_file(tmp_path)])
    # the other refusals come before any model is built, on any device: a stand-in device check lets them be reached without a GPU
    monkeypatch.setattr(SampleReports, "refuse", lambda self, dev, atom_mode: None)
    monkeypatch.setattr(sample_cli, "get_model", lambda *a, **k: pytest.fail("a model was built"))
    common = ["--config", CFG, "--device", "cpu", "--native", "--random_init"]
    with pytest.raises(SystemExit, match="--native needs --pockets"):
        sample_cli.main(common + ["--synthetic", "1"])
    with pytest.raises(SystemExit, match="pocket 1 carries no ligand_pos"):
        sample_cli.main(common + ["--pockets", pockets_file(tmp_path, ligand_pos=None)])
    with pytest.raises(SystemExit, match="pocket 1: ligand_atom_type out of range"):
        sample_cli.main(common + ["--pockets", pockets_file(tmp_path, ligand_atom_type=np.array([0, 1, 2, 3, 99]))])
    with pytest.raises(SystemExit, match="pocket 1: ligand_atom_type out of range"):
        sample_cli.main(common + ["--pockets", pockets_file(tmp_path, ligand_atom_type=np.array([0, 1, 2, 3, -1]))])
    with pytest.raises(SystemExit, match=r"pocket 1: ligand_pos \(5, 3\) and ligand_atom_type \(4,\)"):
        sample_cli.main(common + ["--pockets", pockets_file(tmp_path, ligand_atom_type=np.array([0, 1, 2, 3]))])
    with pytest.raises(SystemExit, match=r"pocket 1: ligand_pos \(0, 3\)"):
        sample_cli.main(common + ["--pockets", pockets_file(tmp_path, ligand_pos=np.zeros((0, 3)), ligand_atom_type=np.zeros(0))])
    pos, typ = sample_cli.load_native(torch.load(pockets_file(tmp_path, ligand_gen_index=[np.array([0, 1])]), weights_only=False), 13)[1]
    assert pos.dtype == np.float32 and pos.shape == (5, 3) and typ.dtype == np.int64 and typ.shape == (5,)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_pocket_contacts", "cbgx_native_compare")


def test_entries_are_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH, sources
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _native.EXPORTS and hasattr(lib, name)
    assert len(_native.EXPORTS[ENTRIES[0]][1]) == 15 and len(_native.EXPORTS[ENTRIES[1]][1]) == 23
    assert _native.EXPORTS[ENTRIES[0]][1][9] is ctypes.c_double
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ENTRIES:
            assert f" {name}\n" in sym, (path, name)
    for xcheck in (False, True):
        assert any(os.path.basename(p) == "native.hip" for p in sources(xcheck))
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    for name, value in (("CONTACTS_GRAPH_COLS", len(G.CONTACTS_GRAPH_COLUMNS)), ("NATIVE_SAMPLE_COLS", len(G.NATIVE_SAMPLE_COLUMNS)),
                        ("NATIVE_GROUP_COLS", len(G.NATIVE_GROUP_COLUMNS))):
        assert f"#define CBGX_{name} {value} " in hdr, name
    for name, value in (("CONTACTS_CUTOFF2", G.CONTACTS_CUTOFF2), ("CONTACTS_EMPTY", G.CONTACTS_EMPTY),
                        ("NATIVE_SAMPLE_NOT_EVALUATED", G.NATIVE_SAMPLE_NOT_EVALUATED), ("NATIVE_NATIVE_NOT_EVALUATED", G.NATIVE_NATIVE_NOT_EVALUATED),
                        ("NATIVE_POCKET_MISMATCH", G.NATIVE_POCKET_MISMATCH), ("NATIVE_BAD_GROUPS", G.NATIVE_BAD_GROUPS)):
        assert f"#define CBGX_{name} {value}\n" in hdr, name
    assert (len(G.CONTACTS_GRAPH_COLUMNS), len(G.NATIVE_SAMPLE_COLUMNS), len(G.NATIVE_GROUP_COLUMNS), G.CONTACTS_CUTOFF2, G.CONTACTS_EMPTY,
            G.MAX_LIGAND_ATOMS) == (NM.CONTACT_COLS, NM.SAMPLE_COLS, NM.GROUP_COLS, NM.CUTOFF2, NM.EMPTY, NM.MAX_LIGAND) == (6, 6, 9, 16.0, 16, 1024)
    assert (NM.SAMPLE_NOT_EVALUATED, NM.NATIVE_NOT_EVALUATED, NM.POCKET_MISMATCH, NM.BAD_GROUPS) == (1, 2, 4, 8) == \
        (G.NATIVE_SAMPLE_NOT_EVALUATED, G.NATIVE_NATIVE_NOT_EVALUATED, G.NATIVE_POCKET_MISMATCH, G.NATIVE_BAD_GROUPS)
    assert sample_reports._GPU_ONLY["native"].startswith("--native runs on the GPU")


ONE = ctypes.c_void_p(16)       # a pointer that is never dereferenced: argument checks come first
PC_POINTERS = ("x_lig", "z_lig", "lig_ptr", "x_rec", "z_rec", "rec_ptr", "rec_contact", "lig_contact", "centroid", "graph_out")
SIDE = ("fp", "mol_hash", "fp_status", "rec_contact", "rec_ptr", "centroid", "contacts_status")
NC_POINTERS = SIDE + tuple(k + "_nat" for k in SIDE) + ("group_ptr", "sample_out", "centroid_d2", "group_out")


def _contacts(n_lig, n_rec, B, **kw):
    a = {k: kw.get(k, ONE) for k in PC_POINTERS}
    return _native.lib().cbgx_pocket_contacts(a["x_lig"], a["z_lig"], a["lig_ptr"], n_lig, a["x_rec"], a["z_rec"], a["rec_ptr"], n_rec, B, 16.0,
                                              a["rec_contact"], a["lig_contact"], a["centroid"], a["graph_out"], None)


def _compare(B, n_rec, P, n_rec_nat, **kw):
    a = {k: kw.get(k, ONE) for k in NC_POINTERS}
    return _native.lib().cbgx_native_compare(*[a[k] for k in SIDE], B, n_rec, *[a[k + "_nat"] for k in SIDE], P, n_rec_nat, a["group_ptr"],
                                             a["sample_out"], a["centroid_d2"], a["group_out"], None)


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    assert [_contacts(-1, 3, 2), _contacts(4, -1, 2), _contacts(4, 3, -1)] == [-1] * 3 and b"negative" in lib.cbgx_last_error()
    for name in PC_POINTERS:
        assert _contacts(4, 3, 2, **{name: None}) == -1 and b"NULL" in lib.cbgx_last_error(), name
    # B == 0: nothing to do, nothing is dereferenced; the per-atom arrays may be NULL without atoms
    assert _contacts(0, 0, 0, **{k: None for k in PC_POINTERS}) == 0 and _contacts(7, 5, 0, lig_ptr=None, centroid=None) == 0
    x = np.zeros((4, 3), np.float32)
    assert _contacts(4, 3, 2, x_lig=ctypes.c_void_p(x.ctypes.data)) == -1
    msg = lib.cbgx_last_error().decode()
    assert "NULL" not in msg and "x_lig is not memory the device can read" in msg
    ptr = np.zeros(3, np.int32)
    pp = ctypes.c_void_p(ptr.ctypes.data)
    assert _contacts(0, 0, 2, lig_ptr=pp, **{k: None for k in ("x_lig", "z_lig", "x_rec", "z_rec", "rec_contact", "lig_contact")}) == -1
    assert "lig_ptr is not memory the device can read" in lib.cbgx_last_error().decode()

    assert [_compare(-1, 1, 1, 1), _compare(2, -1, 1, 1), _compare(2, 1, -1, 1), _compare(2, 1, 1, -1)] == [-1] * 4
    assert b"negative" in lib.cbgx_last_error()
    for name in NC_POINTERS:
        assert _compare(2, 3, 1, 3, **{name: None}) == -1 and b"NULL" in lib.cbgx_last_error(), name
    # P == 0: nothing to do, nothing is dereferenced; the contact bytes may be NULL without pocket atoms
    assert _compare(0, 0, 0, 0, **{k: None for k in NC_POINTERS}) == 0
    assert _compare(5, 0, 0, 0, rec_contact=None, rec_contact_nat=None, group_ptr=None, group_out=None, rec_ptr=None) == 0
    fp = np.zeros((2, 32), np.uint32)
    assert fp.ctypes.data % 16 == 0
    assert _compare(2, 0, 1, 0, fp=ctypes.c_void_p(fp.ctypes.data), rec_contact=None, rec_contact_nat=None) == -1
    msg = lib.cbgx_last_error().decode()
    assert "NULL" not in msg and "fp is not memory the device can read" in msg
    assert _compare(2, 1, 1, 1, fp=ctypes.c_void_p(fp.ctypes.data + 4)) == -1 and b"fp is not aligned" in lib.cbgx_last_error()
    assert _compare(2, 1, 1, 1, fp_nat=ctypes.c_void_p(fp.ctypes.data + 8)) == -1 and b"fp_nat is not aligned" in lib.cbgx_last_error()
    assert _compare(0, 0, 1, 0, group_ptr=pp, **{k: None for k in SIDE if k != "rec_ptr"}, rec_contact_nat=None, sample_out=None,
                    centroid_d2=None) == -1
    assert "is not memory the device can read" in lib.cbgx_last_error().decode()
