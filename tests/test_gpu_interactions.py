"""Typed pocket contacts and the Vina-form pair terms on the GPU (csrc/interactions.hip: cbgx_pocket_types, cbgx_ligand_interactions;
cbgbench_amd/geometry.py; sample_cli --interactions) against the numpy / Python model of tests/interactions_model.py.

Every integer and byte output is compared with ``==``.  Every float output must satisfy |device - model| <= 1e-9 * sum|addends|, the
model's value being the correctly rounded sum (math.fsum) of the same addends: the arguments of exp are bit-equal by construction, the
device's fp64 exp is good to a few ulp, and re-ordering at most 256 x 2048 addends costs at most n 2^-53 sum|addends|, about 6e-11 of it.
Output buffers handed to the entries are pre-filled with 0xFF bytes and carry a 0xFF guard tail inside the same allocation, which must
stay as it is."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, geometry as G
from tests import interactions_model as IM, valence_model as VM
from tests.test_gpu_rings import DEV, GUARD, _dev, _equal, _ff
from tests.test_gpu_valence import benzene_with_pendants
from tests.test_interactions import (C_X_SINGLE_PM, INTERACTION_FIELDS, MOLECULES, assemble, hand_batch, hand_pairs, ligand_coordinates,
                                     make_pocket, seeded_interactions, threshold_carbons, threshold_pocket, typing_table_atoms)
from tests.test_valence import HAND, collate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9


def run_pocket(x_rec, z_rec, rec_ptr, rec_aa, rec_backbone):
    """cbgx_pocket_types on a 0xFF output with a guard tail -> rec_type [n_rec]; atoms of no graph stay 255"""
    n_rec, B = len(z_rec), len(rec_ptr) - 1
    t = _ff(n_rec + GUARD, torch.uint8)
    p = _native.ptr
    x, z, rp = _dev(np.asarray(x_rec, np.float32).reshape(-1, 3), np.float32), _dev(z_rec, np.uint8), _dev(rec_ptr, np.int32)
    aa, bb = _dev(rec_aa, np.uint8), _dev(rec_backbone, np.uint8)
    _native.check(_native.lib().cbgx_pocket_types(p(x), p(z), p(rp), n_rec, B, p(aa), p(bb), p(t), _native.current_stream(DEV)),
                  "cbgx_pocket_types")
    torch.cuda.synchronize()
    out = t.cpu().numpy()
    assert (out[n_rec:] == 255).all()
    return out[:n_rec]


def run(x_lig, z_lig, lig_ptr, x_rec, rec_type, rec_ptr, bond_ptr, bond_index, bond_kekule, bond_aromatic, implicit_h, atom_flags,
        valence_status):
    """cbgx_ligand_interactions on 0xFF outputs with guard tails -> the model's dict without the abs sums; the guards are checked here"""
    n_lig, n_rec, B = len(z_lig), len(rec_type), len(lig_ptr) - 1
    bi = _dev(np.asarray(bond_index, np.int32).reshape(2, -1), np.int32)
    nb = bi.shape[1]
    ba = None if bond_aromatic is None else _dev(bond_aromatic, np.uint8)
    at, gt = _ff(n_lig * 5 + GUARD, torch.float64), _ff(B * 5 + GUARD, torch.float64)
    lt, br, gc = _ff(n_lig + GUARD, torch.uint8), _ff(nb + GUARD, torch.uint8), _ff(B * IM.COLS + GUARD, torch.int32)
    p = _native.ptr
    keep = [_dev(np.asarray(x_lig, np.float32).reshape(-1, 3), np.float32), _dev(z_lig, np.uint8), _dev(lig_ptr, np.int32),
            _dev(np.asarray(x_rec, np.float32).reshape(-1, 3), np.float32), _dev(rec_type, np.uint8), _dev(rec_ptr, np.int32),
            _dev(bond_ptr, np.int32), _dev(bond_kekule, np.uint8), _dev(implicit_h, np.uint8), _dev(atom_flags, np.uint8),
            _dev(valence_status, np.int32)]
    xl, zl, lp, xr, rt, rp, bp, bk, ih, af, vs = keep
    _native.check(_native.lib().cbgx_ligand_interactions(
        p(xl), p(zl), p(lp), n_lig, p(xr), p(rt), p(rp), n_rec, B, p(bp), p(bi) if nb else None, p(bk) if nb else None,
        p(ba) if ba is not None and nb else None, nb, p(ih), p(af), p(vs), p(at), p(lt), p(br), p(gt), p(gc), _native.current_stream(DEV)),
        "cbgx_ligand_interactions")
    torch.cuda.synchronize()
    at, gt, lt, br, gc = at.cpu().numpy(), gt.cpu().numpy(), lt.cpu().numpy(), br.cpu().numpy(), gc.cpu().numpy()
    assert (at[n_lig * 5:].view(np.uint8) == 255).all() and (gt[B * 5:].view(np.uint8) == 255).all()
    assert (lt[n_lig:] == 255).all() and (br[nb:] == 255).all() and (gc[B * IM.COLS:] == -1).all()
    return {"atom_terms": at[:n_lig * 5].reshape(n_lig, 5), "lig_type": lt[:n_lig], "bond_rotatable": br[:nb],
            "graph_terms": gt[:B * 5].reshape(B, 5), "graph_out": gc[:B * IM.COLS].reshape(B, IM.COLS)}


def close(got, want):
    """integers and bytes ==; floats within BOUND * sum|addends| of the model, nan exactly where the model has nan (an element the kernel
    does not write keeps its 0xFF bytes, which are a nan)"""
    for k in ("lig_type", "bond_rotatable", "graph_out"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:10].tolist())
    for k, scale in (("atom_terms", "atom_abs"), ("graph_terms", "graph_abs")):
        g, w, s = got[k], want[k], want[scale]
        assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), k
        ok = ~np.isnan(w)
        err, bound = np.abs(g[ok] - w[ok]), BOUND * s[ok]
        assert (err <= bound).all(), (k, float(err.max()), np.argwhere(~(np.abs(g - w) <= BOUND * s) & ok)[:10].tolist())


def bits(out):
    return {k: (v.view(np.uint64) if v.dtype == np.float64 else v) for k, v in out.items()}


def check(args):
    want = IM.batch_interactions(**args)
    got = run(**args)
    close(got, want)
    return got, want


# ---- the hand cases ----------------------------------------------------------------------------------------------------------------------------
def test_hand_pairs_at_every_breakpoint_and_at_the_cutoff():
    args = hand_batch()
    got, want = check(args)
    by_name = {p[0]: g for g, p in enumerate(hand_pairs())}
    n_pairs = {name: int(got["graph_out"][g, 6]) for name, g in by_name.items() if name.startswith("r_")}
    assert n_pairs == {"r_eight": 0, "r_eight_diagonal": 0, "r_float32_below_eight": 1, "r_double_below_eight": 1, "r_above_eight": 0}
    # one pair per graph: one addend per sum, so everything but exp is exact
    assert np.array_equal(got["graph_terms"][:, 2:], want["graph_terms"][:, 2:]) and np.array_equal(got["atom_terms"], got["graph_terms"])
    assert got["graph_terms"][by_name["F_S_hyd@d0.5@1"], 3] == 1.0 and got["graph_terms"][by_name["F_S_hyd@d1.5@1"], 3] == 0.0
    assert got["graph_terms"][by_name["O_acc_N_don@d0.0@1"], 4] == 0.0 and got["graph_terms"][by_name["O_acc_N_don@d-0.7@0"], 4] == 1.0


def test_hand_molecules_in_one_batch():
    """the 21 hand molecules of tests/test_interactions.py with the valence model's outputs, each in a seeded pocket of 60 - 120 atoms: the device
    gives the types and rotatable bonds written down there (and everything else the model gives).  The batch holds what the seeded sets
    lack: a triple bond, explicit hydrogens, an aromatic bridge whose bond_kekule is 1, a phosphorus atom"""
    names = list(MOLECULES)
    cases = [MOLECULES[k][0] for k in names]
    rng = random.Random(53)
    args, _ = assemble(cases, [make_pocket(rng, rng.randint(60, 120)) for _ in cases], [ligand_coordinates(rng, c[0]) for c in cases])
    assert (args["valence_status"] == 0).all()
    got, want = check(args)
    assert (got["graph_out"][:, -1] == 0).all()
    lp, bp, idx = args["lig_ptr"], args["bond_ptr"], args["bond_index"]
    for g, name in enumerate(names):
        _, types, rotatable = MOLECULES[name]
        b0, b1 = int(bp[lp[g]]), int(bp[lp[g + 1]])
        assert {a: int(got["lig_type"][lp[g] + a]) for a in types} == types, name
        pairs = [(int(i - lp[g]), int(j - lp[g])) for i, j in idx[:, b0:b1].T]
        assert [e for e, r in zip(pairs, got["bond_rotatable"][b0:b1]) if r] == rotatable and got["graph_out"][g, 2] == len(rotatable), name
    # what makes those rules decisive is in the batch
    z, kek, aro = args["z_lig"], args["bond_kekule"], args["bond_aromatic"]
    assert (kek == 3).sum() == 2 and 15 in z and (z[idx[1]] == 1).sum() == 4
    g = names.index("next_to_triple")
    b0 = int(bp[lp[g]])
    assert kek[b0:b0 + 4].tolist() == [1, 1, 3, 1] and got["bond_rotatable"][b0:b0 + 4].tolist() == [0, 0, 0, 0]
    g = names.index("aromatic_bridge")
    at = int(bp[lp[g]]) + 1
    assert (idx[:, at] - lp[g]).tolist() == [1, 2] and aro[at] == 1 and kek[at] == 1 and got["bond_rotatable"][at] == 0
    plain = run(**dict(args, bond_aromatic=None))                       # the same bytes without the aromatic ones: now it rotates
    assert plain["bond_rotatable"][at] == 1 and (plain["bond_rotatable"] != got["bond_rotatable"]).sum() == 1
    g = names.index("explicit_h")
    assert args["implicit_h"][lp[g] + 1] == 0 and got["lig_type"][lp[g] + 1] == 3 | IM.DON | IM.ACC and got["lig_type"][lp[g] + 2] == 0
    assert got["graph_out"][g, 2] == 0 and got["graph_out"][g, 3] == 1
    g = names.index("halides")
    assert got["lig_type"][lp[g] + 3] == 5 and got["atom_terms"][lp[g] + 3, 1] > 0.0 and got["atom_terms"][lp[g] + 3, 3] == 0.0


def test_typing_table_and_threshold_carbons():
    """the pocket kernel on the atoms of the residue table (all 20 residues and "other" x backbone / side chain x C, N, O, S, Se, H, P, F,
    0) and on the carbons around the table-bond threshold of C-N, C-O and C-S: the types written down in tests/test_interactions.py"""
    x, z, aa, bb, want = typing_table_atoms()
    n = len(z)
    assert run_pocket(x, z, [0, n], aa, bb).tolist() == want
    assert run_pocket(x, z, [0, 7, 200, 201, n], aa, bb).tolist() == want       # far apart: the same in any split into graphs
    pocket, want = threshold_pocket()
    got = run_pocket(**pocket)
    assert got[1::2].tolist() == want and {1, 1 | IM.HYD} == set(want) and np.array_equal(got, IM.pocket_types(**pocket))
    cases = threshold_carbons()
    for z_other, pm in C_X_SINGLE_PM:       # the three float32 distances around each threshold fall on both sides of it
        around = [(c[1], int(t)) for c, t in zip(cases, got[1::2]) if c[0] == z_other and abs(c[1] - (pm + 10) / 100.0) < 1e-5]
        assert len(around) == 3 and {t for _, t in around} == {1, 1 | IM.HYD}, around
    # one graph for all pairs: the carbons 100 A apart see only their own partner
    assert run_pocket(**dict(pocket, rec_ptr=[0, len(pocket["z_rec"])]))[1::2].tolist() == want


def test_host_memory_is_refused_for_every_array():
    """any array with a non-zero count that is plain host memory is refused before a launch and named, not only the first CSR"""
    _, (args, pocket) = three_graphs()
    lib, p = _native.lib(), _native.ptr
    host = np.zeros(4096, np.uint8)
    bad = ctypes.c_void_p(host.ctypes.data)
    dev = {k: _dev(v, dt) for k, v, dt in (("x_rec", pocket["x_rec"], np.float32), ("z_rec", pocket["z_rec"], np.uint8),
                                           ("rec_ptr", pocket["rec_ptr"], np.int32), ("rec_aa", pocket["rec_aa"], np.uint8),
                                           ("rec_backbone", pocket["rec_backbone"], np.uint8))}
    n_rec, out = len(pocket["z_rec"]), _ff(len(pocket["z_rec"]), torch.uint8)
    order = ("x_rec", "z_rec", "rec_ptr", "rec_aa", "rec_backbone")
    for name in order + ("rec_type",):
        a = [bad if k == name else p(dev[k]) for k in order] + [bad if name == "rec_type" else p(out)]
        assert lib.cbgx_pocket_types(a[0], a[1], a[2], n_rec, 3, a[3], a[4], a[5], None) == -1
        assert f"{name} is not memory the device can read" in lib.cbgx_last_error().decode(), name
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 255).all()                              # nothing was launched
    n_lig, nb = len(args["z_lig"]), args["bond_index"].shape[1]
    t = {"x_lig": _dev(args["x_lig"], np.float32), "z_lig": _dev(args["z_lig"], np.uint8), "lig_ptr": _dev(args["lig_ptr"], np.int32),
         "x_rec": dev["x_rec"], "rec_type": _dev(args["rec_type"], np.uint8), "rec_ptr": dev["rec_ptr"],
         "bond_ptr": _dev(args["bond_ptr"], np.int32), "bond_index": _dev(args["bond_index"], np.int32),
         "bond_kekule": _dev(args["bond_kekule"], np.uint8), "bond_aromatic": _dev(args["bond_aromatic"], np.uint8),
         "implicit_h": _dev(args["implicit_h"], np.uint8), "atom_flags": _dev(args["atom_flags"], np.uint8),
         "valence_status": _dev(args["valence_status"], np.int32), "atom_terms": _ff(n_lig * 5, torch.float64),
         "lig_type": _ff(n_lig, torch.uint8), "bond_rotatable": _ff(nb, torch.uint8), "graph_terms": _ff(15, torch.float64),
         "graph_out": _ff(3 * IM.COLS, torch.int32)}
    for name in t:
        a = {k: (bad if k == name else p(v)) for k, v in t.items()}
        rc = lib.cbgx_ligand_interactions(a["x_lig"], a["z_lig"], a["lig_ptr"], n_lig, a["x_rec"], a["rec_type"], a["rec_ptr"], n_rec, 3,
                                          a["bond_ptr"], a["bond_index"], a["bond_kekule"], a["bond_aromatic"], nb, a["implicit_h"],
                                          a["atom_flags"], a["valence_status"], a["atom_terms"], a["lig_type"], a["bond_rotatable"],
                                          a["graph_terms"], a["graph_out"], None)
        assert rc == -1 and f"{name} is not memory the device can read" in lib.cbgx_last_error().decode(), name
    torch.cuda.synchronize()
    assert (t["graph_out"].cpu().numpy() == -1).all() and (t["lig_type"].cpu().numpy() == 255).all()


# ---- seeded molecule-like graphs in seeded pockets ---------------------------------------------------------------------------------------------
def test_three_hundred_and_twenty_seeded_graphs_in_seeded_pockets():
    args, pocket, want = seeded_interactions()
    assert len(args["lig_ptr"]) - 1 >= 300 and (want["graph_out"][:, -1] == 0).all()
    rec_type = run_pocket(**pocket)
    assert rec_type.dtype == np.uint8 and np.array_equal(rec_type, args["rec_type"]), np.argwhere(rec_type != args["rec_type"])[:10].tolist()
    close(run(**dict(args, rec_type=rec_type)), want)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------
def sized_case(n):
    return HAND["empty"][0] if n == 0 else HAND["one_carbon"][0] if n == 1 else benzene_with_pendants(n)


def test_ligand_and_pocket_sizes():
    """ligands of 0, 1, 63, 64, 65, 255, 256 and 257 atoms (the last: status) and pockets of 0, 1, 255, 256, 257 and 1025 atoms, each size
    of one side against several of the other"""
    rng = random.Random(19)
    lig_sizes = [0, 1, 63, 64, 65, 255, 256, 257, 30, 30, 30, 30, 30, 30, 0, 1]
    rec_sizes = [257, 1025, 256, 255, 1, 0, 1025, 300, 0, 1, 255, 256, 257, 1025, 0, 1]
    cases = [sized_case(n) for n in lig_sizes]
    args, pocket = assemble(cases, [make_pocket(rng, n, ("Se", "H")) for n in rec_sizes], [ligand_coordinates(rng, n) for n in lig_sizes])
    rec_type = run_pocket(**pocket)
    assert np.array_equal(rec_type, args["rec_type"])
    got, want = check(args)
    assert got["graph_out"][:, 0].tolist() == lig_sizes and got["graph_out"][:, -1].tolist() == [0] * 7 + [9] + [0] * 8
    assert got["graph_out"][7].tolist() == [257, 257] + [-1] * 10 + [IM.TOO_MANY_ATOMS | IM.NO_VALENCE]
    assert got["graph_out"][6, 6] > 10000 and got["graph_out"][6, 2] > 100 and got["graph_out"][1, 6] > 0 and got["graph_out"][5, 6] == 0
    # a pocket without a ligand: nothing but its own untyped atoms
    assert (got["graph_out"][[0, 14], 2:11] == 0).all() and (got["graph_out"][[0, 1, 6, 13], 11] > 0).all() and got["graph_out"][14, 11] == 0
    # more than 256 atoms with a valence status of 0 handed in: its own bit alone (and the 255 bytes of bond_kekule are not looked at)
    status = args["valence_status"].copy()
    status[7] = 0
    kek = np.where(args["bond_kekule"] == 255, 1, args["bond_kekule"]).astype(np.uint8)
    got, _ = check(dict(args, valence_status=status, bond_kekule=kek))
    assert got["graph_out"][7, -1] == IM.TOO_MANY_ATOMS


def test_no_graphs_and_no_atoms():
    e = np.zeros(0)
    out = run(np.zeros((0, 3)), e, [0], np.zeros((0, 3)), e, [0], [0], np.zeros((2, 0)), e, None, e, e, e)
    assert out["graph_out"].shape == (0, 13) and out["graph_terms"].shape == (0, 5)
    assert run_pocket(np.zeros((0, 3)), e, [0], e, e).shape == (0,)
    # graphs without atoms on either side
    args = dict(x_lig=np.zeros((0, 3)), z_lig=e, lig_ptr=[0, 0, 0], x_rec=np.zeros((0, 3)), rec_type=e, rec_ptr=[0, 0, 0], bond_ptr=[0],
                bond_index=np.zeros((2, 0)), bond_kekule=e, bond_aromatic=None, implicit_h=e, atom_flags=e, valence_status=[0, 0])
    got, _ = check(args)
    assert got["graph_out"].tolist() == [[0] * 13] * 2 and got["graph_terms"].tolist() == [[0.0] * 5] * 2
    dev_e = torch.zeros(0, device=DEV)
    assert G.pocket_types(torch.zeros(0, 3, device=DEV), dev_e.long(), dev_e.long(), 0, dev_e.long(), dev_e).shape == (0,)


def three_graphs():
    cases = [HAND["naphthalene"][0], HAND["pyridone"][0], HAND["biphenyl"][0]]
    rng = random.Random(23)
    return cases, assemble(cases, [make_pocket(rng, n) for n in (90, 70, 110)], [ligand_coordinates(rng, c[0]) for c in cases])


def test_a_graph_the_valence_report_gave_up():
    cases, (args, _) = three_graphs()
    clean, _ = check(args)
    # what cbgx_ligand_valence writes for a graph over its step budget: status, and 255 in its three arrays
    z, lig_ptr, n_lig, bond_ptr, idx, order, aro = collate(cases[:2])
    h2, f2, k2, vout = VM.batch_valence(z, lig_ptr, n_lig, bond_ptr, idx, order, aro, max_steps=7)
    assert vout[:, -1].tolist() == [VM.SEARCH_LIMIT, VM.SEARCH_LIMIT] and (h2 == 255).all() and (k2 == 255).all()
    h, f, k, status = (args[name].copy() for name in ("implicit_h", "atom_flags", "bond_kekule", "valence_status"))
    h[:17], f[:17], k[:18], status[:2] = h2, f2, k2, vout[:, -1]
    gave_up = dict(args, implicit_h=h, atom_flags=f, bond_kekule=k, valence_status=status)
    got, want = check(gave_up)
    assert got["graph_out"][:, -1].tolist() == [IM.NO_VALENCE, IM.NO_VALENCE, 0] and got["graph_out"][1].tolist() == [7, 7] + [-1] * 10 + [8]
    assert np.isnan(got["graph_terms"][:2]).all() and (got["lig_type"][:17] == 255).all() and (got["bond_rotatable"][:18] == 255).all()
    for k in got:
        lo, hi = {"atom_terms": (17, 29), "lig_type": (17, 29), "bond_rotatable": (18, 31), "graph_terms": (2, 3), "graph_out": (2, 3)}[k]
        assert np.array_equal(bits(got)[k][lo:hi], bits(clean)[k][lo:hi]), k


# ---- malformed input stays inside the buffers ----------------------------------------------------------------------------------------------
def test_malformed_ranges_and_lists_are_reported_and_clamped():
    """naphthalene | pyridone with a broken list | biphenyl: the broken graph carries BAD_BONDS, -1, nan and 255, its neighbours their clean
    results bit for bit, and the guard tails stay 0xFF (checked in ``run``)"""
    cases, (args, pocket) = three_graphs()
    clean, _ = check(args)
    assert clean["graph_out"][:, -1].tolist() == [0, 0, 0]
    lig_ptr, bond_ptr, n_lig = args["lig_ptr"], args["bond_ptr"], len(args["z_lig"])
    b0, b1, a0 = int(bond_ptr[lig_ptr[1]]), int(bond_ptr[lig_ptr[2]]), int(lig_ptr[1])

    def swap(bp, bi, bk):             # a bond with j <= i
        bi[:, b0 + 2] = bi[::-1, b0 + 2].copy()

    def equal(bp, bi, bk):
        bi[1, b0 + 1] = bi[0, b0 + 1]

    def leaves(bp, bi, bk):           # a bond that leaves the graph's atom range: into the next graph
        bi[1, b1 - 1] = lig_ptr[2] + 1

    def wild(bp, bi, bk):             # rows no array has
        bi[0, b0] = -7
        bi[1, b0 + 3] = 2 ** 31 - 1
        bi[1, b0 + 4] = n_lig + 1000

    def out_of_order(bp, bi, bk):     # two bonds exchanged
        bi[:, [b0, b0 + 1]] = bi[:, [b0 + 1, b0]]

    def pointer(bp, bi, bk):          # non-monotone inside the graph; the graph's own range is what it was
        bp[a0 + 2] = bp[a0 + 3] + 2

    def kekule_zero(bp, bi, bk):
        bk[b0 + 5] = 0

    def kekule_five(bp, bi, bk):
        bk[b1 - 1] = 5

    def everything(bp, bi, bk):
        swap(bp, bi, bk), leaves(bp, bi, bk), pointer(bp, bi, bk), kekule_zero(bp, bi, bk)

    for what in (swap, equal, leaves, wild, out_of_order, pointer, kekule_zero, kekule_five, everything):
        bp, bi, bk = bond_ptr.copy(), args["bond_index"].copy(), args["bond_kekule"].copy()
        what(bp, bi, bk)
        got, want = check(dict(args, bond_ptr=bp, bond_index=bi, bond_kekule=bk))
        assert got["graph_out"][:, -1].tolist() == [0, IM.BAD_BONDS, 0], what.__name__
        assert got["graph_out"][1].tolist() == [7, 7] + [-1] * 10 + [IM.BAD_BONDS] and np.isnan(got["graph_terms"][1]).all()
        assert (got["lig_type"][a0:lig_ptr[2]] == 255).all() and (got["bond_rotatable"][b0:b1] == 255).all()
        assert np.isnan(got["atom_terms"][a0:lig_ptr[2]]).all()
        for g in (0, 2):
            lo, hi = bond_ptr[lig_ptr[g]], bond_ptr[lig_ptr[g + 1]]
            assert np.array_equal(got["graph_out"][g], clean["graph_out"][g]) and np.array_equal(got["bond_rotatable"][lo:hi], clean["bond_rotatable"][lo:hi])
            assert np.array_equal(bits(got)["graph_terms"][g], bits(clean)["graph_terms"][g]), (what.__name__, g)
            assert np.array_equal(bits(got)["atom_terms"][lig_ptr[g]:lig_ptr[g + 1]], bits(clean)["atom_terms"][lig_ptr[g]:lig_ptr[g + 1]])
    # bond pointers outside the list at a graph boundary
    bp = bond_ptr.copy()
    bp[lig_ptr[2]] = args["bond_index"].shape[1] + 500
    bp[lig_ptr[1]] = -3
    got, _ = check(dict(args, bond_ptr=bp))
    assert (got["graph_out"][:, -1] == IM.BAD_BONDS).all()
    # lig_ptr and rec_ptr outside their arrays are clamped: the same graphs, the same bits
    lp, rp = lig_ptr.copy(), args["rec_ptr"].copy()
    lp[0], lp[3], rp[0], rp[3] = -4, n_lig + 77, -9, len(args["rec_type"]) + 1000
    got, _ = check(dict(args, lig_ptr=lp, rec_ptr=rp))
    for k in got:
        assert np.array_equal(bits(got)[k], bits(clean)[k]), k
    assert np.array_equal(run_pocket(**dict(pocket, rec_ptr=rp)), args["rec_type"])
    # ranges that cover only a part: atoms, bonds and pocket atoms outside every graph's range are not written (they keep 0xFF)
    lp, rp = np.array([0, 10, 10, 17], np.int32), np.array([5, 60, 95, 150], np.int32)
    got, want = check(dict(args, lig_ptr=lp, rec_ptr=rp))
    assert got["graph_out"][:, 0].tolist() == [10, 0, 7] and (got["lig_type"][17:] == 255).all()
    assert (got["atom_terms"][17:].view(np.uint8) == 255).all() and (got["bond_rotatable"][18:] == 255).all()
    part = run_pocket(**dict(pocket, rec_ptr=rp))
    assert (part[:5] == 255).all() and (part[150:] == 255).all() and np.array_equal(part, IM.pocket_types(**dict(pocket, rec_ptr=rp)))


# ---- placement ---------------------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_place_in_the_batch():
    """the same graph alone, first, last and in the middle of a 65-graph batch: the same bits"""
    rng = random.Random(31)
    cases = [benzene_with_pendants(n) for n in (40, 200)] + [HAND["pyridone"][0]]
    pockets = [make_pocket(rng, n) for n in (500, 1025, 3)]
    coords = [ligand_coordinates(rng, c[0]) for c in cases]
    from tests.test_valence import seeded_sets
    fill = list(seeded_sets()[0][:64])
    fill_pockets = [make_pocket(rng, rng.randint(40, 300)) for _ in fill]
    fill_coords = [ligand_coordinates(rng, c[0]) for c in fill]
    for case, pocket, xyz in zip(cases, pockets, coords):
        alone_args, _ = assemble([case], [pocket], [xyz])
        alone = bits(run(**alone_args))
        n, m = case[0], len(case[1])
        for at in (0, 32, 64):
            args, _ = assemble(fill[:at] + [case] + fill[at:], fill_pockets[:at] + [pocket] + fill_pockets[at:],
                               fill_coords[:at] + [xyz] + fill_coords[at:])
            assert len(args["lig_ptr"]) == 66
            got = bits(run(**args))
            l0, b0 = int(args["lig_ptr"][at]), int(args["bond_ptr"][args["lig_ptr"][at]])
            assert np.array_equal(got["graph_terms"][at], alone["graph_terms"][0]) and np.array_equal(got["graph_out"][at], alone["graph_out"][0])
            assert np.array_equal(got["atom_terms"][l0:l0 + n], alone["atom_terms"]) and np.array_equal(got["lig_type"][l0:l0 + n], alone["lig_type"])
            assert np.array_equal(got["bond_rotatable"][b0:b0 + m], alone["bond_rotatable"])
        assert alone["graph_out"][0, 6] > 0 or len(pocket[1]) < 100


# ---- from coordinates, the Python entries ----------------------------------------------------------------------------------------------------
def test_from_coordinates_through_batch_interactions():
    """graph 0: biphenyl (two hexagons at 1.40 A, a 1.48 A link), aromatic carbon types; graph 1: 2-pyridone; graph 2: an ethanol-like
    C-C-O chain of 'basic'-looking plain types inside add_aromatic (C = 1, O = 5); each in a seeded pocket shifted to sit around it"""
    ang = np.arange(6) * np.pi / 3
    hexagon = np.stack([1.40 * np.cos(ang), 1.40 * np.sin(ang), 0 * ang], 1)
    second = hexagon * [-1, 1, 1] + [1.40 + 1.48 + 1.40, 0, 0]
    pyridone = np.concatenate([hexagon, hexagon[1:2] * (1.40 + 1.22) / 1.40]) + [0, 40.0, 0]
    ethanol = np.array([[0, 80.0, 0], [1.52, 80.0, 0], [2.2, 81.2, 0]])
    x_lig = np.concatenate([hexagon, second, pyridone, ethanol]).astype(np.float32)
    c = torch.tensor([2] * 12 + [4, 2, 2, 2, 2, 2, 5] + [1, 1, 5], dtype=torch.long, device=DEV)
    lig_b = torch.tensor([0] * 12 + [1] * 7 + [2] * 3, device=DEV)
    rng = random.Random(41)
    pockets = [make_pocket(rng, n, must) for n, must in ((300, ("Se",)), (257, ("H", "HIS")), (120, ("PRO",)))]
    centres = [x_lig[:12].mean(0), x_lig[12:19].mean(0), x_lig[19:].mean(0)]
    x_rec = np.concatenate([p[0] + ctr for p, ctr in zip(pockets, centres)]).astype(np.float32)
    z_rec, aa, bb = (np.concatenate([p[k] for p in pockets]) for k in (1, 2, 3))
    rec_b = np.repeat(np.arange(3), [len(p[1]) for p in pockets])
    feat = np.zeros((len(z_rec), 7), np.float32)
    feat[:, 6] = bb
    batch = {"num_graphs": 3, "protein_pos": torch.from_numpy(x_rec).to(DEV), "protein_element": torch.from_numpy(z_rec.astype(np.int64)).to(DEV),
             "protein_element_batch": torch.from_numpy(rec_b).to(DEV), "protein_aa_type": torch.from_numpy(aa.astype(np.int64)).to(DEV),
             "protein_atom_feature": torch.from_numpy(feat).to(DEV)}
    x = torch.from_numpy(x_lig).to(DEV)
    out = G.batch_interactions(batch, x, c, lig_b, "add_aromatic")
    assert sorted(out) == ["atom_terms", "bond_rotatable", "graph_counts", "graph_terms", "lig_type", "rec_type"]
    assert all(v.device.type == "cuda" for v in out.values())
    assert (out["atom_terms"].dtype, out["graph_terms"].dtype, out["graph_counts"].dtype, out["lig_type"].dtype) == (
        torch.float64, torch.float64, torch.int32, torch.uint8)
    gc = out["graph_counts"].cpu().numpy()
    assert gc[:, -1].tolist() == [0, 0, 0] and gc[:, 2].tolist() == [1, 0, 0] and gc[:, 0].tolist() == [12, 7, 3] and (gc[:, 6] > 50).all()
    assert gc[0, 11] >= 1                                                              # the selenium of pocket 0
    HYD, DON, ACC = IM.HYD, IM.DON, IM.ACC
    assert out["lig_type"].tolist() == [1 | HYD] * 12 + [2 | DON, 1, 1 | HYD, 1 | HYD, 1 | HYD, 1, 3 | ACC] + [1 | HYD, 1, 3 | DON | ACC]
    assert out["bond_rotatable"].tolist().count(1) == 1
    # against the model on the lists the device made
    bonds = G.batch_bonds(batch, x, c, lig_b, "add_aromatic")
    val = G.batch_valence(batch, x, c, lig_b, "add_aromatic", bonds=bonds)
    z = torch.tensor(C.config._ATOMIC_NUMBER["add_aromatic"], device=DEV)[c].cpu().numpy()
    idx = bonds["bond_index"].cpu().numpy()
    rec_ptr = np.concatenate([[0], np.cumsum([len(p[1]) for p in pockets])])
    rec_type = IM.pocket_types(x_rec, z_rec, rec_ptr, aa, bb)
    assert np.array_equal(out["rec_type"].cpu().numpy(), rec_type)
    want = IM.batch_interactions(x_lig, z, [0, 12, 19, 22], x_rec, rec_type, rec_ptr,
                                 np.concatenate([[0], np.cumsum(np.bincount(idx[0], minlength=22))]), idx, val["bond_kekule"].cpu().numpy(), None,
                                 val["implicit_h"].cpu().numpy(), val["atom_flags"].cpu().numpy(), val["graph_counts"][:, -1].cpu().numpy())
    got = {k: out[k].cpu().numpy() for k in ("atom_terms", "lig_type", "bond_rotatable", "graph_terms")}
    got["graph_out"] = gc
    close(got, want)
    # given or computed here, with or without the aromatic bytes: the same bits (an aromatic bond of that report is never a bridge)
    aro = G.batch_aromatic(batch, x, c, lig_b, "add_aromatic", bonds=bonds)
    again = G.batch_interactions(batch, x, c, lig_b, "add_aromatic", bonds=bonds, valence=val)
    direct = G.ligand_interactions(x, torch.from_numpy(z).to(DEV), lig_b, batch["protein_pos"], out["rec_type"], batch["protein_element_batch"],
                                   3, bonds, val, aromatic=aro)
    for k in direct:
        assert torch.equal(again[k].view(torch.uint8), out[k].view(torch.uint8)) and torch.equal(direct[k].view(torch.uint8), out[k].view(torch.uint8)), k
    # the host's score of those rows
    inter, score = G.interaction_scores(gc, out["graph_terms"])
    mi, ms = IM.scores(gc, got["graph_terms"])
    assert np.array_equal(inter, mi) and np.array_equal(score, ms) and score[0] == inter[0] / (1.0 + 0.05846) and score[1] == inter[1]
    s = G.summarise_interactions(gc, out["graph_terms"])
    assert s["counts"]["n_mol_evaluated"] == 3 and s["mean_score"] == (sum(int(np.rint(v * 1e6)) for v in score) / 1e6) / 3


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
def _records(out_dir, n):
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".pt"))
    assert files == [f"pocket_{i:05d}.pt" for i in range(n)]
    return [torch.load(os.path.join(out_dir, f), map_location="cpu", weights_only=False) for f in files]


def _same_field(a, b):
    return _equal(a, b) or (torch.is_tensor(a) and a.is_floating_point() and torch.equal(a.isnan(), b.isnan())
                            and torch.equal(a.nan_to_num(), b.nan_to_num())) or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


def test_sample_cli_interactions(tmp_path, capsys):
    """the T = 20 fixture config, three synthetic pockets x two samples, --noise counter, one saved random checkpoint"""
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    config, _ = C.load_config(cfg)
    C.set_num_atom_type(config)
    torch.manual_seed(123)
    ckpt = tmp_path / "random_init.pt"
    torch.save({"model": C.get_model(config.model).state_dict()}, ckpt)
    tail = ["--synthetic", "3", "--num_samples", "2", "--seed", "2024", "--noise", "counter", "--no_translate"]

    def go(tag, *extra):
        out, stats = tmp_path / tag, {}
        assert sample_cli.main(["--config", cfg, "--checkpoint", str(ckpt), *tail, "--out_root", str(out)] + list(extra), stats=stats) == 0
        d = str(out / os.path.splitext(os.path.basename(cfg))[0])
        return d, _records(d, 3), stats

    def text(d, name):
        with open(os.path.join(d, name)) as f:
            return f.read()

    whole = ("--pockets_per_batch", "3", "--streams", "1")
    dir_base, base, stats_base = go("base", *whole)
    dir_ia, alone, stats_ia = go("ia", *whole, "--interactions")
    dir_val, val, _ = go("val", *whole, "--valence", "--bonds", "--sdf")
    dir_all, both, stats_all = go("all", *whole, "--interactions", "--valence", "--bonds", "--sdf")
    _, split, _ = go("split", "--pockets_per_batch", "1", "--streams", "1", "--interactions")
    printed = capsys.readouterr().out
    assert printed.count("interactions: mean_score ") == 3 and printed.count("not the Vina program") == 3
    assert stats_ia["interactions"] > 0.0 and stats_all["interactions"] > 0.0 and "interactions" not in stats_base
    assert not {"bonds", "rings", "aromatic", "valence"} & set(stats_ia)

    # without the flag nothing of it is written, and what is written does not change with it: byte for byte for the text files, field by
    # field outside the new keys for the records
    assert not os.path.exists(os.path.join(dir_base, "interactions_summary.json")) and not os.path.exists(os.path.join(dir_val, "interactions_summary.json"))
    assert sorted(os.listdir(dir_ia)) == sorted(os.listdir(dir_base) + ["interactions_summary.json"])
    assert sorted(os.listdir(dir_all)) == sorted(os.listdir(dir_val) + ["interactions_summary.json"])
    for name in os.listdir(dir_val):
        if not name.endswith(".pt"):
            assert text(dir_all, name) == text(dir_val, name), name
    for without, with_it in ((base, alone), (val, both)):
        for r, r2 in zip(without, with_it):
            assert sorted(set(r2) - set(r)) == ["interactions"] and all(_same_field(r[k], r2[k]) for k in r if k != "samples")
            for s, s2 in zip(r["samples"], r2["samples"]):
                assert sorted(set(s2) - set(s)) == sorted(INTERACTION_FIELDS)
                assert all(_same_field(s[k], s2[k]) for k in s), [k for k in s if not _same_field(s[k], s2[k])]

    # the new fields: alone, with the other flags and in 1-pocket batches they are the same bits; and they are the model's on the graph
    # the file holds, in the pocket the job made
    rows, all_terms = [], []
    for rb, ra, rs in zip(both, alone, split):
        assert rb["interactions"] == ra["interactions"] == rs["interactions"] and set(rb["interactions"]) == set(G.INTERACTION_COUNT_KEYS)
        assert all(isinstance(v, int) for v in rb["interactions"].values())
        mine, terms = [], []
        for sb, sa, ss in zip(rb["samples"], ra["samples"], rs["samples"]):
            for k in INTERACTION_FIELDS:
                assert _same_field(sb[k], sa[k]) and _same_field(sb[k], ss[k]), k
            n, nb = len(sb["atom"]), sb["bond_index"].shape[1]
            assert sb["lig_xs_type"].dtype == sb["bond_rotatable"].dtype == torch.uint8 and sb["atom_terms"].dtype == torch.float64
            assert sb["lig_xs_type"].shape == (n,) and sb["atom_terms"].shape == (n, 5) and sb["bond_rotatable"].shape == (nb,)
            assert sb["interaction_terms"].shape == (5,) and isinstance(sb["score"], float) and isinstance(sb["n_rotatable"], int)
            row = [n, nb, sb["n_rotatable"], int(((sb["lig_xs_type"] & 16) != 0).sum()), int(((sb["lig_xs_type"] & 32) != 0).sum()),
                   int(((sb["lig_xs_type"] & 8) != 0).sum()), 0, sb["n_hbond_pairs"], sb["n_hydrophobic_pairs"], sb["n_close_pairs"],
                   sb["n_contact_atoms"], 0, sb["interactions_status"]]
            if sb["interactions_status"] == 0:
                # ligand types and rotatable bonds of the model on the graph and the valence fields the file holds
                types, rot = IM.ligand_graph(n, list(zip(*sb["bond_index"].tolist())), [int(v) for v in sb["atom"]], sb["bond_kekule"].tolist(),
                                             [0] * nb, sb["implicit_h"].tolist(), sb["valence_flags"].tolist())
                assert sb["lig_xs_type"].tolist() == types and sb["bond_rotatable"].tolist() == rot and sb["n_rotatable"] == sum(rot)
                inter, score = G.interaction_scores([row], sb["interaction_terms"].numpy()[None])
                assert sb["score_inter"] == inter[0] and sb["score"] == score[0]
                assert np.allclose(sb["atom_terms"].sum(0).numpy(), sb["interaction_terms"].numpy(), rtol=1e-12, atol=0.0)
                assert sb["interaction_terms"][1] > 0.0
            else:
                assert np.isnan(sb["score"]) and sb["n_rotatable"] == -1
            mine.append(row)
            terms.append(sb["interaction_terms"].numpy())
        counts = G.summarise_interactions(np.array(mine), np.array(terms))["counts"]
        assert {k: v for k, v in rb["interactions"].items() if k not in ("n_pairs", "n_protein_untyped")} == {
            k: v for k, v in counts.items() if k not in ("n_pairs", "n_protein_untyped")}
        rows += mine
        all_terms += terms
    want = G.summarise_interactions(np.array(rows), np.array(all_terms))
    for d in (dir_ia, dir_all):
        summary = json.loads(text(d, "interactions_summary.json"))
        assert set(summary) == set(G.INTERACTION_RATIOS) | {"counts"} and summary["counts"]["n_mol"] == 6
        assert summary["counts"]["score_micro"] == sum(r["interactions"]["score_micro"] for r in both)
        for k in ("mean_score", "mean_score_inter", "negative_score_mol_ratio", "hbond_pairs_per_mol", "rotatable_per_mol", "mol_with_hbond_ratio",
                  "hydrophobic_pairs_per_mol", "close_pairs_per_mol"):
            assert summary[k] == want[k] or (np.isnan(summary[k]) and np.isnan(want[k])), k
    assert text(dir_ia, "interactions_summary.json") == text(dir_all, "interactions_summary.json")
