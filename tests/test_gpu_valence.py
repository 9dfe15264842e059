"""Kekule orders, implicit hydrogens and valence flags on the GPU (csrc/valence.hip: cbgx_ligand_valence; cbgbench_amd/geometry.py;
sample_cli --valence) against the plain-Python model of tests/valence_model.py.  Every comparison is ``==``: the results are integers.
Output buffers handed to the entry are pre-filled with 0xFF bytes and carry a 0xFF guard tail inside the same allocation, which must stay
as it is."""
import json
import os
import random

import networkx as nx
import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, geometry as G
from tests import valence_model as VM
from tests.test_aromatic import read_sdf
from tests.test_gpu_rings import DEV, GUARD, _dev, _equal, _ff, same
from tests.test_valence import HAND, collate, graph, relabel, ring, seeded_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(z, lig_ptr, n_lig, bond_ptr, bond_index, bond_order, bond_aromatic=None, max_steps=VM.MAX_STEPS):
    """the entry on 0xFF outputs with guard tails -> (implicit_h [n_lig], atom_flags [n_lig], bond_kekule [n_bonds], graph_out [B, 22]); the
    guards are checked here"""
    lp, bp, bi = _dev(lig_ptr, np.int32), _dev(bond_ptr, np.int32), _dev(np.asarray(bond_index, np.int32).reshape(2, -1), np.int32)
    zz, bo = _dev(z, np.uint8), _dev(bond_order, np.uint8)
    ba = None if bond_aromatic is None else _dev(bond_aromatic, np.uint8)
    B, nb = lp.shape[0] - 1, bi.shape[1]
    h, f, k = _ff(n_lig + GUARD, torch.uint8), _ff(n_lig + GUARD, torch.uint8), _ff(nb + GUARD, torch.uint8)
    gc = _ff(B * VM.COLS + GUARD, torch.int32)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_valence(p(zz), p(lp), n_lig, B, p(bp), p(bi) if nb else None, p(bo) if nb else None,
                                                    p(ba) if ba is not None and nb else None, nb, max_steps, p(h), p(f), p(k), p(gc),
                                                    _native.current_stream(DEV)), "cbgx_ligand_valence")
    torch.cuda.synchronize()
    h, f, k, gc = h.cpu().numpy(), f.cpu().numpy(), k.cpu().numpy(), gc.cpu().numpy()
    assert (h[n_lig:] == 255).all() and (f[n_lig:] == 255).all() and (k[nb:] == 255).all() and (gc[B * VM.COLS:] == -1).all()
    return h[:n_lig], f[:n_lig], k[:nb], gc[:B * VM.COLS].reshape(B, VM.COLS)


def check(cases, max_steps=VM.MAX_STEPS):
    """kernel == model on one batch of cases -> the model's outputs"""
    args = collate(cases)
    want = VM.batch_valence(*args, max_steps=max_steps)
    same(run(*args, max_steps=max_steps), want)
    return want


# ---- the hand cases --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    cases = [c for c, _, _, _ in HAND.values()]
    args = collate(cases)
    return cases, args, VM.batch_valence(*args)


def test_hand_cases_in_one_batch(hand):
    cases, args, want = hand
    lp, bp = args[1], args[3]
    for g, (name, (_, kekule, hydrogens, steps)) in enumerate(HAND.items()):
        assert want[2][bp[lp[g]]:bp[lp[g + 1]]].tolist() == kekule and want[0][lp[g]:lp[g + 1]].tolist() == hydrogens, name
        assert want[3][g, 20] == max(steps, default=0) and want[3][g, 21] == 0, name
    same(run(*args), want)


def test_each_graph_alone_twice_and_reversed(hand):
    cases, args, want = hand
    first, second = run(*args), run(*args)
    same(first, want)
    same(second, first)
    lp, bp = args[1], args[3]
    for g, case in enumerate(cases):
        h, f, k, gc = run(*collate([case]))
        assert np.array_equal(gc[0], first[3][g]) and np.array_equal(h, first[0][lp[g]:lp[g + 1]]), g
        assert np.array_equal(f, first[1][lp[g]:lp[g + 1]]) and np.array_equal(k, first[2][bp[lp[g]]:bp[lp[g + 1]]]), g
    back = collate(cases[::-1])
    h, f, k, gc = run(*back)
    assert np.array_equal(gc[::-1], first[3])
    lpb, bpb = back[1], back[3]
    for g in range(len(cases)):
        r = len(cases) - 1 - g
        assert np.array_equal(h[lpb[r]:lpb[r + 1]], first[0][lp[g]:lp[g + 1]]) and np.array_equal(f[lpb[r]:lpb[r + 1]], first[1][lp[g]:lp[g + 1]])
        assert np.array_equal(k[bpb[lpb[r]]:bpb[lpb[r + 1]]], first[2][bp[lp[g]]:bp[lp[g + 1]]]), g


# ---- the seeded sets -------------------------------------------------------------------------------------------------------------------------
def test_a_thousand_molecule_like_graphs_and_two_hundred_randomly_aromatic_ones():
    for args, want in seeded_model():
        assert (want[3][:, 21] == 0).all()
        same(run(*args), want)


# ---- wave and limit boundaries ---------------------------------------------------------------------------------------------------------------
def benzene_with_pendants(n):
    """an aromatic hexagon and a chain of n - 6 carbons on it, every fifth of them a nitrogen: n atoms, n bonds"""
    return graph([6] * 6 + [7 if a % 5 == 0 else 6 for a in range(6, n)], ring(6), plain=[(a - 1 if a > 6 else 0, a) for a in range(6, n)])


def polyhex(rows, cols, pendants=0, seed=None):
    """rows x cols fused hexagons, every bond aromatic, every atom a carbon, and ``pendants`` more carbons on aromatic bonds of their
    own at atoms with two ring bonds; ``seed``: a relabelling"""
    g = nx.hexagonal_lattice_graph(rows, cols)
    index = {v: i for i, v in enumerate(sorted(g.nodes()))}
    edges = [(index[a], index[b]) for a, b in g.edges()]
    n = len(index)
    outer = [a for a in range(n) if sum(a in e for e in edges) == 2]
    for t in range(pendants):
        edges.append((outer[3 * t], n + t))
    case = graph([6] * (n + pendants), edges)
    if seed is None:
        return case
    perm = list(range(n + pendants))
    random.Random(seed).shuffle(perm)
    return relabel(case, perm)


def model_steps(case):
    try:
        return VM.graph_valence(*case)[4]
    except VM.SearchLimit:
        return None


def cheapest(make, seeds=range(12)):
    """the labelling (None: as built; else a seeded shuffle) whose model step count is smallest: the limit tests want a search inside the
    budget whatever the order of the list costs"""
    found = [(steps[0], k) for k, steps in ((k, model_steps(make(k))) for k in [None] + list(seeds)) if steps]
    assert found
    return make(min(found, key=lambda t: t[0])[1])


def test_wave_boundaries():
    cases = [benzene_with_pendants(n) for n in (63, 64, 65, 127, 128, 129, 256, 257)]
    want = check(cases)
    assert want[3][:, 0].tolist() == [63, 64, 65, 127, 128, 129, 256, 257]
    assert want[3][:, 21].tolist() == [0] * 7 + [VM.TOO_MANY_ATOMS] and want[3][6, 3] == 1 and want[3][6, 19] == 1
    assert want[3][7].tolist() == [257, 257] + [-1] * 19 + [1]
    # 130 systems cannot be (a system has two atoms): 128 aromatic pairs in one graph, two per lane
    pairs = graph([6, 7] * 128, [(2 * t, 2 * t + 1) for t in range(128)])
    want = check([pairs, pairs])
    assert want[3][0, 3] == 128 and want[3][0, 5] == 128 and want[3][0, 20] == 2 and want[3][0, 21] == 0


def test_eligible_bond_and_atom_limits():
    p63, p64 = (cheapest(lambda s, t=t: polyhex(4, 4, t, s)) for t in (0, 1))
    p65 = polyhex(4, 4, 2)
    path64, path65 = graph([6] * 64, [(a, a + 1) for a in range(63)]), graph([6] * 65, [(a, a + 1) for a in range(64)])
    cases = [p63, p64, p65, path64, path65, HAND["benzene"][0]]
    want = check(cases)
    assert want[3][:, 1].tolist() == [63, 64, 65, 63, 64, 6]
    assert want[3][:, 21].tolist() == [0, 0, VM.SEARCH_LIMIT, 0, VM.SEARCH_LIMIT, 0]
    assert want[3][0, 5] == 24 and want[3][0, 19] == 1 and want[3][1, 4] + want[3][1, 5] > 0 and want[3][3, 5] == 32
    lp, bp = collate(cases)[1], collate(cases)[3]
    for g in (2, 4):
        assert want[3][g, 2:21].tolist() == [-1] * 19 and (want[0][lp[g]:lp[g + 1]] == 255).all()
        assert (want[1][lp[g]:lp[g + 1]] == 255).all() and (want[2][bp[lp[g]]:bp[lp[g + 1]]] == 255).all()


def test_step_budget_is_exact():
    benzene = HAND["benzene"][0]
    big = cheapest(lambda s: polyhex(3, 4, 0, s))                    # 12 fused hexagons, 38 atoms, 49 bonds
    steps = model_steps(big)[0]
    assert 49 < steps <= VM.MAX_STEPS
    for case, need in ((benzene, 8), (big, steps)):
        inside, outside = check([case, benzene], need), check([benzene, case, benzene], need - 1)
        assert inside[3][:, 21].tolist() == [0, 0] and inside[3][0, 20] == need
        assert outside[3][1].tolist() == [case[0], len(case[1])] + [-1] * 19 + [VM.SEARCH_LIMIT]
        assert (outside[2][6:6 + len(case[1])] == 255).all()
        if need - 1 >= 8:
            assert outside[3][[0, 2], 21].tolist() == [0, 0]
    want = check([benzene], 1)
    assert want[3][0, 21] == VM.SEARCH_LIMIT
    # a must atom without an eligible bond fails in one step, inside any budget: toluene-like carbon between two oxygens
    lonely = graph([8, 6, 8, 6, 6], ring(5))
    want = check([lonely], 1)
    assert want[3][0, 21] == 0 and want[3][0, 20] == 1 and want[3][0, 4] == 1 and want[2].tolist() == [4] * 5


# ---- small batches, missing arrays, a graph the aromatic report gave up ----------------------------------------------------------------------
def test_small_batches_null_aromatic_and_no_bonds():
    benzene, pyrrole, empty = HAND["benzene"][0], HAND["pyrrole"][0], HAND["empty"][0]
    check([benzene])
    check([empty])
    check([benzene, empty])
    check([benzene, empty, pyrrole])
    check([empty, empty])
    args = collate([benzene, empty, pyrrole, HAND["pyridone"][0]])
    want = VM.batch_valence(*args[:6], None)
    assert want[3][:, 3].tolist() == [0] * 4 and want[3][:, 21].tolist() == [0] * 4 and want[2].tolist() == args[5].tolist()
    same(run(*args[:6], None), want)
    atoms = collate([graph([6, 7, 8, 1, 9], []), empty, graph([5, 16], [])])
    assert atoms[4].shape == (2, 0)
    want = VM.batch_valence(*atoms)
    assert want[0].tolist() == [4, 3, 2, 1, 1, 0, 2] and want[3][:, 2].tolist() == [5, 0, 2] and want[3][:, 8].tolist() == [0, 0, 1]
    same(run(*atoms), want)
    same(run(*atoms[:6], None), want)


def test_not_evaluated_aromatic_bytes_stop_their_graph_only():
    args = list(collate([HAND["benzene"][0], HAND["naphthalene"][0], HAND["pyrrole"][0]]))
    args[6] = args[6].copy()
    args[6][6 + 4] = 255
    want = VM.batch_valence(*args)
    assert want[3][:, 21].tolist() == [0, VM.NO_AROMATIC, 0] and want[3][1].tolist() == [10, 11] + [-1] * 19 + [8]
    assert (want[2][6:17] == 255).all() and (want[0][6:16] == 255).all() and want[2][:6].tolist() == [2, 1, 1, 2, 1, 2]
    same(run(*args), want)


# ---- malformed input stays inside the buffers ----------------------------------------------------------------------------------------------
def test_malformed_lists_are_reported_and_clamped():
    """naphthalene | pyridone with a broken list | biphenyl, the breakages of tests/test_gpu_aromatic.py and two orders outside 1..3: the
    broken graph carries BAD_BONDS, -1 and 255, its neighbours their clean results, and the guard tails stay 0xFF (checked in ``run``)"""
    cases = [HAND["naphthalene"][0], HAND["pyridone"][0], HAND["biphenyl"][0]]
    z, lig_ptr, n_lig, bond_ptr, idx, order, aro = collate(cases)
    clean = run(z, lig_ptr, n_lig, bond_ptr, idx, order, aro)
    same(clean, VM.batch_valence(z, lig_ptr, n_lig, bond_ptr, idx, order, aro))
    assert clean[3][:, 21].tolist() == [0, 0, 0]
    b0, b1 = int(bond_ptr[lig_ptr[1]]), int(bond_ptr[lig_ptr[2]])
    a0 = int(lig_ptr[1])

    def swap(bp, bi, bo):             # a bond with j <= i
        bi[:, b0 + 2] = bi[::-1, b0 + 2].copy()

    def equal(bp, bi, bo):
        bi[1, b0 + 1] = bi[0, b0 + 1]

    def leaves(bp, bi, bo):           # a bond that leaves the graph's atom range: into the next graph
        bi[1, b1 - 1] = lig_ptr[2] + 1

    def wild(bp, bi, bo):             # rows no array has
        bi[0, b0] = -7
        bi[1, b0 + 3] = 2 ** 31 - 1
        bi[1, b0 + 4] = n_lig + 1000

    def out_of_order(bp, bi, bo):     # two bonds exchanged
        bi[:, [b0, b0 + 1]] = bi[:, [b0 + 1, b0]]

    def pointer(bp, bi, bo):          # non-monotone inside the graph; the graph's own range is what it was
        bp[a0 + 2] = bp[a0 + 3] + 2

    def order_zero(bp, bi, bo):
        bo[b0 + 5] = 0

    def order_four(bp, bi, bo):
        bo[b1 - 1] = 4

    def everything(bp, bi, bo):
        swap(bp, bi, bo), leaves(bp, bi, bo), pointer(bp, bi, bo), order_zero(bp, bi, bo)

    for what in (swap, equal, leaves, wild, out_of_order, pointer, order_zero, order_four, everything):
        bp, bi, bo = bond_ptr.copy(), idx.copy(), order.copy()
        what(bp, bi, bo)
        want = VM.batch_valence(z, lig_ptr, n_lig, bp, bi, bo, aro)
        assert want[3][:, 21].tolist() == [0, VM.BAD_BONDS, 0], what.__name__
        got = run(z, lig_ptr, n_lig, bp, bi, bo, aro)
        same(got, want)
        assert got[3][1].tolist() == [7, 7] + [-1] * 19 + [VM.BAD_BONDS]
        assert (got[0][lig_ptr[1]:lig_ptr[2]] == 255).all() and (got[1][lig_ptr[1]:lig_ptr[2]] == 255).all() and (got[2][b0:b1] == 255).all()
        for g in (0, 2):
            lo, hi = bond_ptr[lig_ptr[g]], bond_ptr[lig_ptr[g + 1]]
            assert np.array_equal(got[3][g], clean[3][g]) and np.array_equal(got[2][lo:hi], clean[2][lo:hi]), (what.__name__, g)
            for k in (0, 1):
                assert np.array_equal(got[k][lig_ptr[g]:lig_ptr[g + 1]], clean[k][lig_ptr[g]:lig_ptr[g + 1]]), (what.__name__, g)
    # pointers outside the list at a graph boundary and a lig_ptr outside the atoms: ranges are clamped as the model clamps them
    bp = bond_ptr.copy()
    bp[lig_ptr[2]] = len(idx[0]) + 500
    bp[lig_ptr[1]] = -3
    want = VM.batch_valence(z, lig_ptr, n_lig, bp, idx, order, aro)
    assert (want[3][:, 21] == VM.BAD_BONDS).all()
    same(run(z, lig_ptr, n_lig, bp, idx, order, aro), want)
    lp = lig_ptr.copy()
    lp[0], lp[3] = -4, n_lig + 77
    same(run(z, lp, n_lig, bond_ptr, idx, order, aro), clean)


# ---- from coordinates, the Python entries ----------------------------------------------------------------------------------------------------
def test_from_coordinates_through_bonds_rings_aromatic_and_valence():
    """graph 0: biphenyl, two planar C6 hexagons at 1.40 A joined by a 1.48 A bond, aromatic carbon types; graph 1: 2-pyridone, a hexagon
    N0 C1 ... C5 at 1.40 A of aromatic types with an oxygen 1.22 A off C1; graph 2: a lone aromatic-typed carbon and an oxygen far away"""
    ang = np.arange(6) * np.pi / 3
    hexagon = np.stack([1.40 * np.cos(ang), 1.40 * np.sin(ang), 0 * ang], 1)
    second = hexagon * [-1, 1, 1] + [1.40 + 1.48 + 1.40, 0, 0]
    pyridone = np.concatenate([hexagon, hexagon[1:2] * (1.40 + 1.22) / 1.40]) + [0, 40.0, 0]
    apart = np.array([[0, 80.0, 0], [9.0, 80.0, 0]])
    x = torch.from_numpy(np.concatenate([hexagon, second, pyridone, apart]).astype(np.float32)).to(DEV)
    c = torch.tensor([2] * 12 + [4, 2, 2, 2, 2, 2, 5] + [2, 5], dtype=torch.long, device=DEV)    # add_aromatic: 2 = aromatic C, 4 = aromatic N, 5 = O
    lig_b = torch.tensor([0] * 12 + [1] * 7 + [2] * 2, device=DEV)
    batch = {"num_graphs": 3}
    bonds = G.batch_bonds(batch, x, c, lig_b, "add_aromatic")
    assert bonds["graph_counts"][:, 1].tolist() == [13, 7, 0]
    pyridone_orders = bonds["bond_order"][13:].tolist()
    assert pyridone_orders == [1, 1, 1, 2, 1, 1, 1]
    rings = G.batch_rings(batch, x, c, lig_b, "add_aromatic", bonds=bonds)
    aro = G.batch_aromatic(batch, x, c, lig_b, "add_aromatic", bonds=bonds, rings=rings)
    assert aro["bond_type"].tolist().count(4) == 18
    out = G.batch_valence(batch, x, c, lig_b, "add_aromatic", bonds=bonds, aromatic=aro)
    assert sorted(out) == ["atom_flags", "bond_kekule", "graph_counts", "implicit_h"]
    assert all(v.device.type == "cuda" for v in out.values())
    assert [out[k].dtype for k in sorted(out)] == [torch.uint8, torch.uint8, torch.int32, torch.uint8]
    assert out["bond_kekule"].tolist() == HAND["biphenyl"][1] + HAND["pyridone"][1]
    assert out["implicit_h"].tolist() == HAND["biphenyl"][2] + HAND["pyridone"][2] + [4, 2]
    assert out["atom_flags"].tolist() == [8] * 12 + [8] * 6 + [0] + [0, 0]
    gc = out["graph_counts"]
    assert torch.equal(gc[:, 2], bonds["graph_counts"][:, 3]) and gc[:, 2].tolist() == [1, 1, 2]           # n_fragments is the bond report's
    assert gc[:, 19].tolist() == [1, 1, 1] and gc[:, 21].tolist() == [0, 0, 0] and gc[:, 3].tolist() == [2, 1, 0]
    rows = gc.cpu().numpy()
    assert [G.formula(r[11:19], r[6]) for r in rows] == ["C12H10", "C5H5NO", "CH6O"]
    assert G.summarise_valence(rows)["valid_mol_ratio"] == 2 / 3 and G.summarise_valence(rows)["valence_ok_mol_ratio"] == 1.0
    # against the model on the list the device made
    z = torch.tensor(C.config._ATOMIC_NUMBER["add_aromatic"], device=DEV)[c]
    lig_ptr = np.array([0, 12, 19, 21])
    bond_ptr = np.concatenate([[0], np.cumsum(np.bincount(bonds["bond_index"][0].cpu().numpy(), minlength=21))])
    want = VM.batch_valence(z.cpu().numpy(), lig_ptr, 21, bond_ptr, bonds["bond_index"].cpu().numpy(), bonds["bond_order"].cpu().numpy(),
                            aro["aromatic_bond"].cpu().numpy().astype(np.uint8))
    same(tuple(out[k].cpu().numpy() for k in ("implicit_h", "atom_flags", "bond_kekule", "graph_counts")), want)
    # computed here when not given; without aromatic flags ('basic' types: 1 = C, 2 = N, 3 = O) no bond is aromatic
    again = G.batch_valence(batch, x, c, lig_b, "add_aromatic")
    direct = G.ligand_valence(z, lig_b, 3, bonds, aro)
    for k in out:
        assert torch.equal(again[k], out[k]) and torch.equal(direct[k], out[k]), k
    cb = torch.tensor([1] * 12 + [2, 1, 1, 1, 1, 1, 3] + [1, 3], dtype=torch.long, device=DEV)
    basic = G.batch_valence(batch, x, cb, lig_b, "basic")
    assert basic["graph_counts"][:, 3].tolist() == [0, 0, 0] and torch.equal(basic["bond_kekule"], bonds["bond_order"])
    assert torch.equal(basic["bond_kekule"], G.ligand_valence(z, lig_b, 3, bonds)["bond_kekule"])
    assert basic["implicit_h"].tolist() == [1] + [2] * 5 + [1] + [2] * 5 + [1, 0, 2, 2, 2, 2, 0] + [4, 2]
    # a graph the aromatic report did not evaluate; a budget of ten steps: benzene rings fit, nothing else changes
    gave_up = dict(aro, bond_type=torch.where(bonds["bond_graph"] == 1, 255, aro["bond_type"].to(torch.long)).to(torch.uint8))
    out2 = G.ligand_valence(z, lig_b, 3, bonds, gave_up)
    assert out2["graph_counts"][:, 21].tolist() == [0, G.VALENCE_NO_AROMATIC, 0] and out2["bond_kekule"][13:].tolist() == [255] * 7
    assert torch.equal(out2["graph_counts"][[0, 2]], gc[[0, 2]])
    out3 = G.ligand_valence(z, lig_b, 3, bonds, aro, max_steps=7)
    assert out3["graph_counts"][:, 21].tolist() == [G.VALENCE_SEARCH_LIMIT] * 2 + [0]
    with pytest.raises(ValueError, match="max_steps"):
        G.ligand_valence(z, lig_b, 3, bonds, aro, max_steps=0)
    empty = G.ligand_valence(z[:0], lig_b[:0], 2, {"bond_index": bonds["bond_index"][:, :0], "bond_order": bonds["bond_order"][:0]})
    assert empty["graph_counts"].tolist() == [[0] * 22] * 2 and empty["bond_kekule"].shape == (0,)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
VALENCE_FIELDS = ("implicit_h", "valence_flags", "bond_kekule", "formula", "mol_weight", "n_nhoh", "n_no", "valence_ok", "mol_valid",
                  "valence_status")


def _records(out_dir, n):
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".pt"))
    assert files == [f"pocket_{i:05d}.pt" for i in range(n)]
    return [torch.load(os.path.join(out_dir, f), map_location="cpu", weights_only=False) for f in files]


def _same_field(a, b):
    return _equal(a, b) or (torch.is_tensor(a) and a.is_floating_point() and torch.equal(a.isnan(), b.isnan())
                            and torch.equal(a.nan_to_num(), b.nan_to_num())) or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


def test_sample_cli_valence(tmp_path, capsys):
    """the T = 20 fixture config, three synthetic pockets x two samples, --noise counter, one saved random checkpoint (see the issue's list
    in the assertions below)"""
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    config, _ = C.load_config(cfg)
    C.set_num_atom_type(config)
    torch.manual_seed(123)
    ckpt = tmp_path / "random_init.pt"
    torch.save({"model": C.get_model(config.model).state_dict()}, ckpt)
    tail = ["--synthetic", "3", "--num_samples", "2", "--seed", "2024", "--noise", "counter", "--no_translate"]

    def go(tag, *extra, config_path=cfg, weights=("--checkpoint", str(ckpt))):
        out, stats = tmp_path / tag, {}
        assert sample_cli.main(["--config", config_path, *weights, *tail, "--out_root", str(out)] + list(extra), stats=stats) == 0
        d = str(out / os.path.splitext(os.path.basename(config_path))[0])
        return d, _records(d, 3), stats

    def text(d, name):
        with open(os.path.join(d, name)) as f:
            return f.read()

    whole = ("--pockets_per_batch", "3", "--streams", "1")
    dir_base, base, stats_base = go("base", *whole)
    dir_val, alone, stats_val = go("val", *whole, "--valence")
    dir_aro, aro, _ = go("aro", *whole, "--aromatic", "--bonds", "--sdf")
    dir_all, both, stats_all = go("all", *whole, "--valence", "--aromatic", "--bonds", "--sdf")
    _, split, _ = go("split", "--pockets_per_batch", "1", "--streams", "1", "--valence")
    printed = capsys.readouterr().out
    assert printed.count("valence: valence_ok_mol_ratio") == 3 and "sdf: 6 records written, 0 samples left out" in printed
    assert stats_val["valence"] > 0.0 and stats_all["valence"] > 0.0 and "valence" not in stats_base
    assert not {"bonds", "rings", "aromatic"} & set(stats_val)

    # without the flag nothing of it is written, and what is written does not change with it: field by field outside the new keys
    assert not os.path.exists(os.path.join(dir_base, "valence_summary.json")) and not os.path.exists(os.path.join(dir_aro, "valence_summary.json"))
    assert sorted(os.listdir(dir_val)) == sorted(os.listdir(dir_base) + ["valence_summary.json"])
    assert sorted(os.listdir(dir_all)) == sorted(os.listdir(dir_aro) + ["valence_summary.json"])
    for name in ("aromatic_summary.json", "bonds_summary.json"):
        assert text(dir_all, name) == text(dir_aro, name)
    for without, with_it in ((base, alone), (aro, both)):
        for r, r2 in zip(without, with_it):
            assert sorted(set(r2) - set(r)) == ["valence"] and all(_same_field(r[k], r2[k]) for k in r if k != "samples")
            for s, s2 in zip(r["samples"], r2["samples"]):
                assert sorted(set(s2) - set(s)) == sorted(VALENCE_FIELDS)
                assert all(_same_field(s[k], s2[k]) for k in s), [k for k in s if not _same_field(s[k], s2[k])]

    # the new fields against the model on the graph the file holds; alone, with the other flags, and in a 1-pocket batch they are the same
    rows = []
    for rb, ra, rs in zip(both, alone, split):
        assert rb["valence"] == ra["valence"] == rs["valence"] and rb["pocket_index"] == ra["pocket_index"] == rs["pocket_index"]
        mine = []
        for sb, sa, ss in zip(rb["samples"], ra["samples"], rs["samples"]):
            for k in VALENCE_FIELDS:
                assert _same_field(sb[k], sa[k]) and _same_field(sb[k], ss[k]), k
            n = len(sb["atom"])
            idx = sb["bond_index"].numpy()
            bond_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx[0], minlength=n))])
            aromatic = np.where(sb["bond_type"].numpy() == 255, 255, sb["aromatic_bond"].numpy().astype(np.uint8))
            h, f, k, row = VM.batch_valence(sb["atom"], [0, n], n, bond_ptr, idx, sb["bond_order"].numpy(), aromatic)
            assert sb["implicit_h"].dtype == sb["valence_flags"].dtype == sb["bond_kekule"].dtype == torch.uint8
            assert sb["implicit_h"].tolist() == h.tolist() and sb["valence_flags"].tolist() == f.tolist() and sb["bond_kekule"].tolist() == k.tolist()
            col = dict(zip(VM.COLUMNS, row[0].tolist()))
            assert sb["valence_status"] == col["status"] and (sb["n_nhoh"], sb["n_no"]) == (col["n_nhoh"], col["n_no"])
            assert sb["valence_ok"] == (col["status"] == 0 and col["valence_ok"] == 1)
            assert sb["mol_valid"] == (sb["valence_ok"] and sb["n_fragments"] == 1) and isinstance(sb["mol_valid"], bool)
            if col["status"] == 0:
                el = [col[f"el_{c}"] for c in range(8)]
                assert sb["formula"] == G.formula(el, col["n_implicit_h"]) and sb["mol_weight"] == G.mol_weight(el, col["n_implicit_h"])
                assert col["n_fragments"] == sb["n_fragments"]
            mine.append(row[0])
        assert rb["valence"] == G.summarise_valence(np.stack(mine))["counts"]
        rows += mine
    want = G.summarise_valence(np.stack(rows))
    for d in (dir_val, dir_all):
        summary = json.loads(text(d, "valence_summary.json"))
        assert summary["counts"] == want["counts"] and set(summary) == set(G.VALENCE_RATIOS) | {"element_distribution", "counts"}
        for k in G.VALENCE_RATIOS + ("element_distribution",):
            assert summary[k] == want[k] or np.isnan(summary[k]), k
    assert want["counts"]["n_mol"] == 6

    # --sdf: with --valence an evaluated sample carries bond_kekule (no type 4 but on a failed system); without it the file is what it was
    for rec, rec_aro in zip(both, aro):
        name = f"pocket_{rec['pocket_index']:05d}.sdf"
        parsed, before = read_sdf(text(dir_all, name)), read_sdf(text(dir_aro, name))
        assert len(parsed) == len(before) == 2
        for (_, _, _, sdf_bonds), (_, _, _, old_bonds), smp, smp_aro in zip(parsed, before, rec["samples"], rec_aro["samples"]):
            evaluated = smp["valence_status"] == 0
            old_types = smp_aro["bond_type"] if smp_aro["aromatic_status"] == 0 else smp_aro["bond_order"]
            types = smp["bond_kekule"] if evaluated else old_types
            assert sdf_bonds == [(i, j, t) for i, j, t in zip(*smp["bond_index"].tolist(), types.tolist())]
            assert old_bonds == [(i, j, t) for i, j, t in zip(*smp_aro["bond_index"].tolist(), old_types.tolist())]
            if evaluated:
                failed = {b for b, t in enumerate(smp["bond_kekule"].tolist()) if t == 4}
                assert all((t == 4) == (b in failed) for b, (_, _, t) in enumerate(sdf_bonds))
                assert all(smp["valence_flags"][i] & 2 and smp["valence_flags"][j] & 2 for b, (i, j, _) in enumerate(sdf_bonds) if b in failed)

    # the 8-type vocabulary: no aromatic flags, the report runs on the bond list alone
    basic = tmp_path / "targetdiff_T20_basic.yml"
    source = open(cfg).read()
    assert source.count("mode: add_aromatic") == 1
    basic.write_text(source.replace("mode: add_aromatic", "mode: basic").replace("!include common/",
                                                                               "!include " + os.path.join(ROOT, "tests", "fixtures", "common") + "/"))
    dir_basic, recs, stats_basic = go("basic", *whole, "--valence", "--bonds", "--sdf", config_path=str(basic), weights=("--random_init",))
    assert os.path.exists(os.path.join(dir_basic, "valence_summary.json")) and stats_basic["valence"] > 0.0
    for rec in recs:
        assert set(rec["valence"]) == set(G.VALENCE_COUNT_KEYS) and rec["valence"]["n_systems"] == 0
        parsed = read_sdf(text(dir_basic, f"pocket_{rec['pocket_index']:05d}.sdf"))
        for (_, _, _, sdf_bonds), smp in zip(parsed, rec["samples"]):
            assert set(VALENCE_FIELDS) <= set(smp) and "aromatic_bond" not in smp
            assert _equal(smp["bond_kekule"], smp["bond_order"]) and not (smp["valence_flags"] & 10).any()
            assert sdf_bonds == [(i, j, t) for i, j, t in zip(*smp["bond_index"].tolist(), smp["bond_kekule"].tolist())]
