"""Functional groups on the GPU (csrc/groups.hip: cbgx_ligand_groups; cbgbench_amd/geometry.py; sample_cli --groups) against the
plain-Python model of tests/groups_model.py.  Every comparison is ``==``: the results are integers.  Output buffers handed to the entry are
pre-filled with 0xFF bytes and carry a 0xFF guard tail inside the same allocation, which must stay as it is."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, geometry as G
from tests import groups_model as GM
from tests.test_gpu_rings import DEV, GUARD, _dev, _equal, _ff, same
from tests.test_groups import HAND_CASES, NEAR, POSITIVE, mol, seeded_model
from tests.test_valence import collate, graph, relabel, ring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(z, lig_ptr, n_lig, bond_ptr, bond_index, bond_order, bond_aromatic=None):
    """the entry on 0xFF outputs with guard tails -> (atom_group [n_lig], atom_class [n_lig], graph_out [B, 33]); the guards are checked
    here"""
    lp, bp, bi = _dev(lig_ptr, np.int32), _dev(bond_ptr, np.int32), _dev(np.asarray(bond_index, np.int32).reshape(2, -1), np.int32)
    zz, bo = _dev(z, np.uint8), _dev(bond_order, np.uint8)
    ba = None if bond_aromatic is None else _dev(bond_aromatic, np.uint8)
    B, nb = lp.shape[0] - 1, bi.shape[1]
    grp, cls, gc = _ff(n_lig + GUARD, torch.int32), _ff(n_lig + GUARD, torch.uint8), _ff(B * GM.COLS + GUARD, torch.int32)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_groups(p(zz), p(lp), n_lig, B, p(bp), p(bi) if nb else None, p(bo) if nb else None,
                                                   p(ba) if ba is not None and nb else None, nb, p(grp), p(cls), p(gc),
                                                   _native.current_stream(DEV)), "cbgx_ligand_groups")
    torch.cuda.synchronize()
    grp, cls, gc = grp.cpu().numpy(), cls.cpu().numpy(), gc.cpu().numpy()
    assert (grp[n_lig:] == -1).all() and (cls[n_lig:] == 255).all() and (gc[B * GM.COLS:] == -1).all()
    return grp[:n_lig], cls[:n_lig], gc[:B * GM.COLS].reshape(B, GM.COLS)


def check(cases):
    """kernel == model on one batch of cases -> the model's outputs"""
    args = collate(cases)
    want = GM.batch_groups(*args)
    same(run(*args), want)
    return want


# ---- the hand cases --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    cases = list(HAND_CASES)
    args = collate(cases)
    return cases, args, GM.batch_groups(*args)


def test_hand_cases_in_one_batch(hand):
    cases, args, want = hand
    for k in range(GM.CLASSES):
        assert want[2][k, 6 + k] == 1 and want[2][k, 2] == 1, POSITIVE[k]
    for g, (name, (_, names, sizes)) in enumerate(NEAR.items(), GM.CLASSES):
        assert want[2][g, 2] == len(names) and want[2][g, 31] == names.count("other") and want[2][g, 5] == max(sizes), name
    assert (want[2][:, -1] == 0).all()
    same(run(*args), want)


def test_each_graph_alone_twice_and_reversed(hand):
    cases, args, want = hand
    first, second = run(*args), run(*args)
    same(first, want)
    same(second, first)
    lp = args[1]
    for g, case in enumerate(cases):
        grp, cls, gc = run(*collate([case]))
        assert np.array_equal(gc[0], first[2][g]) and np.array_equal(grp, first[0][lp[g]:lp[g + 1]]), g
        assert np.array_equal(cls, first[1][lp[g]:lp[g + 1]]), g
    back = collate(cases[::-1])
    grp, cls, gc = run(*back)
    assert np.array_equal(gc[::-1], first[2])
    lpb = back[1]
    for g in range(len(cases)):
        r = len(cases) - 1 - g
        assert np.array_equal(grp[lpb[r]:lpb[r + 1]], first[0][lp[g]:lp[g + 1]]) and np.array_equal(cls[lpb[r]:lpb[r + 1]], first[1][lp[g]:lp[g + 1]]), g


def test_the_seeded_set():
    args, want, _ = seeded_model()
    assert (want[2][:, -1] == 0).all()
    same(run(*args), want)


def test_placement_in_a_batch_of_65(hand):
    cases, _, _ = hand
    probes = [mol("Oc1ccccc1CC(=O)NC", seed=1), mol(POSITIVE[4], seed=2), mol(NEAR["azulene"][0], seed=3)]
    alone = [run(*collate([p])) for p in probes]
    for slot in (0, 1, 63, 64):
        batch = [cases[(7 * k) % len(cases)] for k in range(65)]
        for k, p in enumerate(probes):
            batch[(slot + 20 * k) % 65] = p
        args = collate(batch)
        got = run(*args)
        same(got, GM.batch_groups(*args))
        lp = args[1]
        for k, (grp, cls, gc) in enumerate(alone):
            g = (slot + 20 * k) % 65
            assert np.array_equal(got[2][g], gc[0]) and np.array_equal(got[0][lp[g]:lp[g + 1]], grp) and np.array_equal(got[1][lp[g]:lp[g + 1]], cls)


# ---- sizes: atoms, groups, lanes -----------------------------------------------------------------------------------------------------------
def ring_with_a_tail(n):
    """an aromatic hexagon (a pyridine) and a chain of n - 6 atoms on it, every third of them a nitrogen, every seventh an oxygen with a
    double bond to the chain: n atoms, n bonds, many small groups"""
    z = [7] + [6] * 5 + [7 if a % 3 == 0 else 8 if a % 7 == 0 else 6 for a in range(6, n)]
    chain = [(a - 1 if a > 6 else 0, a) for a in range(6, n)]
    double = [e for e in chain if z[e[1]] == 8]
    return graph(z, ring(6), double=double, plain=[e for e in chain if e not in double])


def test_atom_limit_and_wave_boundaries():
    cases = [graph([], []), graph([8], []), graph([6], [])] + [ring_with_a_tail(n) for n in (63, 64, 65, 128, 129, 255, 256, 257)]
    want = check(cases)
    assert want[2][:, 0].tolist() == [0, 1, 1, 63, 64, 65, 128, 129, 255, 256, 257]
    assert want[2][:, -1].tolist() == [0] * 10 + [GM.TOO_MANY_ATOMS] and want[2][10].tolist() == [257, 257] + [-1] * 30 + [1]
    assert want[2][0].tolist() == [0] * 33 and want[2][1].tolist() == [1, 0, 1, 1, 0, 1] + [0] * 25 + [1, 0] and want[2][2, 2] == 0
    assert want[2][9, 6 + 3] == 1 and want[2][9, 2] > 64                 # the pyridine ring, and more groups than lanes
    assert (want[0][-257:] == -2).all() and (want[1][-257:] == 255).all()
    shuffled = [relabel(c, random.Random(k).sample(range(c[0]), c[0])) for k, c in enumerate(cases[3:10])]
    check(shuffled)


def test_more_groups_than_lanes():
    oxygens = graph([8] * 256, [])
    want = check([oxygens, graph([8] * 65, []), oxygens])
    assert want[2][0].tolist() == [256, 0, 256, 256, 0, 1] + [0] * 25 + [256, 0] and want[2][1, 2] == 65
    assert want[0][:256].tolist() == list(range(256)) and (want[1] == GM.OTHER).all()
    # 85 nitro groups and one oxygen: more named groups than lanes, every one through the isomorphism test
    z, double = [8], []
    for k in range(85):
        o = 1 + 3 * k
        z += [7, 8, 8]
        double += [(o, o + 1), (o, o + 2)]
    many = graph(z, [], double=double)
    want = check([many, relabel(many, random.Random(4).sample(range(256), 256))])
    assert want[2][:, 2].tolist() == [86, 86] and want[2][:, 6 + 20].tolist() == [85, 85] and want[2][:, 31].tolist() == [1, 1]


def test_groups_of_ten_and_eleven_atoms():
    ten = [mol(POSITIVE[11], seed=5), mol(POSITIVE[16], seed=6), mol(NEAR["azulene"][0], seed=7), mol(NEAR["decapentaene"][0], seed=8),
           mol(NEAR["isoquinoline"][0], seed=9)]
    eleven = [mol(NEAR["chain_of_11"][0], seed=10), mol("Cc1ccc2ccccc2c1=O", seed=11), mol("c1ccc2cc3ccccc3cc2c1", seed=12)]
    want = check(ten + eleven)
    assert want[2][:, 5].tolist() == [10] * 5 + [11, 11, 14]
    assert [int(np.argmax(row[6:32])) for row in want[2]] == [11, 16, 25, 25, 25, 25, 25, 25] and (want[2][:, 2] == 1).all()


def collapsed(n, seed, aromatic_share=0.0):
    """every pair of n atoms bonded: what a collapsed sample of random weights looks like to the bond table"""
    rng = random.Random(seed)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    z = [rng.choice((6, 6, 6, 7, 8, 16, 9, 1)) for _ in range(n)]
    return n, pairs, z, [rng.choice((1, 1, 2, 3)) for _ in pairs], [int(rng.random() < aromatic_share) for _ in pairs]


def test_collapsed_graphs():
    cases = [collapsed(40, 1), collapsed(40, 2, 0.3), collapsed(40, 3, 1.0), collapsed(12, 4), collapsed(5, 5, 0.5)]
    singles = list(collapsed(40, 6))
    singles[3] = [1] * len(singles[1])                         # all single bonds: triangles everywhere, acetal carbons
    want = check(cases + [tuple(singles)])
    assert want[2][:, 1].tolist() == [780, 780, 780, 66, 10, 780] and (want[2][:, -1] == 0).all()
    assert (want[2][:, 5] > 10).sum() >= 4


# ---- missing arrays, a graph the aromatic report gave up, a bad order ----------------------------------------------------------------------
def test_null_aromatic_no_bonds_and_small_batches(hand):
    cases, args, _ = hand
    benzene, empty = mol("Cc1ccccc1"), graph([], [])
    for batch in ([benzene], [empty], [benzene, empty], [empty, empty], [empty, benzene, empty]):
        check(batch)
    want = GM.batch_groups(*args[:6], None)
    assert want[2][0, 2] == 0 and want[2][1].tolist() == check([cases[1]])[2][0].tolist()        # toluene: no members; the amide as it was
    same(run(*args[:6], None), want)
    atoms = collate([graph([6, 7, 8, 1, 9], []), empty, graph([5, 16], [])])
    assert atoms[4].shape == (2, 0)
    want = GM.batch_groups(*atoms)
    assert want[0].tolist() == [-1, 1, 2, -1, 4, -1, 1] and want[1].tolist() == [254, 25, 25, 254, 25, 254, 25]
    same(run(*atoms), want)
    same(run(*atoms[:6], None), want)


def test_not_evaluated_aromatic_bytes_and_bad_orders_stop_their_graph_only():
    cases = [mol("Cc1ccccc1"), mol("Cc1ccc2ccccc2c1"), mol("CC(=O)NC")]
    clean = check(cases)
    args = list(collate(cases))
    args[6] = args[6].copy()
    args[6][7 + 4] = 255
    want = GM.batch_groups(*args)
    assert want[2][:, -1].tolist() == [0, GM.NO_AROMATIC, 0] and want[2][1].tolist() == [11, 12] + [-1] * 30 + [8]
    assert (want[0][7:18] == -2).all() and (want[1][7:18] == 255).all()
    same(run(*args), want)
    for value, where in ((0, 7 + 2), (4, 7 + 11), (255, 0)):
        args = list(collate(cases))
        args[5] = args[5].copy()
        args[5][where] = value
        want = GM.batch_groups(*args)
        bad = 0 if where == 0 else 1
        assert want[2][:, -1].tolist() == [GM.BAD_BONDS if g == bad else 0 for g in range(3)]
        got = run(*args)
        same(got, want)
        for g in range(3):
            if g != bad:
                assert np.array_equal(got[2][g], clean[2][g])
    both = list(collate(cases))
    both[5], both[6] = both[5].copy(), both[6].copy()
    both[5][7 + 1], both[6][7 + 3] = 0, 255
    want = GM.batch_groups(*both)
    assert want[2][1, -1] == GM.BAD_BONDS | GM.NO_AROMATIC
    same(run(*both), want)


# ---- malformed input stays inside the buffers ----------------------------------------------------------------------------------------------
def test_malformed_lists_are_reported_and_clamped():
    """naphthalene | an amide on a pyridone with a broken list | biphenyl: the broken graph carries BAD_BONDS, -1, -2 and 255, its
    neighbours their clean results, and the guard tails stay 0xFF (checked in ``run``)"""
    cases = [mol("Cc1ccc2ccccc2c1", seed=1), mol("CC(=O)Nc1ccc(=O)[nH]c1", seed=2), mol("c1ccccc1-c1ccccc1", seed=3)]
    z, lig_ptr, n_lig, bond_ptr, idx, order, aro = collate(cases)
    clean = run(z, lig_ptr, n_lig, bond_ptr, idx, order, aro)
    same(clean, GM.batch_groups(z, lig_ptr, n_lig, bond_ptr, idx, order, aro))
    assert clean[2][:, -1].tolist() == [0, 0, 0]
    b0, b1 = int(bond_ptr[lig_ptr[1]]), int(bond_ptr[lig_ptr[2]])
    a0 = int(lig_ptr[1])

    def swap(bp, bi):             # a bond with j <= i
        bi[:, b0 + 2] = bi[::-1, b0 + 2].copy()

    def equal(bp, bi):
        bi[1, b0 + 1] = bi[0, b0 + 1]

    def leaves(bp, bi):           # a bond that leaves the graph's atom range: into the next graph
        bi[1, b1 - 1] = lig_ptr[2] + 1

    def wild(bp, bi):             # rows no array has
        bi[0, b0] = -7
        bi[1, b0 + 3] = 2 ** 31 - 1
        bi[1, b0 + 4] = n_lig + 1000

    def out_of_order(bp, bi):     # two bonds exchanged
        bi[:, [b0, b0 + 1]] = bi[:, [b0 + 1, b0]]

    def pointer(bp, bi):          # non-monotone inside the graph; the graph's own range is what it was
        bp[a0 + 2] = bp[a0 + 3] + 2

    def everything(bp, bi):
        swap(bp, bi), leaves(bp, bi), pointer(bp, bi), wild(bp, bi)

    n1, m1 = cases[1][0], len(cases[1][1])
    for what in (swap, equal, leaves, wild, out_of_order, pointer, everything):
        bp, bi = bond_ptr.copy(), idx.copy()
        what(bp, bi)
        want = GM.batch_groups(z, lig_ptr, n_lig, bp, bi, order, aro)
        assert want[2][:, -1].tolist() == [0, GM.BAD_BONDS, 0], what.__name__
        got = run(z, lig_ptr, n_lig, bp, bi, order, aro)
        same(got, want)
        assert got[2][1].tolist() == [n1, m1] + [-1] * 30 + [GM.BAD_BONDS]
        assert (got[0][lig_ptr[1]:lig_ptr[2]] == -2).all() and (got[1][lig_ptr[1]:lig_ptr[2]] == 255).all()
        for g in (0, 2):
            assert np.array_equal(got[2][g], clean[2][g]), (what.__name__, g)
            for k in (0, 1):
                assert np.array_equal(got[k][lig_ptr[g]:lig_ptr[g + 1]], clean[k][lig_ptr[g]:lig_ptr[g + 1]]), (what.__name__, g)
    # pointers outside the list at a graph boundary and a lig_ptr outside the atoms: ranges are clamped as the model clamps them
    bp = bond_ptr.copy()
    bp[lig_ptr[2]] = len(idx[0]) + 500
    bp[lig_ptr[1]] = -3
    want = GM.batch_groups(z, lig_ptr, n_lig, bp, idx, order, aro)
    assert (want[2][:, -1] == GM.BAD_BONDS).all()
    same(run(z, lig_ptr, n_lig, bp, idx, order, aro), want)
    lp = lig_ptr.copy()
    lp[0], lp[3] = -4, n_lig + 77
    same(run(z, lp, n_lig, bond_ptr, idx, order, aro), clean)


# ---- argument checks on the device ---------------------------------------------------------------------------------------------------------
def test_no_graphs_null_and_host_memory_arguments():
    lib, p = _native.lib(), _native.ptr
    z, lig_ptr, n_lig, bond_ptr, idx, order, aro = collate([mol("CC(=O)NC"), mol("Cc1ccccc1")])
    nb = idx.shape[1]
    dev = {"z": _dev(z, np.uint8), "lig_ptr": _dev(lig_ptr, np.int32), "bond_ptr": _dev(bond_ptr, np.int32), "bond_index": _dev(idx, np.int32),
           "bond_order": _dev(order, np.uint8), "bond_aromatic": _dev(aro, np.uint8), "atom_group": _ff(n_lig + GUARD, torch.int32),
           "atom_class": _ff(n_lig + GUARD, torch.uint8), "graph_out": _ff(2 * GM.COLS + GUARD, torch.int32)}
    host = {"z": np.asarray(z, np.uint8), "lig_ptr": np.asarray(lig_ptr, np.int32), "bond_ptr": np.asarray(bond_ptr, np.int32),
            "bond_index": np.ascontiguousarray(idx, np.int32), "bond_order": np.asarray(order, np.uint8),
            "bond_aromatic": np.asarray(aro, np.uint8), "atom_group": np.zeros(n_lig, np.int32), "atom_class": np.zeros(n_lig, np.uint8),
            "graph_out": np.zeros(2 * GM.COLS, np.int32)}
    names = ("z", "lig_ptr", "bond_ptr", "bond_index", "bond_order", "bond_aromatic", "atom_group", "atom_class", "graph_out")
    reported = {"z": "z_lig"}

    def call(B=2, **swap):
        a = {k: swap[k] if k in swap else p(dev[k]) for k in names}
        return lib.cbgx_ligand_groups(a["z"], a["lig_ptr"], n_lig, B, a["bond_ptr"], a["bond_index"], a["bond_order"], a["bond_aromatic"], nb,
                                      a["atom_group"], a["atom_class"], a["graph_out"], _native.current_stream(DEV))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((dev[k].view(torch.uint8) == 255).all()) for k in ("atom_group", "atom_class", "graph_out"))

    assert call(B=0) == 0 and untouched()                                        # B == 0: no launch
    for k in names:
        if k != "bond_aromatic":
            assert call(**{k: None}) == -1 and b"NULL" in lib.cbgx_last_error() and untouched(), k
    for k in names:                                                              # plain host memory: refused before any launch, by name
        assert call(**{k: ctypes.c_void_p(host[k].ctypes.data)}) == -1, k
        assert f"{reported.get(k, k)} is not memory the device can read" in lib.cbgx_last_error().decode() and untouched(), k
    assert call(bond_aromatic=None) == 0
    torch.cuda.synchronize()
    grp = dev["atom_group"].cpu().numpy()
    want = GM.batch_groups(z, lig_ptr, n_lig, bond_ptr, idx, order, None)
    assert np.array_equal(grp[:n_lig], want[0]) and (grp[n_lig:] == -1).all()
    assert call() == 0
    torch.cuda.synchronize()
    want = GM.batch_groups(z, lig_ptr, n_lig, bond_ptr, idx, order, aro)
    assert np.array_equal(dev["atom_class"].cpu().numpy()[:n_lig], want[1])
    assert np.array_equal(dev["graph_out"].cpu().numpy()[:2 * GM.COLS].reshape(2, -1), want[2])


# ---- the Python entries -------------------------------------------------------------------------------------------------------------------
def test_ligand_groups_on_tensors(hand):
    cases, (z, lig_ptr, n_lig, bond_ptr, idx, order, aro), want = hand
    lig_b = torch.from_numpy(np.repeat(np.arange(len(cases)), np.diff(lig_ptr))).to(DEV)
    bonds = {"bond_index": _dev(idx, np.int32), "bond_order": _dev(order, np.uint8)}
    aromatic = {"aromatic_bond": _dev(aro, np.uint8).bool(), "bond_type": torch.where(_dev(aro, np.uint8) == 1, 4, _dev(order, np.uint8).long()).to(torch.uint8)}
    out = G.ligand_groups(_dev(z, np.int64), lig_b, len(cases), bonds, aromatic)
    assert sorted(out) == ["atom_class", "atom_group", "graph_counts"] and all(v.device.type == "cuda" for v in out.values())
    assert [out[k].dtype for k in sorted(out)] == [torch.uint8, torch.int32, torch.int32]
    same(tuple(out[k].cpu().numpy() for k in ("atom_group", "atom_class", "graph_counts")), want)
    plain = G.ligand_groups(_dev(z, np.int64), lig_b, len(cases), bonds)
    same(tuple(plain[k].cpu().numpy() for k in ("atom_group", "atom_class", "graph_counts")), GM.batch_groups(z, lig_ptr, n_lig, bond_ptr, idx, order))
    gave_up = dict(aromatic, bond_type=aromatic["bond_type"].clone())
    gave_up["bond_type"][:int(bond_ptr[lig_ptr[1]])] = 255
    out2 = G.ligand_groups(_dev(z, np.int64), lig_b, len(cases), bonds, gave_up)
    assert out2["graph_counts"][:, -1].tolist() == [G.GROUPS_NO_AROMATIC] + [0] * (len(cases) - 1)
    assert torch.equal(out2["graph_counts"][1:], out["graph_counts"][1:])
    s = G.summarise_groups(out["graph_counts"])
    assert s["counts"]["n_mol_evaluated"] == len(cases) and all(s["counts"][f"n_fg_{k}"] >= 1 for k in range(25))
    empty = G.ligand_groups(_dev(z, np.int64)[:0], lig_b[:0], 2, {"bond_index": bonds["bond_index"][:, :0], "bond_order": bonds["bond_order"][:0]})
    assert empty["graph_counts"].tolist() == [[0] * 33] * 2 and empty["atom_group"].shape == (0,)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
GROUP_FIELDS = ("atom_group", "atom_class", "groups", "n_groups", "fg_counts", "groups_status")


def _records(out_dir, n):
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".pt"))
    assert files == [f"pocket_{i:05d}.pt" for i in range(n)]
    return [torch.load(os.path.join(out_dir, f), map_location="cpu", weights_only=False) for f in files]


def _same_field(a, b):
    return _equal(a, b) or (torch.is_tensor(a) and a.is_floating_point() and torch.equal(a.isnan(), b.isnan())
                            and torch.equal(a.nan_to_num(), b.nan_to_num())) or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


def test_sample_cli_groups(tmp_path, capsys):
    """the T = 20 fixture config, three synthetic pockets x two samples, --noise counter, one saved random checkpoint: without the flag the
    records are what they were; with it the per-sample fields are the model's on the graph the file holds; two batches give the records
    of one"""
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    config, _ = C.load_config(cfg)
    C.set_num_atom_type(config)
    torch.manual_seed(123)
    ckpt = tmp_path / "random_init.pt"
    torch.save({"model": C.get_model(config.model).state_dict()}, ckpt)
    tail = ["--synthetic", "3", "--num_samples", "2", "--seed", "2024", "--noise", "counter", "--no_translate", "--checkpoint", str(ckpt)]

    def go(tag, *extra):
        out, stats = tmp_path / tag, {}
        assert sample_cli.main(["--config", cfg, *tail, "--out_root", str(out)] + list(extra), stats=stats) == 0
        d = str(out / os.path.splitext(os.path.basename(cfg))[0])
        return d, _records(d, 3), stats

    whole = ("--pockets_per_batch", "3", "--streams", "1")
    dir_base, base, stats_base = go("base", *whole)
    dir_grp, alone, stats_grp = go("grp", *whole, "--groups")
    dir_all, both, stats_all = go("all", *whole, "--groups", "--aromatic", "--bonds")
    dir_split, split, _ = go("split", "--pockets_per_batch", "2", "--streams", "1", "--groups", "--aromatic", "--bonds")
    printed = capsys.readouterr().out
    assert printed.count("groups: groups_per_mol") == 3 and "not the EFGs program" in printed
    assert stats_grp["groups"] > 0.0 and stats_all["groups"] > 0.0 and "groups" not in stats_base
    assert not {"bonds", "rings", "aromatic"} & set(stats_grp) and list(stats_all)[-1] == "groups"

    # without the flag nothing of it is written, and what is written does not change with it: field by field outside the new keys
    assert not os.path.exists(os.path.join(dir_base, "groups_summary.json"))
    assert sorted(os.listdir(dir_grp)) == sorted(os.listdir(dir_base) + ["groups_summary.json"])
    for r, r2 in zip(base, alone):
        assert sorted(set(r2) - set(r)) == ["groups"] and all(_same_field(r[k], r2[k]) for k in r if k != "samples")
        for s, s2 in zip(r["samples"], r2["samples"]):
            assert sorted(set(s2) - set(s)) == sorted(GROUP_FIELDS)
            assert all(_same_field(s[k], s2[k]) for k in s), [k for k in s if not _same_field(s[k], s2[k])]

    # the new fields against the model on the graph the file holds; alone, with the other flags, and in two batches they are the same
    rows = []
    for rb, ra, rs in zip(both, alone, split):
        assert rb["groups"] == ra["groups"] == rs["groups"] and rb["pocket_index"] == ra["pocket_index"] == rs["pocket_index"]
        assert sorted(rb) == sorted(rs) and all(_same_field(rb[k], rs[k]) for k in rb if k != "samples")
        mine = []
        for sb, sa, ss in zip(rb["samples"], ra["samples"], rs["samples"]):
            for k in GROUP_FIELDS:
                assert _same_field(sb[k], sa[k]), k
            assert sorted(sb) == sorted(ss) and all(_same_field(sb[k], ss[k]) for k in sb), [k for k in sb if not _same_field(sb[k], ss[k])]
            n = len(sb["atom"])
            idx = sb["bond_index"].numpy()
            bond_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx[0], minlength=n))])
            aromatic = np.where(sb["bond_type"].numpy() == 255, 255, sb["aromatic_bond"].numpy().astype(np.uint8))
            grp, cls, row = GM.batch_groups(sb["atom"], [0, n], n, bond_ptr, idx, sb["bond_order"].numpy(), aromatic)
            assert sb["atom_group"].dtype == torch.int32 and sb["atom_class"].dtype == torch.uint8 and sb["fg_counts"].dtype == torch.int64
            assert sb["atom_group"].tolist() == grp.tolist() and sb["atom_class"].tolist() == cls.tolist()
            assert sb["fg_counts"].tolist() == row[0, 6:32].tolist() and sb["n_groups"] == row[0, 2] and sb["groups_status"] == row[0, -1]
            if row[0, -1] == 0:
                want_names = [G.group_name(int(cls[a])) for a in range(n) if grp[a] == a]
                assert sb["groups"] == want_names and len(want_names) == row[0, 2]
            else:
                assert sb["groups"] == []
            mine.append(row[0])
        assert rb["groups"] == G.summarise_groups(np.stack(mine))["counts"]
        rows += mine
    want = G.summarise_groups(np.stack(rows))
    for d in (dir_grp, dir_all, dir_split):
        with open(os.path.join(d, "groups_summary.json")) as f:
            summary = json.load(f)
        assert summary["counts"] == want["counts"] and set(summary) == set(G.GROUP_RATIOS) | {"fg_ratio", "fg_distribution", "counts"}
        assert summary["fg_distribution"] == want["fg_distribution"]
        for k in G.GROUP_RATIOS:
            assert summary[k] == want[k] or np.isnan(summary[k]), k
    assert want["counts"]["n_mol"] == 6
