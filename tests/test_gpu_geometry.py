"""Geometry report on the GPU (csrc/geometry.hip: cbgx_ligand_geometry; cbgbench_amd/geometry.py; sample_cli --geometry) against the
numpy model of tests/geometry_model.py.  Every output is an integer and every comparison is ``==``: no tolerance.  Output buffers handed to
the entry are pre-filled with 0xFF bytes (nr_bonds = -1, flags = 255, counts = -1: values no result can take), so equality with the model
also shows that every element of every graph was written."""
import json
import os

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, geometry as G, synthetic
from cbgbench_amd.priors import PROTEIN_ELEMENTS
from tests import geometry_model as GM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
F32 = np.float32


def run(x_lig, z_lig, lig_ptr, x_rec, z_rec, rec_ptr):
    """the entry on a batch in CSR form, outputs pre-filled with 0xFF bytes -> numpy dict like the model's"""
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)
    x_lig, x_rec = t(np.asarray(x_lig, F32).reshape(-1, 3), F32), t(np.asarray(x_rec, F32).reshape(-1, 3), F32)
    z_lig, z_rec, lig_ptr, rec_ptr = t(z_lig, np.uint8), t(z_rec, np.uint8), t(lig_ptr, np.int32), t(rec_ptr, np.int32)
    n_lig, n_rec, B = x_lig.shape[0], x_rec.shape[0], lig_ptr.shape[0] - 1
    nr = torch.full((n_lig,), -1, dtype=torch.int32, device=DEV)
    fl = torch.full((n_lig,), 255, dtype=torch.uint8, device=DEV)
    gc = torch.full((B, 6), -1, dtype=torch.int32, device=DEV)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_geometry(p(x_lig), p(z_lig), p(lig_ptr), n_lig, p(x_rec), p(z_rec), p(rec_ptr), n_rec, B, p(nr),
                                                     p(fl), p(gc), _native.current_stream(DEV)), "cbgx_ligand_geometry")
    torch.cuda.synchronize()
    return {"nr_bonds": nr.cpu().numpy(), "flags": fl.cpu().numpy(), "graph_counts": gc.cpu().numpy()}


def collate(graphs):
    """[(x_lig, z_lig, x_rec, z_rec), ...] -> CSR batch"""
    cat = lambda k, dt, shape: np.concatenate([np.asarray(g[k], dt).reshape(shape) for g in graphs]) if graphs else np.zeros(shape, dt)
    ptr = lambda k: np.concatenate([[0], np.cumsum([len(np.asarray(g[k]).reshape(-1)) for g in graphs])]).astype(np.int32)
    return cat(0, F32, (-1, 3)), cat(1, np.uint8, (-1,)), ptr(1), cat(2, F32, (-1, 3)), cat(3, np.uint8, (-1,)), ptr(3)


def same(got, want):
    for k in ("nr_bonds", "flags", "graph_counts"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.flatnonzero((got[k] != want[k]).reshape(-1))[:10])


# ---- thresholds, hand-built ----------------------------------------------------------------------------------------------------------
def _around(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def test_bond_thresholds_are_strict():
    """N-O at exactly 1.5 A: p = 150 = 140 + 10, order 0.  C-O at exactly 1.25 A: p = 125 = 120 + 5, order 1, not 2.  Each along an axis and
    off it -- (0.75, 1.0, 0) has length 1.25 exactly; 1.5 has no exact two-component split in binary, (0.5, 1.0, 1.0) is its exact
    three-component one -- and at the float32 neighbours of the axis value, one step below and above.  One two-atom graph per case:
    nr_bonds of both atoms is the pair's order."""
    none = (np.zeros((0, 3), F32), np.zeros(0, np.uint8))
    cases, want = [], []
    for za, zb, d, off_axis, orders in ((7, 8, 1.5, (0.5, 1.0, 1.0), (1, 0, 0)), (6, 8, 1.25, (0.75, 1.0, 0.0), (2, 1, 1))):
        for v, order in zip(_around(d), orders):
            for axis in range(3):
                x = np.zeros((2, 3), F32)
                x[1, axis] = v
                cases.append((x, [za, zb]) + none)
                want.append(order)
        cases.append((np.array([[0, 0, 0], off_axis], F32), [za, zb]) + none)
        want.append(orders[1])
        cases.append((np.array([off_axis, [0, 0, 0]], F32), [zb, za]) + none)
        want.append(orders[1])
    batch = collate(cases)
    got = run(*batch)
    same(got, GM.batch_geometry(*batch))
    assert got["nr_bonds"].reshape(-1, 2).tolist() == [[o, o] for o in want]


def test_clash_threshold_is_strict():
    """a C...C protein-ligand pair at the float32 value nearest the model's threshold (1.7 + 1.7) - 0.4 and at its two neighbours: a clash
    iff the float32 distance, widened, is below the float64 threshold"""
    T = G.tables()
    r = T["vdw_r"][list(T["vdw_z"]).index(6)]
    thr = (r + r) - T["tolerance"]
    cases, want = [], []
    for v in _around(thr):
        for axis in range(3):
            x_rec = np.zeros((1, 3), F32)
            x_rec[0, axis] = v
            cases.append((np.zeros((1, 3), F32), [6], x_rec, [6]))
            want.append(bool(float(v) < thr))
    assert True in want and False in want
    batch = collate(cases)
    got = run(*batch)
    same(got, GM.batch_geometry(*batch))
    assert ((got["flags"] & GM.INTER) != 0).tolist() == want and got["graph_counts"][:, 3].tolist() == [int(w) for w in want]


def test_valence_overflow():
    """carbon with five hydrogens at 1.09 A (trigonal bipyramid) is unstable, the hydrogens are stable; methane is a stable molecule"""
    s = np.sqrt(3.0) / 2
    five = 1.09 * np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-0.5, s, 0], [-0.5, -s, 0]])
    four = 1.09 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
    none = (np.zeros((0, 3), F32), np.zeros(0, np.uint8))
    batch = collate([(np.concatenate([np.zeros((1, 3)), five]), [6] + [1] * 5) + none,
                     (np.concatenate([np.zeros((1, 3)), four]), [6] + [1] * 4) + none])
    got = run(*batch)
    same(got, GM.batch_geometry(*batch))
    assert got["nr_bonds"].tolist() == [5, 1, 1, 1, 1, 1, 4, 1, 1, 1, 1]
    assert (got["flags"] & GM.STABLE).tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    # the hydrogens have no table bond with each other (H-H: below 0.84 A) and are closer than (1.2 + 1.2) - 0.4 = 2.0 A -- 1.54 / 1.89 A
    # in the bipyramid, 1.78 A in methane --: every hydrogen carries the intra-clash flag, the carbon (bonded to all of them) does not
    assert ((got["flags"] & GM.INTRA) != 0).tolist() == [False] + [True] * 5 + [False] + [True] * 4
    assert got["graph_counts"].tolist() == [[6, 5, 0, 0, 5, 0], [5, 5, 1, 0, 4, 0]]


# ---- regime boundaries ---------------------------------------------------------------------------------------------------------------
LIG_SIZES = (0, 1, 2, 255, 256, 257, 1024, 0)        # around the 256 threads of a workgroup, and the LDS capacity
REC_SIZES = (256, 257, 1025, 0, 1, 255, 256, 0)      # paired off with them; (0, 0) is the graph with nothing in it


@pytest.fixture(scope="module")
def regime_batch():
    """seeded graphs: ligands are chains with 0.7-1.6 A steps (all bond orders, stable and unstable atoms, non-bonded close contacts),
    protein atoms are scattered around ligand atoms (clashing and free), Se among them; one ligand atom is Br"""
    rng = np.random.default_rng(7)
    graphs = []
    for n, m in zip(LIG_SIZES, REC_SIZES):
        step = rng.uniform(0.7, 1.6, size=(n, 1))
        u = rng.normal(size=(n, 3))
        x = np.cumsum(step * u / np.linalg.norm(u, axis=1, keepdims=True), axis=0).astype(F32).reshape(-1, 3)
        z = np.array([1, 6, 7, 8, 9, 15, 16, 17], np.uint8)[rng.choice(8, size=n, p=[.1, .4, .15, .15, .05, .05, .05, .05])]
        if n == 257:
            z[100] = 35
        if n == 2:                                   # a C-C single bond: two stable atoms, a stable molecule
            x, z = np.array([[0, 0, 0], [1.5, 0, 0]], F32), np.array([6, 6], np.uint8)
        anchor = x[rng.integers(0, n, size=m)] if n else np.zeros((m, 3))
        x_rec = (anchor + rng.normal(scale=3.0, size=(m, 3))).astype(F32)
        z_rec = np.array([1, 6, 7, 8, 16, 34], np.uint8)[rng.choice(6, size=m, p=[.05, .55, .15, .15, .05, .05])]
        graphs.append((x, z, x_rec, z_rec))
    batch = collate(graphs)
    return graphs, batch, GM.batch_geometry(*batch)


def test_regime_batch_reaches_every_case(regime_batch):
    graphs, batch, want = regime_batch
    assert batch[2].tolist() == np.concatenate([[0], np.cumsum(LIG_SIZES)]).tolist()
    assert batch[5].tolist() == np.concatenate([[0], np.cumsum(REC_SIZES)]).tolist()
    for bit in (GM.STABLE, GM.INTER, GM.INTRA, GM.UNKNOWN):
        on = (want["flags"] & bit) != 0
        assert on.any() and not on.all(), bit
    assert int(((want["flags"] & GM.UNKNOWN) != 0).sum()) == 1
    orders = set()
    for x, z, _, _ in graphs:
        orders |= set(np.unique(GM.bond_orders(x, z)[0]).tolist()) if len(z) else set()
    assert orders == {0, 1, 2, 3}
    gc = want["graph_counts"]
    assert gc[:, 0].tolist() == list(LIG_SIZES) and (gc[:, 5] > 0).sum() >= 3 and gc[:, 2].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert gc[0].tolist()[:5] == [0, 0, 0, 0, 0] and gc[7].tolist() == [0] * 6


def test_regime_batch_equals_the_model(regime_batch):
    _, batch, want = regime_batch
    same(run(*batch), want)


def test_each_graph_alone_gives_its_rows_of_the_batch(regime_batch):
    graphs, batch, want = regime_batch
    whole = run(*batch)
    same(whole, want)
    lp = batch[2]
    for g, graph in enumerate(graphs):
        alone = run(*collate([graph]))
        assert np.array_equal(alone["nr_bonds"], whole["nr_bonds"][lp[g]:lp[g + 1]]), g
        assert np.array_equal(alone["flags"], whole["flags"][lp[g]:lp[g + 1]]), g
        assert np.array_equal(alone["graph_counts"][0], whole["graph_counts"][g]), g


def test_python_entry(regime_batch):
    """ligand_geometry builds the CSR from the graph indices and returns device tensors equal to the model; an index vector that is not
    grouped by graph and a ligand above 1024 atoms raise ValueError"""
    _, batch, want = regime_batch
    x_lig, z_lig, lp, x_rec, z_rec, rp = batch
    B = len(lp) - 1
    lig_b = torch.from_numpy(np.repeat(np.arange(B), np.diff(lp))).to(DEV)
    rec_b = torch.from_numpy(np.repeat(np.arange(B), np.diff(rp))).to(DEV)
    t = lambda a: torch.from_numpy(a).to(DEV)
    out = G.ligand_geometry(t(x_lig), t(z_lig).long(), lig_b, t(x_rec), t(z_rec).long(), rec_b, B)
    assert all(v.device.type == "cuda" for v in out.values())
    same({k: v.cpu().numpy() for k, v in out.items()}, want)
    with pytest.raises(ValueError, match="not grouped"):
        G.ligand_geometry(t(x_lig), t(z_lig), lig_b.flip(0), t(x_rec), t(z_rec), rec_b, B)
    big = torch.zeros(1025, 3, device=DEV)
    zero = torch.zeros(1025, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="1025"):
        G.ligand_geometry(big, zero + 6, zero, big[:0], zero[:0], zero[:0], 1)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
NEW_FIELDS = ("nr_bonds", "atom_stable", "inter_clash", "intra_clash_table_bonds", "mol_stable")


def _records(out_dir):
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".pt"))
    assert files == [f"pocket_{i:05d}.pt" for i in range(3)]
    return [torch.load(os.path.join(out_dir, f), weights_only=False) for f in files]


def _equal(a, b):
    return (a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)) if torch.is_tensor(a) else a == b


def test_sample_cli_geometry(tmp_path, capsys):
    """the T = 20 fixture config, three synthetic pockets x two samples, --noise counter, one saved random checkpoint, --no_translate:
    with --geometry every pre-existing field of every pocket file equals the run without it; the new fields equal the model on the
    file's own pos / atom and the pocket's protein_pos; geometry_summary.json equals summarise over the files; and the run split into
    one pocket per batch gives the same geometry fields."""
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    config, _ = C.load_config(cfg)
    C.set_num_atom_type(config)
    torch.manual_seed(123)
    ckpt = tmp_path / "random_init.pt"
    torch.save({"model": C.get_model(config.model).state_dict()}, ckpt)
    common = ["--config", cfg, "--synthetic", "3", "--num_samples", "2", "--checkpoint", str(ckpt), "--seed", "2024", "--noise", "counter",
              "--no_translate"]

    def go(tag, *extra):
        out, stats = tmp_path / tag, {}
        assert sample_cli.main(common + ["--out_root", str(out)] + list(extra), stats=stats) == 0
        return out / "targetdiff_T20", _records(out / "targetdiff_T20"), stats

    dir_plain, plain, stats_plain = go("plain", "--pockets_per_batch", "3", "--streams", "1")
    dir_geo, geo, stats_geo = go("geo", "--pockets_per_batch", "3", "--streams", "1", "--geometry")
    _, split, _ = go("split", "--pockets_per_batch", "1", "--streams", "3", "--geometry")
    assert "geometry" not in stats_plain and stats_geo["geometry"] > 0.0
    assert not os.path.exists(os.path.join(dir_plain, "geometry_summary.json"))
    assert "geometry: mol_stable" in capsys.readouterr().out
    # the pockets sample_cli made (its own recipe: synthetic.make_pocket from default_rng(seed))
    rng0 = np.random.default_rng(2024)
    pockets = [synthetic.make_pocket(rng0, int(rng0.integers(350, 651))) for _ in range(3)]
    counts = []
    for rp, rg, rs, (ppos, feat, _) in zip(plain, geo, split, pockets):
        assert sorted(set(rg) - set(rp)) == ["geometry"] and set(rp) <= set(rg)
        assert rp["pocket_index"] == rg["pocket_index"] and len(rp["samples"]) == len(rg["samples"]) == 2
        z_rec = PROTEIN_ELEMENTS.numpy()[feat[:, :6].argmax(-1)]
        mine = []
        for sp, sg, ss in zip(rp["samples"], rg["samples"], rs["samples"]):
            assert sorted(set(sg) - set(sp)) == sorted(NEW_FIELDS) and set(sp) <= set(sg)
            for k in sp:
                assert _equal(sp[k], sg[k]), k
            nr, flags, c = GM.graph_geometry(sg["pos"].numpy(), np.asarray(sg["atom"]), ppos, z_rec)
            assert sg["nr_bonds"].dtype == torch.int32 and np.array_equal(sg["nr_bonds"].numpy(), nr)
            assert np.array_equal(sg["atom_stable"].numpy(), (flags & GM.STABLE) != 0)
            assert np.array_equal(sg["inter_clash"].numpy(), (flags & GM.INTER) != 0)
            assert np.array_equal(sg["intra_clash_table_bonds"].numpy(), (flags & GM.INTRA) != 0)
            assert sg["mol_stable"] is bool(c[2])
            for k in NEW_FIELDS:
                assert _equal(sg[k], ss[k]), k
            mine.append(c)
        assert rg["geometry"] == G.summarise(np.stack(mine))["counts"] == rs["geometry"]
        counts += mine
    with open(os.path.join(dir_geo, "geometry_summary.json")) as f:
        summary = json.load(f)
    want = G.summarise(np.stack(counts))
    assert summary["counts"] == want["counts"]
    for k in G.RATIOS:
        assert summary[k] == want[k] or (np.isnan(summary[k]) and np.isnan(want[k]))
