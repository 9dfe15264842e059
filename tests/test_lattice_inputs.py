"""The lattice batches of tests/lattice.py exercise what tests/test_gpu_forward_lists.py needs them for: re-derived here, without a
GPU, with the oracle's knn_graph.  These are conditions on the inputs, not measurements of the code under test."""
import numpy as np
import pytest

from tests import lattice

NAMES = sorted(lattice.SEEDS)


def test_batch_shapes_and_regimes():
    assert lattice.SMALL_NODES == 5885 <= lattice.LIST_REGIME_MAX
    n = {name: lattice.batch(name)["x"].shape[0] for name in NAMES}
    assert n["small"] == n["context"] == 5885
    assert n["at_threshold"] == 8192 and n["above_threshold"] == 8193 and 8193 < n["large"] < 9000
    for name in NAMES:
        b = lattice.batch(name)
        assert b["sizes"][:len(lattice.SMALL_SIZES)] == lattice.SMALL_SIZES
        x = b["x"].numpy()
        assert np.array_equal(x, np.round(x / 0.75) * 0.75) and np.abs(x).max() < 64          # exact in fp32, squares and sums too
        assert np.abs(x.mean(0)).max() > 0.5, "the batch is not to be centred"
        lig, gen, gp = b["lig_flag"].numpy(), b["gen_flag"].numpy(), b["graph_ptr"].numpy()
        assert not (gen & ~lig).any()
        for g, (n_rec, n_lig) in enumerate(b["sizes"]):         # ligand rows close each graph
            s, e = gp[g], gp[g + 1]
            assert e - s == n_rec + n_lig and not lig[s:s + n_rec].any() and lig[s + n_rec:e].all()
        if name == "context":
            fixed = lig & ~gen
            assert fixed.sum() > 100 and (gen.sum() > fixed.sum())
            rows = np.nonzero(lig)[0]
            flips = (gen[rows][1:] != gen[rows][:-1]).sum()
            assert flips > fixed.sum(), "context atoms are interleaved with the generated ones"
        else:
            assert np.array_equal(gen, lig)
    # the same seed gives the same batch
    assert np.array_equal(lattice.make("small")["x"].numpy(), lattice.batch("small")["x"].numpy())


@pytest.mark.parametrize("name", NAMES)
def test_batches_hold_the_ties_they_claim(name):
    b = lattice.batch(name)
    rep = lattice.tie_report(b)
    for r in rep:
        if r["n"] > 33:
            assert r["ties_32_33"] >= 1, r
    assert sum(r["ties_32_33_mixed"] for r in rep) >= 1, "no rank-32/33 tie between a protein and a ligand atom"
    assert sum(r["ligand_at_cached_32nd"] for r in rep) >= 1, "no protein atom with its nearest ligand atom at the cached 32nd distance"
    assert sum(r["coincident"] for r in rep) >= 1, "no coincident pair"
    # the reference graph itself: sorted by (d2, index) within a centre, -1 padded past the degree
    ref = lattice.reference(b)
    d2, nbr, deg = ref["d2"], ref["nbr"], ref["deg"]
    pad = np.arange(32)[None, :] >= deg[:, None]
    assert (nbr[pad] == -1).all() and (nbr[~pad] >= 0).all()
    both = ~pad[:, 1:]
    assert (d2[:, 1:][both] >= d2[:, :-1][both]).all()
    tied = both & (d2[:, 1:] == d2[:, :-1])
    assert tied.sum() > 1000 and (nbr[:, 1:][tied] > nbr[:, :-1][tied]).all()


@pytest.mark.parametrize("name", NAMES)
def test_lists_of_the_large_pockets_are_strict_subsets(name):
    b = lattice.batch(name)
    defs = lattice.list_definitions(b)
    gp, lig = b["graph_ptr"].numpy(), b["lig_flag"].numpy()
    seen = 0
    for g, (n_rec, n_lig) in enumerate(b["sizes"]):
        if n_rec < 760:
            continue
        seen += 1
        s, e = gp[g], gp[g + 1]
        for k in ("A1", "A2", "A3", "D1", "D2", "S1", "S2", "act"):
            c = int(((defs[k] >= s) & (defs[k] < e)).sum())
            assert 0 < c < e - s, (g, k, c)
        d1 = defs["D1"][(defs["D1"] >= s) & (defs["D1"] < e)]
        frac = (~lig[d1]).sum() / n_rec
        assert 0.02 < frac < 0.6, (g, frac)
        for k in ("all", "D2", "A1", "A2"):       # both roles of every pair occur (A1 is almost all general: the batch decides below)
            gen_c = int(((defs[k + "_general"] >= s) & (defs[k + "_general"] < e)).sum())
            assert gen_c > 0, (g, k)
    assert seen >= 3
    for k in ("all", "D2", "A1", "A2"):
        assert defs[k + "_protein"].size > 0 and defs[k + "_general"].size > 0, k
    # every pair partitions its set
    for k, whole in (("D2", defs["D2"]), ("A1", defs["A1"]), ("A2", defs["A2"])):
        assert np.array_equal(np.sort(np.concatenate([defs[k + "_general"], defs[k + "_protein"]])), whole)
