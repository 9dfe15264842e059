"""Without a GPU: every precondition that tests/test_gpu_stack_backward.py relies on, re-derived from the case builder and the float64
oracle of tests/stack_cases.py -- the committed seeds are clean, removing any single head row would be seen, the lists have the sizes
the cases are named after, and every boundary named in the GPU file's docstring has a case on each side."""
import pytest
import torch

from tests import stack_cases as S

STRICT_INPUTS = list(dict.fromkeys(S.input_key(k) for k in S.all_cases() if S.is_strict(k)))
LOOSE_INPUTS = list(dict.fromkeys(S.input_key(k) for k in S.all_cases() if k.R <= S.STRICT_MAX_HOT and not S.is_strict(k)))


def _key(ik):
    return S.StackKey(*ik[:7], "", ik[7])


def _id(ik):
    return S.key_id(_key(ik))


LARGE_INPUTS = list(dict.fromkeys(S.input_key(k) for k in S.all_cases() if k.R in S.R_LARGE and k.L == 1))


def test_seed_table_matches_the_cases():
    assert set(S.SEEDS) == set(STRICT_INPUTS) | set(LARGE_INPUTS)
    ids = [S.key_id(k) for k in S.all_cases()]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("ik", STRICT_INPUTS, ids=_id)
def test_strict_case_preconditions(ik):
    """the committed seed gives inputs on which no ReLU that carries gradient is within rounding of its kink, and (head families) the
    removal of ANY single listed row's contribution dlogits_i (x) act_i moves one of the four classifier gradients by more than 10 x
    its tolerance"""
    k = _key(ik)
    c = S.build(k, S.SEEDS[ik])
    res = S.oracle(c)
    bad = S.carrying_near(c, res)
    assert not bad, f"{len(bad)} pre-ReLU value(s) within {S.FLIP_EPS} of zero on units that carry gradient, e.g. {bad[:3]}: " \
                    f"pick another seed (python -m tests.stack_cases {k.family})"
    assert len(c.hot) == k.R and int(c.gen.sum()) == k.g and set(c.gen.nonzero().flatten().tolist()) <= set(c.hot)
    if k.family in ("head", "dense", "classes"):
        sens = S.head_sensitivity(c, res)
        assert sorted(sens) == sorted(c.hot)
        assert all(v > 10.0 for v in sens.values()), min(sens.values())
        if k.mode == "full" and k.R >= 7:
            assert bool((~c.lig[c.hot]).any()), "the hot rows of a full-mode head case must include protein rows"


@pytest.mark.parametrize("ik", LOOSE_INPUTS, ids=_id)
def test_cases_that_are_not_strict_cannot_be(ik):
    """a case of at most 65 hot rows takes the ONE-flip form of gerr only where find_seed's probe shows that no seed can be expected to
    be clean: more than PROBE_MAX near-zero units that carry gradient, on average over the first seeds"""
    k = _key(ik)
    counts = []
    for seed in range(S.PROBE_SEEDS):
        c = S.build(k, seed)
        counts.append(len(S.carrying_near(c, S.oracle(c, backward=False))))
    assert 0 not in counts, counts
    assert sum(counts) / len(counts) > S.PROBE_MAX or S.find_seed(k) is None, counts      # (or: searched, and none of 400 seeds is clean)


def test_flip_selection_names_the_flipped_units():
    """select_flips on gradients that ARE the oracle's with two units flipped: it names exactly those two"""
    k = S.StackKey("depth", 47, 10, 13, "lo", 9, 3, "", "xl")
    c = S.build(k, 0)
    res = S.oracle(c)
    heavy = sorted(res["influence"], key=lambda u: -res["influence"][u])[:2]
    force = {}
    for p, r, u in heavy:
        force.setdefault(p, []).append((r, u))
    flipped = S.oracle(c, force=force)["ref"]
    assert S.select_flips(res["ref"], res) == {}
    got = S.select_flips(flipped, res)
    assert {(p, r, u) for p, lst in got.items() for r, u in lst} == set(heavy)


@pytest.mark.parametrize("ik", LARGE_INPUTS, ids=_id)
def test_large_case_seeds(ik):
    """the 2048 / 2049-row head cases: the committed seed is the one with the fewest heavy near-zero units (find_seed)"""
    assert S.find_seed(_key(ik)) == S.SEEDS[ik]


@pytest.mark.parametrize("k", [k for k in S.cases_list_vs_grid() if k.variant == ""],
                         ids=S.key_id)
def test_lists_have_the_sizes_the_cases_are_named_after(k):
    """g = 0: A1 is exactly the R hot rows (the head list too) and A2 = A1 + nbr(A1); g > 0: A1 also holds nbr(gen).  The last row
    (6-node graph) and the 1-node graph's row are listed from R = 1 / R = 2 on, so the last list entry has edges."""
    c = S.build(k, S.seed_of(k))
    a1, a2 = S.list_sizes(c)
    assert len(S.head_rows(c)) == k.R == int(c.lig.sum()) and int(c.gen.sum()) == k.g
    if k.g == 0:
        assert a1 == k.R
    else:
        assert k.R <= a1 <= k.R + 32 * k.g
    assert a1 <= a2 <= k.n and (a2 > a1 or k.R in (0, k.n) or a1 == k.n)
    if k.R >= 1:
        assert k.n - 1 in c.hot
    if k.R >= 2:
        assert k.n - 7 in c.hot and S.graph_sizes(k.n)[-2:] == [1, 6]
    if k.R <= S.STRICT_MAX_HOT and k.n > 600:
        last = len(S.graph_sizes(k.n)) - 1          # the oracle evaluates the first graph and the two small ones only
        assert set(c.hot_graphs) <= {0, last - 1, last}


def test_every_boundary_has_a_case_on_each_side():
    cases = S.all_cases()
    have = lambda **kw: any(all(getattr(k, f) == v for f, v in kw.items()) for k in cases)
    # list count against grid: the three grids, counts on both sides of the 8-row groups / 16- / 32- / 64-row tiles, the 2048-row cap
    for n in S.GRID_N:
        for lo in (8, 16, 32):
            for R in (lo - 1, lo, lo + 1):
                assert have(family="grid", n=n, R=R, g=0)
        assert have(family="grid", n=n, R=0) and have(family="grid", n=n, R=1)
    for n in (600, 2100):
        for R in (63, 64, 65):
            assert have(family="grid", n=n, R=R, g=0) and have(family="grid", n=n, R=R, g=1) and have(family="grid", n=n, R=R, g=9)
    assert have(family="grid", n=47, R=47)
    for g in (0, 1, 9):
        assert have(family="grid", n=2100, R=2048, g=g) and have(family="grid", n=2100, R=2049, g=g)
    for R in S.R_SWEEP:
        assert have(family="grid", n=600, R=R, variant="edge_rows")
    # the listed head in both modes
    for mode in ("lo", "full"):
        for R in S.R_SWEEP:
            assert have(family="head", n=600, mode=mode, R=R)
        assert have(family="head", n=2100, mode=mode, R=2048) and have(family="head", n=2100, mode=mode, R=2049)
    # the dense head: node_grid's cap (256 / 257), splits_for's step (512 / 513), the colsum's second pass of 8 x 256 rows (2048 / 2049), n = 1, 2
    for n in (1, 2, 255, 256, 257, 512, 513, 2048, 2049):
        assert have(family="dense", n=n, variant="dense", mode="full")
    # classes: sgemm's 16-wide K staging and 64-wide tiles, node_linear's 16-column tiles, the marking's 64-lane halves, the ABI's ends
    for C in (1, 2, 8, 15, 16, 17, 32, 33, 63, 64, 65, 127, 128):
        for mode, variant in (("lo", ""), ("full", ""), ("full", "dense")):
            assert have(family="classes", C=C, mode=mode, variant=variant)
    # depth: pruning from 3 layers, PACK_BLOCKS_MAX = 20 blocks per pack pass (10 / 11 layers), QLN_SLOTS = 64 (2 L <= 64: 33 is past it)
    for L in (1, 2, 3, 4, 10, 11, 33):
        for mode in S.MODES:
            assert have(family="depth", L=L, mode=mode, n=47)
    for L in (2, 3):
        assert have(family="depth", L=L, variant="edge_rows")
    assert 2 * 33 > 64 >= 2 * 11 and 2 * 10 == 20
    for L in (1, 3):
        assert have(family="absent", L=L, loss="x") and have(family="absent", L=L, loss="h") and have(family="absent", L=L, R=0, mode="lo")
    assert have(family="absent", L=1, loss="l")


def test_constants_follow_the_sources():
    """the switches the cases straddle, as the sources state them"""
    import os
    import cbgbench_amd
    csrc = os.path.join(os.path.dirname(os.path.abspath(cbgbench_amd.__file__)), "csrc")
    text = open(os.path.join(csrc, "api_train.hip")).read()
    for line in ("constexpr int EDGE_GRID = 256;", "constexpr int QLN_SLOTS = 64;", "#define CBGX_NODE_GRID 256", "&& L >= 3;",
                 "const bool qln_slots = 2 * L <= QLN_SLOTS;"):
        assert line in text, line
    assert "constexpr int PACK_BLOCKS_MAX = 20;" in open(os.path.join(csrc, "kernels.h")).read()
    tests = os.path.join(os.path.dirname(csrc), "..", "tests")
    assert "tol = TOL if k in (\"x\", \"h\") else 1e-3" in open(os.path.join(tests, "test_gpu_coord_grad.py")).read() and S.PARAM_TOL == 1e-3
    assert "#define CBGX_MAX_CLASSES 128" in open(os.path.join(os.path.dirname(csrc), "..", "include", "cbgx.h")).read()


def test_row_bound_sees_a_missing_and_a_doubled_row():
    """the 2048 / 2049-row cases rely on row_failures: dropping or doubling ONE row's gradient fails it, rounding noise does not"""
    k = S.StackKey("head", 2100, 1, 13, "lo", 2049, 0, "", "l")
    g = torch.Generator().manual_seed(3)
    ref = torch.zeros(k.n, 128, dtype=torch.float64)
    rows = torch.randperm(k.n, generator=g)[:k.R]
    ref[rows] = torch.randn(k.R, 128, generator=g, dtype=torch.float64)
    noisy = ref * (1 + 2e-4 * torch.randn(ref.shape, generator=g, dtype=torch.float64))
    assert not S.row_failures(noisy, ref, "h")[1]
    for scale in (0.0, 2.0):
        broken = noisy.clone()
        broken[rows[-1]] *= scale
        worst, msgs = S.row_failures(broken, ref, "h")
        assert msgs and worst > 50
