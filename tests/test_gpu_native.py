"""The comparison with a pocket's native ligand on the GPU (csrc/native.hip: cbgx_pocket_contacts, cbgx_native_compare;
cbgbench_amd/geometry.py; sample_cli --native) against the numpy / Python-int model of tests/native_model.py.  Every comparison is ``==``
(NaN positions equal).  Output buffers handed to the entries are pre-filled with 0xFF bytes and carry a 0xFF guard tail inside the same
allocation, which must stay as it is."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, geometry as G, synthetic
from cbgbench_amd.sample_reports import SampleReports
from tests import native_model as NM
from tests.test_gpu_rings import DEV, GUARD, _dev, _equal, _ff
from tests.test_native import NATIVE_FIELDS, words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = NM.WORDS


def run_contacts(x_lig, z_lig, lig_ptr, x_rec, z_rec, rec_ptr, cutoff2=NM.CUTOFF2):
    """the entry on 0xFF outputs with guard tails -> (rec_contact, lig_contact, centroid [B, 3], graph_out [B, 6]); what the kernel does
    not write reads 0xFF, which is what the model leaves there; the guards are checked here"""
    x_lig, x_rec = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(x_rec, np.float32).reshape(-1, 3)
    n_lig, n_rec, B = x_lig.shape[0], x_rec.shape[0], len(lig_ptr) - 1
    xl, zl, lp, xr, zr, rp = (_dev(x_lig, np.float32), _dev(z_lig, np.uint8), _dev(lig_ptr, np.int32), _dev(x_rec, np.float32),
                              _dev(z_rec, np.uint8), _dev(rec_ptr, np.int32))
    rc, lc = _ff(n_rec + GUARD, torch.uint8), _ff(n_lig + GUARD, torch.uint8)
    cen, out = _ff(3 * B + GUARD, torch.float64), _ff(NM.CONTACT_COLS * B + GUARD, torch.int32)
    p = _native.ptr
    some = lambda t: p(t) if t.numel() else None
    _native.check(_native.lib().cbgx_pocket_contacts(some(xl), some(zl), p(lp), n_lig, some(xr), some(zr), p(rp), n_rec, B, float(cutoff2),
                                                     p(rc), p(lc), p(cen), p(out), _native.current_stream(DEV)), "cbgx_pocket_contacts")
    torch.cuda.synchronize()
    rc, lc, cen, out = rc.cpu().numpy(), lc.cpu().numpy(), cen.cpu().numpy(), out.cpu().numpy()
    assert (rc[n_rec:] == 255).all() and (lc[n_lig:] == 255).all() and (cen[3 * B:].view(np.int64) == -1).all()
    assert (out[NM.CONTACT_COLS * B:] == -1).all()
    return rc[:n_rec], lc[:n_lig], cen[:3 * B].reshape(B, 3), out[:NM.CONTACT_COLS * B].reshape(B, NM.CONTACT_COLS)


def same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == np.float64:
            assert NM.same_floats(g, w), np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:10].tolist()
        else:
            assert np.array_equal(g, w), np.argwhere(g != w)[:10].tolist()


def collate(graphs):
    """[(x_lig, z_lig, x_rec, z_rec)] -> the arguments of run_contacts and of the model"""
    lig_ptr = np.concatenate([[0], np.cumsum([len(g[1]) for g in graphs])]).astype(np.int32)
    rec_ptr = np.concatenate([[0], np.cumsum([len(g[3]) for g in graphs])]).astype(np.int32)
    cat = lambda k, dt, shape: np.concatenate([np.asarray(g[k], dt).reshape(shape) for g in graphs])
    return cat(0, np.float32, (-1, 3)), cat(1, np.uint8, (-1,)), lig_ptr, cat(2, np.float32, (-1, 3)), cat(3, np.uint8, (-1,)), rec_ptr


def graph(rng, n_lig, n_rec, lig_h=0.15, rec_h=0.15):
    """a ligand in a ball of a few A inside a pocket box of +-9 A: some pocket atoms within 4 A, most not; a share of hydrogens"""
    z = lambda n, h: np.where(rng.random(n) < h, 1, rng.choice([6, 7, 8, 16, 0, 35], n)).astype(np.uint8)
    return (rng.normal(size=(n_lig, 3)).astype(np.float32) * 2.5, z(n_lig, lig_h),
            rng.uniform(-9, 9, size=(n_rec, 3)).astype(np.float32), z(n_rec, rec_h))


LIG_SIZES, REC_SIZES = (0, 1, 63, 64, 65, 256, 257, 1024), (0, 1, 63, 64, 65, 1025, 8193)


@pytest.fixture(scope="module")
def shapes():
    """every ligand size with a pocket size and back, the extremes together, and all-hydrogen sides; the model's answer, once"""
    rng = np.random.default_rng(41)
    graphs = [graph(rng, n, REC_SIZES[(k + 3) % len(REC_SIZES)]) for k, n in enumerate(LIG_SIZES)]
    graphs += [graph(rng, 1024, 8193), graph(rng, 0, 0), graph(rng, 65, 64, lig_h=1.0), graph(rng, 64, 65, rec_h=1.0), graph(rng, 1, 1, 0.0, 0.0)]
    assert {len(g[1]) for g in graphs} >= set(LIG_SIZES) and {len(g[3]) for g in graphs} >= set(REC_SIZES)
    want = NM.pocket_contacts(*collate(graphs), len(graphs))
    assert want[3][:, 3].max() > 100 and (want[3][:, 5] == NM.EMPTY).sum() >= 3 and 0.1 < want[0].mean() < 0.9
    return graphs, want


def test_contact_shapes_against_the_model(shapes):
    graphs, want = shapes
    same(run_contacts(*collate(graphs)), want)


def test_every_graph_alone_twice_and_reversed_in_a_batch_of_65(shapes):
    graphs, want = shapes
    lig_ptr, rec_ptr = collate(graphs)[2], collate(graphs)[5]

    def rows(g):
        return (want[0][rec_ptr[g]:rec_ptr[g + 1]], want[1][lig_ptr[g]:lig_ptr[g + 1]], want[2][g:g + 1], want[3][g:g + 1])
    for g, one in enumerate(graphs):
        for _ in range(2):
            same(run_contacts(*collate([one])), rows(g))
    order = [g for _ in range(5) for g in reversed(range(len(graphs)))]
    assert len(order) == 65
    got = run_contacts(*collate([graphs[g] for g in order]))
    lp, rp = collate([graphs[g] for g in order])[2], collate([graphs[g] for g in order])[5]
    for k, g in enumerate(order):
        same((got[0][rp[k]:rp[k + 1]], got[1][lp[k]:lp[k + 1]], got[2][k:k + 1], got[3][k:k + 1]), rows(g))


def test_one_float32_ulp_across_the_cutoff():
    """a ligand atom off the lattice and pocket atoms at distance 4 in seeded directions, each twice: the float32 x on either side of the
    cutoff.  The model's d2 (three differences, three products, two sums, each rounded once) is asserted to straddle 16, here on the CPU"""
    rng = np.random.default_rng(5)
    lig = np.array([1.5625, -2.28125, 0.71875], np.float32)
    rec = []
    for _ in range(48):
        u = rng.normal(size=3)
        u[0] = abs(u[0]) + 0.2                                                 # x grows with the distance
        v = (lig.astype(np.float64) + 4.0 * u / np.linalg.norm(u)).astype(np.float32)
        while NM.dist2(v, lig) <= 16.0:
            v[0] = np.nextafter(v[0], np.float32(np.inf))
        while NM.dist2(v, lig) > 16.0:
            v[0] = np.nextafter(v[0], np.float32(-np.inf))
        beyond = v.copy()
        beyond[0] = np.nextafter(v[0], np.float32(np.inf))
        assert NM.dist2(v, lig) <= 16.0 < NM.dist2(beyond, lig) and beyond[0] - v[0] <= 2.0 ** -21
        rec += [v, beyond]
    rec += [lig + np.array([4, 0, 0], np.float32), lig + np.array([0, -4, 0], np.float32)]       # exactly 16
    assert all(float(NM.dist2(r, lig)) == 16.0 for r in rec[-2:])
    args = ([lig], [6], [0, 1], np.stack(rec), [6] * len(rec), [0, len(rec)])
    want = NM.pocket_contacts(*args, 1)
    assert want[0].tolist() == [1, 0] * 48 + [1, 1]
    same(run_contacts(*args), want)
    # the cutoff is an argument: the same atoms one float64 ulp below 16
    below = np.nextafter(16.0, 0.0)
    want = NM.pocket_contacts(*args, 1, cutoff2=below)
    assert want[0][-2:].tolist() == [0, 0]
    same(run_contacts(*args, cutoff2=below), want)


def test_a_ligand_over_the_limit_is_refused_before_the_launch():
    rng = np.random.default_rng(6)
    with pytest.raises(ValueError, match="1025 ligand atoms, more than the 1024"):
        run_contacts(*collate([graph(rng, 3, 5), graph(rng, 1025, 5)]))


# ---- the comparison -------------------------------------------------------------------------------------------------------------------------
def compare_case(rng, sizes, rec_sizes, nat_fp_status=None):
    """-> the fourteen arrays of the model for groups of ``sizes`` samples whose pockets have ``rec_sizes`` atoms, and group_ptr"""
    P, B = len(sizes), int(sum(sizes))
    group = np.repeat(np.arange(P), sizes)
    pool = np.stack([words(rng.choice(1024, int(rng.integers(0, 60)), replace=False)) for _ in range(12)])

    def side(n, rec_len, mismatch):
        fp = pool[rng.integers(0, 12, n)]
        h = rng.choice(np.array([3, 2 ** 63 + 5, 2 ** 64 - 1], np.uint64), n)
        st = np.where(rng.random(n) < 0.15, rng.choice([1, 4, 8, 16], n), 0).astype(np.int32)
        lens = np.array([rec_len[k] + (int(rng.integers(1, 3)) if mismatch and rng.random() < 0.1 else 0) for k in range(n)])
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        con = (rng.random(int(ptr[-1])) < 0.3).astype(np.uint8) * rng.choice(np.array([1, 1, 7], np.uint8), int(ptr[-1]))
        cs = np.where(rng.random(n) < 0.1, NM.EMPTY, 0).astype(np.int32)
        cen = rng.normal(size=(n, 3)) * 3
        cen[cs != 0] = np.nan
        return [fp, h, st, con, ptr, cen, cs]
    mine = side(B, [rec_sizes[p] for p in group], True)
    theirs = side(P, rec_sizes, False)
    if nat_fp_status is not None:
        theirs[2] = np.asarray(nat_fp_status, np.int32)
    return mine + theirs + [np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)]


def run_compare(args):
    """the entry on 0xFF outputs with guard tails -> (sample_out [B, 6], centroid_d2 [B], group_out [P, 9]); rows the kernel does not
    write read -1 (the float: that bit pattern), which is what the model leaves there"""
    B, P = len(args[1]), len(args[8])
    dts = [np.int32, np.int64, np.int32, np.uint8, np.int32, np.float64, np.int32]
    dev = [_dev(np.asarray(a).view(np.int32) if k % 7 == 0 else (np.asarray(a).view(np.int64) if k % 7 == 1 else a), dts[k % 7])
           for k, a in enumerate(args[:14])]
    gp = _dev(args[14], np.int32)
    out, d2, grp = _ff(NM.SAMPLE_COLS * B + GUARD, torch.int64), _ff(B + GUARD, torch.float64), _ff(NM.GROUP_COLS * P + GUARD, torch.int64)
    p = _native.ptr
    some = lambda t: p(t) if t.numel() else None
    a = [p(t) if k % 7 == 4 else some(t) for k, t in enumerate(dev)]
    _native.check(_native.lib().cbgx_native_compare(*a[:7], B, len(args[3]), *a[7:], P, len(args[10]), p(gp), p(out), p(d2), p(grp),
                                                    _native.current_stream(DEV)), "cbgx_native_compare")
    torch.cuda.synchronize()
    out, d2, grp = out.cpu().numpy(), d2.cpu().numpy(), grp.cpu().numpy()
    assert (out[NM.SAMPLE_COLS * B:] == -1).all() and (d2[B:].view(np.int64) == -1).all() and (grp[NM.GROUP_COLS * P:] == -1).all()
    return out[:NM.SAMPLE_COLS * B].reshape(B, NM.SAMPLE_COLS), d2[:B], grp[:NM.GROUP_COLS * P].reshape(P, NM.GROUP_COLS)


def same_compare(got, want):
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:10].tolist()
    assert np.array_equal(got[1].view(np.int64) == -1, want[1].view(np.int64) == -1) and NM.same_floats(got[1], want[1])
    assert np.array_equal(got[2], want[2]), np.argwhere(got[2] != want[2])[:10].tolist()


def test_groups_of_every_size_natives_not_evaluated_and_mismatched_pockets():
    rng = np.random.default_rng(77)
    args = compare_case(rng, [0, 1, 2, 65, 1025, 3, 0], [5, 0, 1, 63, 65, 130, 7], nat_fp_status=[0, 0, 0, 0, 0, 8, 1])
    want = NM.native_compare(*args)
    st = want[0][:, 5]
    assert all(((st & bit) != 0).any() for bit in (NM.SAMPLE_NOT_EVALUATED, NM.NATIVE_NOT_EVALUATED, NM.POCKET_MISMATCH)) and (st == 0).sum() > 500
    assert np.isnan(want[1]).any() and (want[1] > 0).any() and want[2][:, 0].tolist() == [0, 1, 2, 65, 1025, 3, 0]
    assert want[2][4, 2] > 0 and want[2][4, 4] == 1000000 and (want[0][:, 4] > 0).any()
    same_compare(run_compare(args), want)
    # one sample and one native, nothing at all in their pockets
    args = compare_case(rng, [1], [0])
    same_compare(run_compare(args), NM.native_compare(*args))


def test_malformed_group_ptr_between_guard_tails():
    rng = np.random.default_rng(78)
    args = compare_case(rng, [3, 3, 3], [4, 9, 2])
    for group_ptr in ([-5, 3, 5, 4], [0, 2, 9 + 9, 9], [2 ** 31 - 1, -2 ** 31, 4, 4], [9, 9, 9, 0], [2, 1, 9, 9]):
        bad = args[:14] + [np.asarray(group_ptr, np.int32)]
        want = NM.native_compare(*bad)
        assert (want[2][:, 8] & NM.BAD_GROUPS).any()
        same_compare(run_compare(bad), want)
    # (a group reads its own native whatever samples it is handed: pockets of another length are reported, not read past)
    assert (NM.native_compare(*args[:14], np.asarray([-5, 3, 5, 4], np.int32))[0][:, 5] & NM.POCKET_MISMATCH).any()


# ---- argument checks on the device ---------------------------------------------------------------------------------------------------------
def test_null_and_host_memory_arguments():
    lib, p = _native.lib(), _native.ptr
    rng = np.random.default_rng(9)
    graphs = [graph(rng, 5, 9), graph(rng, 7, 11)]
    xl, zl, lp, xr, zr, rp = collate(graphs)
    dev = {"x_lig": _dev(xl, np.float32), "z_lig": _dev(zl, np.uint8), "lig_ptr": _dev(lp, np.int32), "x_rec": _dev(xr, np.float32),
           "z_rec": _dev(zr, np.uint8), "rec_ptr": _dev(rp, np.int32), "rec_contact": _ff(20 + GUARD, torch.uint8),
           "lig_contact": _ff(12 + GUARD, torch.uint8), "centroid": _ff(6 + GUARD, torch.float64), "graph_out": _ff(12 + GUARD, torch.int32)}
    host = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in dev.items()}
    outs = ("rec_contact", "lig_contact", "centroid", "graph_out")

    def call(B=2, **swap):
        a = {k: swap[k] if k in swap else p(dev[k]) for k in dev}
        return lib.cbgx_pocket_contacts(a["x_lig"], a["z_lig"], a["lig_ptr"], 12, a["x_rec"], a["z_rec"], a["rec_ptr"], 20, B, 16.0,
                                        a["rec_contact"], a["lig_contact"], a["centroid"], a["graph_out"], _native.current_stream(DEV))

    def untouched(d=dev, names=outs):
        torch.cuda.synchronize()
        return all(bool((d[k].view(torch.uint8) == 255).all()) for k in names)

    assert call(B=0) == 0 and untouched()
    for k in dev:
        assert call(**{k: None}) == -1 and b"NULL" in lib.cbgx_last_error() and untouched(), k
    for k in dev:                                                                # plain host memory: refused before any launch, by name
        assert call(**{k: ctypes.c_void_p(host[k].ctypes.data)}) == -1, k
        assert f"{k} is not memory the device can read" in lib.cbgx_last_error().decode() and untouched(), k
    assert call() == 0
    torch.cuda.synchronize()
    want = NM.pocket_contacts(xl, zl, lp, xr, zr, rp, 2)
    assert np.array_equal(dev["rec_contact"].cpu().numpy()[:20], want[0]) and np.array_equal(dev["graph_out"].cpu().numpy()[:12].reshape(2, 6), want[3])

    args = compare_case(rng, [2], [20])
    args[3], args[4] = want[0].copy(), rp.copy()                                  # the two samples' contacts from above: 9 and 11 atoms
    side = ("fp", "mol_hash", "fp_status", "rec_contact", "rec_ptr", "centroid", "contacts_status")
    names = side + tuple(k + "_nat" for k in side) + ("group_ptr",)
    dts = [np.int32, np.int64, np.int32, np.uint8, np.int32, np.float64, np.int32]
    view = lambda k, a: np.asarray(a).view(np.int32) if k % 7 == 0 else (np.asarray(a).view(np.int64) if k % 7 == 1 else a)
    cdev = {n: _dev(view(k, a), (dts * 2 + [np.int32])[k]) for k, (n, a) in enumerate(zip(names, args))}
    cdev.update(sample_out=_ff(12 + GUARD, torch.int64), centroid_d2=_ff(2 + GUARD, torch.float64), group_out=_ff(9 + GUARD, torch.int64))
    chost = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in cdev.items()}
    couts = ("sample_out", "centroid_d2", "group_out")

    def ccall(P=1, **swap):
        a = {k: swap[k] if k in swap else p(cdev[k]) for k in cdev}
        return lib.cbgx_native_compare(*[a[k] for k in side], 2, 20, *[a[k + "_nat"] for k in side], P, 20, a["group_ptr"], a["sample_out"],
                                       a["centroid_d2"], a["group_out"], _native.current_stream(DEV))

    assert ccall(P=0) == 0 and untouched(cdev, couts)
    for k in cdev:
        assert ccall(**{k: None}) == -1 and b"NULL" in lib.cbgx_last_error() and untouched(cdev, couts), k
    assert chost["fp"].ctypes.data % 16 == 0 and chost["fp_nat"].ctypes.data % 16 == 0
    for k in cdev:
        assert ccall(**{k: ctypes.c_void_p(chost[k].ctypes.data)}) == -1, k
        assert f"{k} is not memory the device can read" in lib.cbgx_last_error().decode() and untouched(cdev, couts), k
    assert ccall() == 0
    torch.cuda.synchronize()
    cwant = NM.native_compare(*args)
    assert np.array_equal(cdev["sample_out"].cpu().numpy()[:12].reshape(2, 6), cwant[0])
    assert (cwant[0][:, 5] & NM.POCKET_MISMATCH).all()                           # 9 and 11 atoms against the native's 20


# ---- through the Python layers ----------------------------------------------------------------------------------------------------------------
def toluene_like(centre):
    """a benzene ring with a methyl carbon and a hydroxyl oxygen in 'add_aromatic' type indices (2: aromatic C, 1: C, 5: O)"""
    ang = np.arange(6) * np.pi / 3
    ring = np.stack([1.40 * np.cos(ang), 1.40 * np.sin(ang), np.zeros(6)], 1)
    pos = np.concatenate([ring, [[2.91, 0, 0]], [[-2.76, 0, 0]]]) + np.asarray(centre)
    return pos.astype(np.float32), np.array([2] * 6 + [1, 5], np.int64)


def test_a_native_ligand_as_a_sample_of_its_own_pocket():
    """two pockets x three samples; sample 0 of each pocket is its native ligand's atoms, sample 1 those shifted by 30 A, sample 2 the
    batch's priors.  Every shared report field of native and sample 0 is equal, and the comparison says so"""
    from cbgbench_amd import sample_cli
    rng = np.random.default_rng(11)
    pockets = [synthetic.make_pocket(rng, n) for n in (140, 170)]
    batch = sample_cli.build_pocket_batch(pockets, 3, np.random.default_rng(1), 13, device=DEV)
    ligands = [toluene_like(p[0][np.argmin(np.linalg.norm(p[0], axis=1))] + 1.9) for p in pockets]
    ligands[1] = (ligands[1][0][:7], ligands[1][1][:7])
    group_ptr = [0, 3, 6]
    native = SampleReports.native_state(batch, group_ptr, ligands)
    assert native["lig_batch"].tolist() == [0] * 8 + [1] * 7 and native["batch"]["protein_element_batch"].tolist() == [0] * 140 + [1] * 170
    shift = batch["ligand_translation"][batch["ligand_element_batch"] == 3][0].cpu()
    assert torch.equal(native["x"][8:].cpu(), torch.from_numpy(ligands[1][0]) - shift)
    xs, cs, bs = [], [], []
    prior_c = batch["ligand_atom_type"].argmax(-1) if batch["ligand_atom_type"].dim() == 2 else batch["ligand_atom_type"]
    for g in range(6):
        nat = native["lig_batch"] == g // 3
        own = batch["ligand_element_batch"] == g
        x, c = (native["x"][nat], native["c"][nat]) if g % 3 < 2 else (batch["ligand_pos"][own], prior_c[own])
        xs.append(x + (30.0 if g % 3 == 1 else 0.0))
        cs.append(c)
        bs.append(torch.full((c.shape[0],), g, dtype=torch.long, device=DEV))
    state = (torch.cat(xs), torch.cat(cs), torch.cat(bs))
    requested = ("geometry", "bonds", "rings", "aromatic", "valence", "interactions", "groups", "diversity", "native")
    r = SampleReports(requested)
    ev = r.evaluate(DEV, state, batch, 6, "add_aromatic", group_ptr=group_ptr, native=native)
    assert sorted(ev["native_reports"]) == sorted(requested[:-1]) and r.seconds["native"] > 0.0
    samples = sample_cli.split_samples(state[0].cpu(), state[1].cpu(), state[2].cpu(), 6, "add_aromatic")
    r.annotate(samples, ev)
    natives = r.annotate_native(sample_cli.split_samples(native["x"].cpu(), native["c"].cpu(), native["lig_batch"].cpu(), 2, "add_aromatic"), ev)
    for p, nat in enumerate(natives):
        smp, far = samples[3 * p], samples[3 * p + 1]
        shared = sorted(set(nat) & set(smp))
        assert len(shared) >= 60 and {"score", "fingerprint", "mol_hash", "formula", "ring_sizes", "n_aromatic_rings", "atom_terms"} <= set(shared)
        differ = [k for k in shared if k not in ("duplicate_of", "nearest_sample", "nearest_similarity") and not
                  (_equal(nat[k], smp[k]) or (isinstance(nat[k], float) and math.isnan(nat[k]) and math.isnan(smp[k])))]
        assert differ == [], differ
        assert nat["score_micro"] == G.score_micro(nat["score"]) and nat["n_pocket_contact_atoms"] > 0 and nat["interactions_status"] == 0
        assert (smp["native_similarity"], smp["native_same_hash"], smp["native_contact_jaccard"], smp["native_centroid_distance"],
                smp["score_minus_native"], smp["better_than_native"], smp["native_status"]) == (1.0, True, 1.0, 0.0, 0.0, False, 0)
        assert smp["native_contact_common"] == smp["native_contact_union"] == nat["n_pocket_contact_atoms"]
        assert smp["ligand_efficiency"] == nat["score_micro"] / 1e6 / (8, 7)[p]
        assert (far["native_similarity"], far["native_same_hash"], far["native_contact_common"], far["native_contact_union"]) == \
            (1.0, True, 0, nat["n_pocket_contact_atoms"])
        assert far["native_contact_jaccard"] == 0.0 and abs(far["native_centroid_distance"] - 30 * math.sqrt(3)) < 1e-4
        assert sorted(set(smp) - set(nat)) == sorted(NATIVE_FIELDS)
        rec = r.pocket_counts(ev, 3 * p, 3 * p + 3)["native_comparison"]
        assert rec["n_mol"] == 3 and rec["n_same_hash"] >= 2 and rec["native_score_micro"] == nat["score_micro"] and rec["sim_micro_max"] == 1000000
    # the Python entries on tensors: the model on what they were handed
    nat = ev["native"]
    lig_b = state[2]
    z = torch.tensor(C.config._ATOMIC_NUMBER["add_aromatic"], device=DEV)[state[1]]
    con = G.pocket_contacts(state[0], z, lig_b, batch["protein_pos"], batch["protein_element"], batch["protein_element_batch"], 6)
    lig_ptr = np.concatenate([[0], np.cumsum(np.bincount(lig_b.cpu().numpy(), minlength=6))])
    want = NM.pocket_contacts(state[0].cpu().numpy(), z.cpu().numpy(), lig_ptr, batch["protein_pos"].cpu().numpy(),
                              batch["protein_element"].cpu().numpy(), con["rec_ptr"].cpu().numpy(), 6)
    same(tuple(con[k].cpu().numpy() for k in ("rec_contact", "lig_contact", "centroid", "graph_counts")), want)
    assert torch.equal(con["rec_contact"].cpu(), nat["rec_contact"]) and NM.same_floats(con["centroid"].cpu().numpy(), nat["centroid"].numpy())


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
def _records(out_dir, n):
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".pt"))
    assert files == [f"pocket_{i:05d}.pt" for i in range(n)]
    return [torch.load(os.path.join(out_dir, f), map_location="cpu", weights_only=False) for f in files]


def _same_field(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same_field(a[k], b[k]) for k in a)
    if torch.is_tensor(a) and torch.is_tensor(b) and a.is_floating_point():       # (a sample that was not evaluated carries nan terms)
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())
    return _equal(a, b) or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_sample_cli_native(tmp_path, capsys):
    """the T = 20 fixture config, a pockets file of three small synthetic pockets with native ligands x four samples, --noise counter,
    one saved random checkpoint: one pocket per batch and three give the same `native`, `native_comparison` and per-sample native fields
    and the same summary file, which is summarise_native of the records; with other flags added their fields and files are what they
    are without --native; without the flag none of the new keys is written"""
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    config, _ = C.load_config(cfg)
    C.set_num_atom_type(config)
    torch.manual_seed(123)
    ckpt = tmp_path / "random_init.pt"
    torch.save({"model": C.get_model(config.model).state_dict()}, ckpt)
    rng = np.random.default_rng(2)
    raw = []
    for n in (120, 150, 135):
        pos, feat, aa = synthetic.make_pocket(rng, n)
        lig = toluene_like(pos[np.argmin(np.linalg.norm(pos, axis=1))] + 1.9)
        raw.append({"protein_pos": pos, "protein_atom_feature": feat, "protein_aa_type": aa, "ligand_pos": lig[0].astype(np.float64),
                    "ligand_atom_type": lig[1]})
    pockets = tmp_path / "pockets.pt"
    torch.save(raw, pockets)
    tail = ["--pockets", str(pockets), "--num_samples", "4", "--seed", "2024", "--noise", "counter", "--checkpoint", str(ckpt), "--streams", "1"]

    def go(tag, *extra):
        out, stats = tmp_path / tag, {}
        assert sample_cli.main(["--config", cfg, *tail, "--out_root", str(out)] + list(extra), stats=stats) == 0
        d = str(out / os.path.splitext(os.path.basename(cfg))[0])
        return d, _records(d, 3), stats

    others = ("--interactions", "--diversity", "--rings")
    dir_base, base, stats_base = go("base", "--pockets_per_batch", "3", *others)
    dir_one, one, stats_one = go("one", "--pockets_per_batch", "1", "--native", *others)
    dir_all, whole, stats_all = go("all", "--pockets_per_batch", "3", "--native", *others)
    dir_only, only, stats_only = go("only", "--pockets_per_batch", "3", "--native")
    printed = capsys.readouterr().out
    assert printed.count("native: improved_mol_ratio") == 3 and "not the Vina program" in printed and "not RDKit's" in printed
    assert stats_one["native"] > 0.0 and stats_all["native"] > 0.0 and "native" not in stats_base
    assert sorted(k for k in stats_only if k in ("bonds", "rings", "aromatic", "valence", "interactions", "diversity", "native")) == ["native"]

    # with the other flags their fields and files are what they are without --native
    assert not os.path.exists(os.path.join(dir_base, "native_summary.json"))
    assert sorted(os.listdir(dir_all)) == sorted(os.listdir(dir_base) + ["native_summary.json"])
    for name in os.listdir(dir_base):
        if name.endswith(".json"):
            assert open(os.path.join(dir_base, name)).read() == open(os.path.join(dir_all, name)).read(), name
    for r, r2 in zip(base, whole):
        assert sorted(set(r2) - set(r)) == ["native", "native_comparison"] and all(_same_field(r[k], r2[k]) for k in r if k != "samples")
        for s, s2 in zip(r["samples"], r2["samples"]):
            assert sorted(set(s2) - set(s)) == sorted(NATIVE_FIELDS)
            assert all(_same_field(s[k], s2[k]) for k in s), [k for k in s if not _same_field(s[k], s2[k])]

    # one pocket per batch or three: the same records; the native record is a function of the pocket alone, in the caller's frame
    for p, (ra, rb, ro) in enumerate(zip(one, whole, only)):
        assert _same_field(ra["native"], rb["native"]) and ra["native_comparison"] == rb["native_comparison"] == ro["native_comparison"]
        assert tuple(rb["native_comparison"]) == G.NATIVE_POCKET_KEYS and rb["native_comparison"]["n_mol"] == 4
        for sa, sb, so in zip(ra["samples"], rb["samples"], ro["samples"]):
            assert sorted(sa) == sorted(sb) and all(_same_field(sa[k], sb[k]) for k in sa), [k for k in sa if not _same_field(sa[k], sb[k])]
            assert all(_same_field(so[k], sb[k]) for k in so) and set(NATIVE_FIELDS) <= set(so)
        nat = rb["native"]
        assert torch.equal(nat["pos"], torch.from_numpy(raw[p]["ligand_pos"].astype(np.float32))) and nat["type"].tolist() == raw[p]["ligand_atom_type"].tolist()
        assert nat["score_micro"] == rb["native_comparison"]["native_score_micro"] and nat["n_pocket_contact_atoms"] > 0
        assert {"score", "fingerprint", "ring_sizes", "interactions_status"} <= set(nat) and set(ro["native"]) < set(nat)
        assert sorted(ro["native"]) == sorted(["pos", "type", "atom_type", "atom", "aromatic", "type_vector", "score", "score_micro", "n_contact_atoms", "n_pocket_contact_atoms"])
        for s in rb["samples"]:
            assert s["native_status"] in (0, NM.SAMPLE_NOT_EVALUATED) and s["native_contact_union"] >= nat["n_pocket_contact_atoms"]
            assert 0.0 <= s["native_similarity"] <= 1.0 if s["native_status"] == 0 else math.isnan(s["native_similarity"])
            if s["interactions_status"] == 0:
                assert s["better_than_native"] == (G.score_micro(s["score"]) < nat["score_micro"])
                assert s["score_minus_native"] == (G.score_micro(s["score"]) - nat["score_micro"]) / 1e6
            else:
                assert s["better_than_native"] is None and math.isnan(s["score_minus_native"])
    want = G.summarise_native([r["native_comparison"] for r in whole])
    texts = [open(os.path.join(d, "native_summary.json")).read() for d in (dir_one, dir_all, dir_only)]
    assert texts[0] == texts[1] == texts[2] == json.dumps(want, indent=1, sort_keys=True)
    assert want["counts"]["n_pockets"] == 3 and want["counts"]["n_mol"] == 12
