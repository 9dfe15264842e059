"""Integer-lattice batches for the inference forward: inputs on which equal squared distances are the rule, not an accident.

Protein atoms sit on a random half of the sites of a cubic lattice of spacing 1.5, ligand atoms on distinct sites of a lattice of
spacing 0.75 around the pocket's centre (every second site of it is a protein site, so some ligand atoms coincide with a protein
atom).  All coordinates are multiples of 0.75 below 2^7, their differences and the sums of three squared differences are exact in
fp32, so d2 is the same number however it is evaluated and a tie is a tie on every path.  Nothing is centred.  Rows are in the
composed order of the samplers: per graph the protein rows, then the ligand rows.

tests/test_lattice_inputs.py pins, with the oracle's knn_graph, that these batches hold the ties and list sizes the GPU tests of
tests/test_gpu_forward_lists.py rely on.  Everything here is numpy / CPU torch and deterministic in its seed."""
import numpy as np
import torch

from oracle import unitransformer as OU

K = 32
# (protein, ligand) sizes: a pocket below the neighbour count, more ligand than pocket atoms, the ligand counts around the rank-counting
# merge's second candidate register (63 / 64 / 65) and its hand-over to the scan (127 / 128), graph totals around the small register-cached
# kNN size (512 / 513) and the large one (768 / 769), a graph that takes the rescanning search, a ligand-free and a pocket-free graph
SMALL_SIZES = [(20, 5), (33, 40), (300, 63), (300, 64), (300, 65), (300, 127), (260, 128), (512 - 12, 12), (513 - 12, 12),
               (768 - 8, 8), (769 - 8, 8), (900, 12), (400, 0), (0, 6)]
SMALL_NODES = sum(p + l for p, l in SMALL_SIZES)      # 5885
LIST_REGIME_MAX = 8192       # kernels.h GRAPH_LISTS_MAX_NODES = NODE_STAGE_MAX_ROWS: the last input of the per-graph list kernel
_PAD = [(700, 20), (700, 20), (600, 30)]
SEEDS = {"small": 20261, "context": 20262, "at_threshold": 20263, "above_threshold": 20264, "large": 20265}


def _sizes(name):
    if name in ("small", "context"):
        return list(SMALL_SIZES)
    if name in ("at_threshold", "above_threshold"):
        total = LIST_REGIME_MAX + (name == "above_threshold")
        rest = total - SMALL_NODES - sum(p + l for p, l in _PAD)
        return SMALL_SIZES + _PAD + [(rest - 7, 7)]
    if name == "large":          # just above the threshold with other graphs than the padded copy: two more rescanning pockets
        return SMALL_SIZES + [(900, 12), (800, 70), (790, 8)]
    raise KeyError(name)


def _cube(n_sites, spacing):
    """the sites of the smallest cube of a cubic lattice that has at least n_sites sites, centred on a lattice site or cell"""
    m = 1
    while m ** 3 < n_sites:
        m += 1
    g = np.arange(m) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), m


def lattice_graph(rng, n_rec, n_lig):
    """-> (protein positions [n_rec,3], ligand positions [n_lig,3]) float32, exact multiples of 0.75"""
    origin = 0.75 * rng.integers(-8, 9, size=3)          # not centred: the pocket's corner anywhere within +-6
    sites, m = _cube(2 * max(n_rec, 1), 1.5)
    rec = sites[rng.choice(sites.shape[0], size=n_rec, replace=False)] + origin
    lsites, lm = _cube(2 * max(n_lig, 1), 0.75)
    # the ligand's cube around the pocket cube's centre, snapped to the fine lattice
    corner = origin + 0.75 * np.round((1.5 * (m - 1) / 2 - 0.75 * (lm - 1) / 2) / 0.75)
    lig = lsites[rng.choice(lsites.shape[0], size=n_lig, replace=False)] + corner
    return rec.astype(np.float32), lig.astype(np.float32)


def make(name):
    """the batch `name` of SEEDS -> dict of CPU tensors: x [N,3], batch_idx, graph_ptr (int32), lig_flag, gen_flag (bool), sizes, and what
    the model's embedders take: protein_feat [n_rec,7], protein_aa [n_rec], ligand_type [n_lig]"""
    rng = np.random.default_rng(SEEDS[name])
    sizes = _sizes(name)
    xs, lig, gen, bidx = [], [], [], []
    for g, (n_rec, n_lig) in enumerate(sizes):
        rec, lg = lattice_graph(rng, n_rec, n_lig)
        xs += [rec, lg]
        lig.append(np.concatenate([np.zeros(n_rec, bool), np.ones(n_lig, bool)]))
        gl = np.ones(n_lig, bool)
        if name == "context":
            gl[rng.integers(0, 3)::3] = False           # fixed context atoms interleaved with the generated ones
        gen.append(np.concatenate([np.zeros(n_rec, bool), gl]))
        bidx.append(np.full(n_rec + n_lig, g, np.int64))
    lig, gen = np.concatenate(lig), np.concatenate(gen)
    n_rec_all, n_lig_all = int((~lig).sum()), int(lig.sum())
    elem = rng.choice(6, size=n_rec_all, p=[0.0, 0.62, 0.17, 0.19, 0.02, 0.0])
    feat = np.zeros((n_rec_all, 7), np.float32)
    feat[np.arange(n_rec_all), elem] = 1.0
    feat[:, 6] = rng.random(n_rec_all) < 0.45
    counts = np.array([p + l for p, l in sizes])
    return {"name": name, "sizes": sizes, "x": torch.from_numpy(np.concatenate(xs)), "batch_idx": torch.from_numpy(np.concatenate(bidx)),
            "graph_ptr": torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)),
            "lig_flag": torch.from_numpy(lig), "gen_flag": torch.from_numpy(gen), "protein_feat": torch.from_numpy(feat),
            "protein_aa": torch.from_numpy(rng.integers(0, 20, size=n_rec_all).astype(np.int64)),
            "ligand_type": torch.from_numpy(rng.integers(0, 13, size=n_lig_all).astype(np.int64))}


_CACHE = {}


def batch(name):
    """`make(name)` once per process (the tests share it and leave it unchanged)"""
    if name not in _CACHE:
        _CACHE[name] = make(name)
    return _CACHE[name]


# ---- the reference graph and the list definitions (include/cbgx.h, csrc/api.hip forward_impl), in numpy from the oracle's edge list ----
def _d2(x, i, j):
    d = x[i] - x[j]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]        # the oracle's expression, fp32


def reference(b):
    """-> dict: nbr [N,32] (-1 padded), deg [N], edge_index (oracle), and per centre d2 of its neighbours in rank order (inf padded)"""
    key = ("ref", b["name"])
    if key in _CACHE:
        return _CACHE[key]
    x, N = b["x"], b["x"].shape[0]
    ei = OU.knn_graph(x, b["batch_idx"], K)
    src, dst = ei[0].numpy(), ei[1].numpy()
    deg = np.bincount(dst, minlength=N).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(deg)])[:-1]
    slot = np.arange(src.shape[0]) - start[dst]
    nbr = np.full((N, K), -1, np.int32)
    nbr[dst, slot] = src
    d2 = np.full((N, K), np.inf, np.float32)
    d2[dst, slot] = _d2(x.numpy(), dst, src)
    _CACHE[key] = {"nbr": nbr, "deg": deg, "edge_index": ei, "d2": d2}
    return _CACHE[key]


def _in_nbrs(nbr, members):
    """nbr(set): the in-neighbours of its members (the sources their edges read), as a boolean mask"""
    out = np.zeros(nbr.shape[0], bool)
    j = nbr[members]
    out[j[j >= 0]] = True
    return out


def _meets(nbr, flags):
    """{i : nbr(i) meets the flagged set}"""
    return (flags[np.clip(nbr, 0, None)] & (nbr >= 0)).any(1)


def list_definitions(b, prune=True, cached=True):
    """every node list of a forward call as a sorted int array, from its definition on the oracle's graph; a list the call does not
    build (see include/cbgx_xcheck.h) is empty"""
    nbr = reference(b)["nbr"]
    lig, gen = b["lig_flag"].numpy(), b["gen_flag"].numpy()
    N = nbr.shape[0]
    a1 = gen | lig | _in_nbrs(nbr, gen)
    a2 = a1 | _in_nbrs(nbr, a1)
    a3 = a2 | _in_nbrs(nbr, a2)
    d1 = lig | _meets(nbr, lig)
    D2 = d1 | _meets(nbr, d1)
    S1 = d1 | _in_nbrs(nbr, d1)
    S2 = D2 | _in_nbrs(nbr, D2)
    none, every = np.zeros(N, bool), np.ones(N, bool)
    sets = {"act": gen, "A1": a1, "A2": a2 if prune else none, "A3": a3 if prune else none,
            "D1": d1 if cached else none, "S1": S1 if cached else none, "D2": D2 if cached else none, "S2": S2 if cached else none}
    for name, s in (("all", every), ("D2", D2 if cached else none), ("A1", a1 if prune else none), ("A2", a2 if prune else none)):
        sets[name + "_general"] = s & d1
        sets[name + "_protein"] = s & ~d1
    out = {k: np.nonzero(v)[0].astype(np.int32) for k, v in sets.items()}
    out["d1flag"] = d1.astype(np.uint8)
    return out


def tie_report(b):
    """per graph what the inputs are for -> list of dicts (tests/test_lattice_inputs.py asserts on them)"""
    ref = reference(b)
    x = b["x"].numpy()
    lig = b["lig_flag"].numpy()
    gp = b["graph_ptr"].numpy()
    rep = []
    for g, (n_rec, n_lig) in enumerate(b["sizes"]):
        s, e = int(gp[g]), int(gp[g + 1])
        n = e - s
        r = {"graph": g, "n": n, "n_rec": n_rec, "n_lig": n_lig, "ties_32_33": 0, "ties_32_33_mixed": 0, "ligand_at_cached_32nd": 0,
             "coincident": 0}
        p = x[s:e]
        d = p[:, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        np.fill_diagonal(d2, np.inf)
        r["coincident"] = int((d2 == 0).sum() // 2)
        if n > K + 1:
            order = np.argsort(d2, axis=1, kind="stable")
            i = np.arange(n)
            a, c = order[:, K - 1], order[:, K]
            tie = d2[i, a] == d2[i, c]
            r["ties_32_33"] = int(tie.sum())
            r["ties_32_33_mixed"] = int((tie & (lig[s + a] != lig[s + c])).sum())
        if n_rec > K and n_lig > 0:
            # the pocket's own 32nd distance (what the static context caches) against the nearest ligand atom
            pp = d2[:n_rec, :n_rec]
            r32 = np.sort(pp, axis=1)[:, K - 1]
            near = d2[:n_rec, n_rec:].min(1)
            r["ligand_at_cached_32nd"] = int((near == r32).sum())
        rep.append(r)
    return rep
