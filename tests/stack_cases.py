"""Case builder, float64 oracle and seed table of tests/test_gpu_stack_backward.py (the whole training backward, cbgx_unitransformer_backward_ex,
through the public module); tests/test_stack_cases.py re-derives every precondition stated here without a GPU.

A case is a StackKey: family, n (rows), L (layers), C (classes), mode ("lo" = ligand_outputs_only, "full", "src" = h_on_sources),
R (hot rows), g (generated atoms among them), variant ("" | "edge_rows" | "dense" = CBGX_TRAIN_PRUNE_GH=0), loss (which outputs the
score reads: any of "x", "l", "h").

Batch: graph_sizes and the x / h generator of tests/test_gpu_backward_boundaries.py (graphs of at most 600 nodes, then a 1-node graph,
then a 6-node graph last).  The R hot rows are the last row (6-node graph), the 1-node graph's row, row 0, and rows drawn from the
FIRST graph (from every graph once R > 65): with gen_flag = g of them and lig_flag = exactly the hot rows ("lo", "src"), the lists
of the backward have exactly the sizes  A1 = head list = R,  A2 = A1 + nbr(A1),  h2x work list = g.  The score's weights sit on the hot
rows only (x_out on the gen rows), so graphs without a hot row carry an exactly zero gradient and the oracle evaluates the other graphs
only (graphs do not interact).  "full" in the head and class families: lig_flag is the generator's random 10 % (plus the gen rows), so
the hot rows hold protein rows and the head's list comes from the marked support of grad_logits.

Criterion (no tolerance of its own; gerr of tests/test_gpu_training.py at its defaults, `failures` of tests/test_gpu_coord_grad.py).
STRICT cases -- every case of at most 65 hot rows for which a seed can be found (is_strict: the case has an entry in SEEDS): gerr for
every tensor, under the precondition that no pre-ReLU value lies within FLIP_EPS of zero on a unit that carries gradient
(carrying_near).  In the last layer those units are the key / value MLPs on the edges whose centre is hot (x2h) or generated (h2x) and
the query MLPs on those rows; in every earlier layer all x2h units of the evaluated graphs, and the gate on all their edges.  A value
lies that close to zero with probability 4e-6: one layer and <= 65 hot rows (~2 000 edges x 256 units) are clean on every fourth seed
or so; three layers with a single hot row in the 6-node graph, and two to four layers at 47 nodes, on one seed in 10 - 400.  find_seed
looks at seeds 0 .. 2 first and searches up to 400 only where their mean count is at most PROBE_MAX = 6 (e^-6 x 400 ~ 1 expected hit).
Where it is larger no seed can be clean -- a 600-node graph and three layers: 19 000 edges x 512 units x 2 blocks, 120 - 140 values
inside FLIP_EPS on every seed; 47 nodes and 10 layers or more: 30 - 100 -- and the case is NOT strict: gerr for every tensor still,
against the oracle with ONE verified ReLU flip applied (select_flips names the flipped units from the LayerNorm-bias gradient of their
MLP, which a flip changes by exactly dL/d relu(y) of that unit; the oracle with ONE of them forced to the other side must reproduce
every tensor element-wise).  With ~130 units inside FLIP_EPS two can flip in one run, each visible element-wise in its own MLP's
tensors, which no single flip reproduces (2 cases on the MI355X, named in the GPU file's docstring): then the whole named set, forced
together in one oracle run, must reproduce every tensor element-wise.  Flips are confined to units inside FLIP_EPS: a lost or doubled
row is not among the things they can explain.
More than 65 hot rows (2048 / 2049): `failures` (relative L2 2e-4 for x / h, 1e-3 for parameters) plus the row-wise bound
row_failures.  The one-layer head cases: ONE verified flip.  The three-layer list cases: ONE flip, else the SET of flips select_flips
names, verified together in one oracle run -- each unit lies inside FLIP_EPS (it comes from relu_margins), and the oracle finds ~490 such units there, 21
of which move a tensor of their MLP past 1e-3 on their own; on the GPU two of those flipped at once (blocks.2 hk_func edge 28715 unit
103 and an hq_func row: hk tensors 1.1e-3 - 1.8e-3, hq tensors 1.7e-3 - 2.2e-3 off, every other tensor below 1.2e-4; the oracle's own
fp32 run is 1.6e-3 off), which no single flip explains.  The number of flips used is printed."""
import collections
import contextlib
import functools
import inspect
import math

import torch
import torch.nn.functional as F

from oracle import unitransformer as OU
from oracle import weights as W
from tests.relu_flip import FLIP_EPS, relu_margins
from tests.test_gpu_backward_boundaries import graph_sizes, make_case
from tests.test_gpu_coord_grad import TOL
from tests.test_gpu_training import gerr

StackKey = collections.namedtuple("StackKey", "family n L C mode R g variant loss")
R_SWEEP = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
R_LARGE = (2048, 2049)
GRID_N = (47, 600, 2100)                       # x2h edge grids of 6, 72 and 256 workgroups
DENSE_N = (1, 2, 255, 256, 257, 512, 513, 2048, 2049)
CLASSES = (1, 2, 8, 15, 16, 17, 32, 33, 63, 64, 65, 127, 128)
DEPTHS = (1, 2, 3, 4, 10, 11, 33)
MODES = ("lo", "full", "src")
STRICT_MAX_HOT = 65
DENSE_HOT = 24                                 # hot rows of the dense-head cases (rows 0 and n - 1 among them)


def key_id(k):
    return "-".join(str(v) for v in k if v != "")


def cases_list_vs_grid():
    out = []
    for n in GRID_N:
        # (a list cannot be longer than the batch: at n = 47 the sweep ends with the list that holds every row)
        for R in tuple(r for r in R_SWEEP if r < n) + ((n,) if n < max(R_SWEEP) else ()) + (R_LARGE if n == 2100 else ()):
            for g in (0, 1, 9) if R >= 16 else (0,):
                out.append(StackKey("grid", n, 3, 13, "lo", R, g, "", "xl"))
                if n == 600 and R <= 65:
                    out.append(StackKey("grid", n, 3, 13, "lo", R, g, "edge_rows", "xl"))
    return out


def cases_head_listed():
    out = []
    for mode in ("lo", "full"):
        out += [StackKey("head", 600, 1, 13, mode, R, 0, "", "l") for R in R_SWEEP]
        out += [StackKey("head", 2100, 1, 13, mode, R, 0, "", "l") for R in R_LARGE]
    return out


def cases_head_dense():
    return [StackKey("dense", n, 1, 13, "full", min(n, DENSE_HOT), 0, "dense", "lh") for n in DENSE_N]


def cases_classes():
    out = []
    for C in CLASSES:
        out += [StackKey("classes", 300, 1, C, "lo", 17, 0, "", "l"), StackKey("classes", 300, 1, C, "full", 17, 0, "", "lh"),
                StackKey("classes", 300, 1, C, "full", 17, 0, "dense", "lh")]
    return out


def cases_depth():
    out = []
    for L in DEPTHS:
        for mode in MODES:
            loss = "xl" if mode == "lo" else "xlh"
            out.append(StackKey("depth", 47, L, 13, mode, 9, 3, "", loss))
            if L in (2, 3):
                out.append(StackKey("depth", 47, L, 13, mode, 9, 3, "edge_rows", loss))
    return out


def cases_absent():
    out = []
    for L in (1, 3):
        out += [StackKey("absent", 300, L, 13, "full", 17, 5, "", "x"), StackKey("absent", 300, L, 13, "full", 17, 5, "", "h"),
                StackKey("absent", 300, L, 13, "lo", 0, 0, "", "xl")]
    out.append(StackKey("absent", 300, 1, 13, "full", 17, 5, "", "l"))
    return out


def all_cases():
    return cases_list_vs_grid() + cases_head_listed() + cases_head_dense() + cases_classes() + cases_depth() + cases_absent()


def is_strict(k):
    """gerr without a flip, under the no-near-ReLU precondition: the cases of at most 65 hot rows for which find_seed found a seed"""
    return k.R <= STRICT_MAX_HOT and input_key(k) in SEEDS


# StackKey fields that decide the inputs (family, n, L, C, mode, R, g, loss) -> seed: the first seed >= 0 whose precondition holds
# (find_seed; `python -m tests.stack_cases [family ...]` prints the entries that are missing).  The variant does not change the inputs.
SEEDS = {
    ('head', 600, 1, 13, 'lo', 0, 0, 'l'): 0,
    ('head', 600, 1, 13, 'lo', 1, 0, 'l'): 0,
    ('head', 600, 1, 13, 'lo', 7, 0, 'l'): 0,
    ('head', 600, 1, 13, 'lo', 8, 0, 'l'): 1,
    ('head', 600, 1, 13, 'lo', 9, 0, 'l'): 1,
    ('head', 600, 1, 13, 'lo', 15, 0, 'l'): 2,
    ('head', 600, 1, 13, 'lo', 16, 0, 'l'): 1,
    ('head', 600, 1, 13, 'lo', 17, 0, 'l'): 1,
    ('head', 600, 1, 13, 'lo', 31, 0, 'l'): 1,
    ('head', 600, 1, 13, 'lo', 32, 0, 'l'): 2,
    ('head', 600, 1, 13, 'lo', 33, 0, 'l'): 19,
    ('head', 600, 1, 13, 'lo', 63, 0, 'l'): 38,
    ('head', 600, 1, 13, 'lo', 64, 0, 'l'): 11,
    ('head', 600, 1, 13, 'lo', 65, 0, 'l'): 54,
    ('head', 600, 1, 13, 'full', 0, 0, 'l'): 0,
    ('head', 600, 1, 13, 'full', 1, 0, 'l'): 0,
    ('head', 600, 1, 13, 'full', 7, 0, 'l'): 0,
    ('head', 600, 1, 13, 'full', 8, 0, 'l'): 1,
    ('head', 600, 1, 13, 'full', 9, 0, 'l'): 1,
    ('head', 600, 1, 13, 'full', 15, 0, 'l'): 0,
    ('head', 600, 1, 13, 'full', 16, 0, 'l'): 3,
    ('head', 600, 1, 13, 'full', 17, 0, 'l'): 1,
    ('head', 600, 1, 13, 'full', 31, 0, 'l'): 0,
    ('head', 600, 1, 13, 'full', 32, 0, 'l'): 2,
    ('head', 600, 1, 13, 'full', 33, 0, 'l'): 10,
    ('head', 600, 1, 13, 'full', 63, 0, 'l'): 5,
    ('head', 600, 1, 13, 'full', 64, 0, 'l'): 2,
    ('head', 600, 1, 13, 'full', 65, 0, 'l'): 17,
    ('classes', 300, 1, 1, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 1, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 2, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 2, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 8, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 8, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 15, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 15, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 16, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 16, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 17, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 17, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 32, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 32, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 33, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 33, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 63, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 63, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 64, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 64, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 65, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 65, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 127, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 127, 'full', 17, 0, 'lh'): 0,
    ('classes', 300, 1, 128, 'lo', 17, 0, 'l'): 3,
    ('classes', 300, 1, 128, 'full', 17, 0, 'lh'): 0,
    ('depth', 47, 1, 13, 'lo', 9, 3, 'xl'): 9,
    ('depth', 47, 1, 13, 'full', 9, 3, 'xlh'): 9,
    ('depth', 47, 1, 13, 'src', 9, 3, 'xlh'): 9,
    ('absent', 300, 1, 13, 'full', 17, 5, 'x'): 109,
    ('absent', 300, 1, 13, 'full', 17, 5, 'h'): 3,
    ('absent', 300, 1, 13, 'lo', 0, 0, 'xl'): 0,
    ('absent', 300, 1, 13, 'full', 17, 5, 'l'): 3,
    ('dense', 1, 1, 13, 'full', 1, 0, 'lh'): 0,
    ('dense', 2, 1, 13, 'full', 2, 0, 'lh'): 0,
    ('dense', 255, 1, 13, 'full', 24, 0, 'lh'): 5,
    ('dense', 256, 1, 13, 'full', 24, 0, 'lh'): 2,
    ('dense', 257, 1, 13, 'full', 24, 0, 'lh'): 0,
    ('dense', 512, 1, 13, 'full', 24, 0, 'lh'): 1,
    ('dense', 513, 1, 13, 'full', 24, 0, 'lh'): 0,
    ('dense', 2048, 1, 13, 'full', 24, 0, 'lh'): 0,
    ('dense', 2049, 1, 13, 'full', 24, 0, 'lh'): 2,
    ('grid', 47, 3, 13, 'lo', 0, 0, 'xl'): 0,
    ('grid', 47, 3, 13, 'lo', 1, 0, 'xl'): 1,
    ('grid', 47, 3, 13, 'lo', 7, 0, 'xl'): 9,
    ('grid', 47, 3, 13, 'lo', 8, 0, 'xl'): 17,
    ('grid', 47, 3, 13, 'lo', 9, 0, 'xl'): 22,
    ('grid', 47, 3, 13, 'lo', 15, 0, 'xl'): 4,
    ('grid', 47, 3, 13, 'lo', 16, 0, 'xl'): 30,
    ('grid', 47, 3, 13, 'lo', 16, 1, 'xl'): 30,
    ('grid', 47, 3, 13, 'lo', 16, 9, 'xl'): 134,
    ('grid', 47, 3, 13, 'lo', 17, 0, 'xl'): 26,
    ('grid', 47, 3, 13, 'lo', 17, 1, 'xl'): 26,
    ('grid', 47, 3, 13, 'lo', 31, 0, 'xl'): 38,
    ('grid', 47, 3, 13, 'lo', 31, 1, 'xl'): 38,
    ('grid', 47, 3, 13, 'lo', 32, 0, 'xl'): 116,
    ('grid', 47, 3, 13, 'lo', 32, 1, 'xl'): 116,
    ('grid', 47, 3, 13, 'lo', 33, 0, 'xl'): 22,
    ('grid', 47, 3, 13, 'lo', 33, 1, 'xl'): 22,
    ('grid', 47, 3, 13, 'lo', 33, 9, 'xl'): 22,
    ('grid', 47, 3, 13, 'lo', 47, 0, 'xl'): 67,
    ('grid', 47, 3, 13, 'lo', 47, 1, 'xl'): 67,
    ('grid', 600, 3, 13, 'lo', 0, 0, 'xl'): 0,
    ('grid', 600, 3, 13, 'lo', 1, 0, 'xl'): 0,
    ('grid', 2100, 3, 13, 'lo', 0, 0, 'xl'): 0,
    ('grid', 2100, 3, 13, 'lo', 1, 0, 'xl'): 0,
    ('depth', 47, 2, 13, 'lo', 9, 3, 'xl'): 17,
    ('depth', 47, 2, 13, 'full', 9, 3, 'xlh'): 17,
    ('depth', 47, 2, 13, 'src', 9, 3, 'xlh'): 17,
    ('depth', 47, 3, 13, 'lo', 9, 3, 'xl'): 22,
    ('depth', 47, 3, 13, 'full', 9, 3, 'xlh'): 22,
    ('depth', 47, 3, 13, 'src', 9, 3, 'xlh'): 22,
    ('absent', 300, 3, 13, 'lo', 0, 0, 'xl'): 0,
    ('head', 2100, 1, 13, 'lo', 2048, 0, 'l'): 2,
    ('head', 2100, 1, 13, 'lo', 2049, 0, 'l'): 1,
    ('head', 2100, 1, 13, 'full', 2048, 0, 'l'): 1,
    ('head', 2100, 1, 13, 'full', 2049, 0, 'l'): 1,
}


def input_key(k):
    return (k.family, k.n, k.L, k.C, k.mode, k.R, k.g, k.loss)


def seed_of(k):
    return SEEDS.get(input_key(k), 0)


class Case:
    pass


def protein_hot_rows(k):
    """the head and class families in "full" mode: lig_flag is not the hot set (the head's list is the marked support of grad_logits)"""
    return k.mode == "full" and k.family in ("head", "dense", "classes", "absent")


def build(k, seed):
    """inputs of one case on the CPU in fp32: x, h, batch, graph_ptr, lig / gen (bool), hot (sorted rows), the score's weights wx / wl / wh
    (None: not read), hot_graphs (indices of the graphs that hold a hot row)"""
    base = make_case("x2h", k.n, "spread", seed)
    gen = torch.Generator().manual_seed(7919 * seed + 31 * k.n + k.R)
    c = Case()
    c.key, c.n, c.x, c.h, c.batch, c.graph_ptr = k, k.n, base.x, base.h, base.batch, base.graph_ptr
    gp = c.graph_ptr.tolist()
    n = k.n
    forced = list(dict.fromkeys(r for r in (n - 1, n - 7, 0, n - 2) if 0 <= r < n))[:k.R]
    # rows of the first graph, or of every graph (many hot rows; the dense head, whose splits and passes cut the batch anywhere)
    pool_end = n if k.R > STRICT_MAX_HOT or k.family == "dense" else gp[1]
    pool = [r for r in torch.randperm(pool_end, generator=gen).tolist() if r not in forced]
    if len(forced) + len(pool) < k.R:                             # (n = 47: more hot rows than the first graph has)
        pool += [r for r in range(n) if r not in forced and r not in pool]
    c.hot = sorted(forced + pool[:k.R - len(forced)])
    assert len(c.hot) == k.R
    gen_rows = c.hot[::-1][:1] + [r for r in torch.tensor(c.hot)[torch.randperm(len(c.hot), generator=gen)].tolist()
                                  if r != c.hot[-1]] if k.g else []
    gen_rows = sorted(gen_rows[:k.g])
    c.gen = torch.zeros(n, dtype=torch.bool)
    c.gen[gen_rows] = True
    if protein_hot_rows(k):
        c.lig = base.lig.clone() | c.gen
    else:
        c.lig = torch.zeros(n, dtype=torch.bool)
        c.lig[c.hot] = True
    hot = torch.zeros(n, dtype=torch.bool)
    hot[c.hot] = True
    c.wx = torch.randn(n, 3, generator=gen) * c.gen[:, None].float() if "x" in k.loss else None
    c.wl = torch.randn(n, k.C, generator=gen) * hot[:, None].float() if "l" in k.loss else None
    c.wh = torch.randn(n, 128, generator=gen) * 0.1 * hot[:, None].float() if "h" in k.loss else None
    if c.wl is not None and protein_hot_rows(k) and k.C > 64 and k.R >= 2:
        # one hot row whose only non-zero weight is in the first column, one in the last: each 64-lane half of the support marking
        # must find its row alone
        for r, col in ((c.hot[0], 0), (c.hot[-1], k.C - 1)):
            keep = c.wl[r, col].clone()
            c.wl[r] = 0.0
            c.wl[r, col] = keep
            if c.wh is not None:
                c.wh[r] = 0.0
    marked = set(c.hot) | set(gen_rows)
    c.hot_graphs = [i for i, (s, e) in enumerate(zip(gp[:-1], gp[1:])) if any(s <= r < e for r in marked)]
    return c


def sub_rows(c):
    """rows of the graphs that hold a hot row, ascending"""
    gp = c.graph_ptr.tolist()
    return torch.cat([torch.arange(gp[i], gp[i + 1]) for i in c.hot_graphs]) if c.hot_graphs else torch.zeros(0, dtype=torch.long)


@functools.lru_cache(maxsize=4)
def state_dict(C, L):
    return {k: v for k, v in W.synthetic_state_dict(C, L, seed=0).items() if k.startswith("denoiser.")}


def score(xo, ho, lo, w):
    """the random-weighted score of the outputs (score of tests/test_gpu_coord_grad.py, every part optional)"""
    s = 0.0
    for out, wt in zip((xo, lo, ho), w):
        if wt is not None:
            s = s + (out * wt.to(device=out.device, dtype=out.dtype)).sum()
    return s


def oracle(c, force=None, backward=True, dtype=torch.float64):
    """float64 autograd of the score through OU.unitransformer_forward on the graphs that hold a hot row.
    -> dict(near {mlp prefix: [(row, unit)]} with edge / node numbers of the SUB-batch, rows, edge_index (sub-batch numbers), logits and
    h_L on `rows`, ref {"x", "h", module parameter name: gradient} at full size)"""
    k = c.key
    rows = sub_rows(c)
    sd = {kk: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() and not kk.endswith("offset") else v)
          for kk, v in state_dict(k.C, k.L).items()}
    res = {"rows": rows, "near": {}}
    params = {kk[len("denoiser."):]: v for kk, v in sd.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    ref = {"x": torch.zeros(c.n, 3, dtype=dtype), "h": torch.zeros(c.n, 128, dtype=dtype)}
    ref.update({kk: torch.zeros_like(v) for kk, v in params.items()})
    res["ref"] = ref
    if not rows.numel():
        return res
    x = c.x[rows].to(dtype).requires_grad_(True)
    h = c.h[rows].to(dtype).requires_grad_(True)
    outs, cur, rm_mlp, relu = {}, [None], None, F.relu

    def tagged_mlp(sd_, prefix, z):
        cur[0] = prefix
        return rm_mlp(sd_, prefix, z)

    def recording_relu(y):
        out = relu(y)
        outs[cur[0]] = out
        return out

    with relu_margins(force) as near, contextlib.ExitStack() as undo:
        rm_mlp = OU.mlp
        OU.mlp, F.relu = tagged_mlp, recording_relu
        undo.callback(lambda: (setattr(OU, "mlp", rm_mlp), setattr(F, "relu", relu)))
        if OU.knn_graph(x.detach(), c.batch[rows], 32).shape[1] == 0:
            # a batch without an edge (n = 1): every attention sum is empty, the blocks are the identity, only the classifier remains
            xo, ho, lo = x, h, OU.classifier(sd, "denoiser", h)
            inter = {"edge_index": torch.zeros(2, 0, dtype=torch.long)}
        else:
            xo, ho, lo, inter = OU.unitransformer_forward(sd, x, h, c.batch[rows], c.lig[rows], c.gen[rows], return_intermediates=True)
        s = score(xo, ho, lo, tuple(None if w is None else w[rows] for w in (c.wx, c.wl, c.wh)))
    res.update(near=dict(near), edge_index=inter["edge_index"], logits=lo.detach(), h_L=ho.detach())
    if backward and isinstance(s, torch.Tensor) and s.requires_grad:
        taps = [p for p in near if p in outs and outs[p].requires_grad]
        leaves = [x, h] + list(params.values()) + [outs[p] for p in taps]
        gs = torch.autograd.grad(s, leaves, allow_unused=True)
        gs = [torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(gs, leaves)]
        ref["x"][rows], ref["h"][rows] = gs[0], gs[1]
        for kk, g_ in zip(params, gs[2:]):
            ref[kk] = g_
        # first-order weight of every near-zero unit: a flipped mask changes dL/dy of that unit by g = dL/d relu(y), which enters the
        # LayerNorm bias gradient of its MLP as it is -- |g| / |that tensor| is the relative L2 change one flip causes there
        # flipdelta: the exact change of that bias gradient's entry `unit` when the unit's mask flips (-g if the unit is on, else +g)
        res["influence"], res["flipdelta"] = {}, {}
        for p, g_ in zip(taps, gs[2 + len(params):]):
            denom = float(ref[p[len("denoiser."):] + ".net.1.bias"].norm())
            for r, u in set(near[p]):
                res["influence"][(p, r, u)] = abs(float(g_[r, u])) / denom if denom > 0 else 0.0
                res["flipdelta"][(p, r, u)] = -float(g_[r, u]) if float(outs[p][r, u].detach()) > 0 else float(g_[r, u])
    return res


def carrying_near(c, res):
    """the near-zero pre-ReLU units of `res` that carry gradient (an upper bound below the last layer).  Last layer: key / value MLPs on
    edges whose centre is hot (x2h, when the score reads the logits or h_out) or generated (h2x, when it reads x_out) or a neighbour of
    a generated row, the query MLPs on those rows.  Earlier layers: every x2h unit of the evaluated graphs, the h2x units of the
    generated rows (only they move).  The gate: every edge a block with gradient reads."""
    k = c.key
    pos = {r: i for i, r in enumerate(res["rows"].tolist())}
    gen_all = {pos[r] for r in c.gen.nonzero().flatten().tolist()}
    hot = {pos[r] for r in c.hot} if ("l" in k.loss or "h" in k.loss) else set()
    gen = gen_all if "x" in k.loss else set()
    if not res["near"] or not (hot or gen):
        return []
    dst = res["edge_index"][1].tolist()
    # an h2x block's gradient reaches the x2h block of the same layer through h_mid of the generated rows and their neighbours
    src_of_gen = {s for s, d in zip(res["edge_index"][0].tolist(), dst) if d in gen}
    x2h_rows = hot | gen | src_of_gen
    bad = []
    for p, lst in res["near"].items():
        last = ".blocks." not in p and k.L == 1 or f".blocks.{k.L - 1}." in p
        for r, u in lst:
            node = r if p.endswith("q_func") else dst[r]
            if ".h2x_layers." in p:
                carry = node in (gen if last else gen_all)
            elif ".x2h_layers." in p:
                carry = node in x2h_rows if last else True
            else:                       # the gate
                carry = node in x2h_rows if k.L == 1 else True
            if carry:
                bad.append((p, r, u))
    return bad


# gerr's own defaults (tests/test_gpu_training.py) and the x / h tolerance of `failures` (tests/test_gpu_coord_grad.py), not restated;
# the 1e-3 of `failures` for parameter tensors is a literal inside that function (test_constants_follow_the_sources pins the line)
GERR_RTOL, GERR_FLOOR = (inspect.signature(gerr).parameters[n].default for n in ("rtol", "floor"))
PARAM_TOL = 1e-3


def heavy_units(res):
    """the near-zero units whose flip ALONE moves a tensor of their MLP past its tolerance (first order, see oracle)"""
    return sorted(u for u, w in res.get("influence", {}).items() if w > PARAM_TOL)


LARGE_SEEDS = 3         # the one-layer 2048 / 2049-row cases take the seed in 0 .. LARGE_SEEDS - 1 with the fewest heavy units
PROBE_SEEDS, PROBE_MAX = 3, 6.0


def find_seed(k, limit=400):
    """<= 65 hot rows: the first seed without a near-zero unit that carries gradient, or None where the mean count over the first
    PROBE_SEEDS seeds is above PROBE_MAX (no seed within `limit` can be expected to be clean: the case is not strict, seed 0).
    The one-layer cases of 2048 / 2049 hot rows are checked with ONE verified ReLU flip, which cannot explain two flips that each move a
    tensor past its tolerance; no seed is free of heavy units at that size (2 - 15 of ~170 near-zero units), so they take the seed with
    the fewest of them (the first on a tie).  The three-layer ones (a set of flips): 0."""
    if k.R <= STRICT_MAX_HOT:
        counts = []
        for seed in range(limit):
            c = build(k, seed)
            counts.append(len(carrying_near(c, oracle(c, backward=False))))
            if counts[-1] == 0:
                return seed
            if len(counts) == PROBE_SEEDS and sum(counts) / PROBE_SEEDS > PROBE_MAX:
                return None
        return None
    if k.R in R_LARGE and k.L == 1:
        counts = [len(heavy_units(oracle(build(k, seed)))) for seed in range(LARGE_SEEDS)]
        return counts.index(min(counts))
    return None


def select_flips(got, res):
    """the near-zero units whose flip the gradients `got` show: a flip of unit (row, u) of an MLP changes entry u of that MLP's
    LayerNorm-bias gradient by exactly flipdelta, so per MLP and entry the subset of its near-zero units (the heaviest; at most 6) that brings the deviation of that entry closest to zero, if it at least halves it.
    -> force {mlp prefix: [(row, unit)]} for oracle().  A choice, not a check: the oracle run with these units forced is."""
    cols = {}
    for (p, r, u), d in sorted(res.get("flipdelta", {}).items()):
        cols.setdefault((p, u), []).append((r, d))
    force = {}
    for (p, u), lst in cols.items():
        name = p[len("denoiser."):] + ".net.1.bias"
        ref = res["ref"][name].double()
        dev = float(got[name].detach().cpu().double()[u]) - float(ref[u])
        # (a tenth of gerr's floor for this tensor: the LayerNorm backward and the inputs amplify a flip by up to ~10 in net.0.weight, and
        # the GPU's rounding of a bias-gradient entry is two orders below gerr's floor -- a lighter unit could only be named by chance)
        tol = 0.1 * GERR_FLOOR * max(float(ref.abs().max()), 1e-12)
        lst = sorted((x for x in lst if abs(x[1]) > tol), key=lambda x: -abs(x[1]))[:6]
        best, left = [], abs(dev)
        for m in range(1, 1 << len(lst)):
            sub = [lst[i] for i in range(len(lst)) if m >> i & 1]
            rest = abs(dev - sum(d for _, d in sub))
            if rest < left:
                best, left = sub, rest
        if best and left < 0.5 * abs(dev):
            force.setdefault(p, []).extend((r, u) for r, _ in best)
    return force


def list_sizes(c):
    """(|A1|, |A2|) of the backward's receptive-field lists as the oracle's knn_graph gives them: A1 = seed | nbr(gen), A2 = A1 | nbr(A1);
    the seed is gen | lig, plus the rows where the score reads h_out or the logits when the caller passes a gradient on h_out"""
    k = c.key
    seed = c.gen | c.lig
    if k.mode != "lo":
        for w in (c.wl, c.wh):
            if w is not None:
                seed = seed | (w.abs().sum(1) > 0)
    src, dst = OU.knn_graph(c.x, c.batch, 32)
    a1 = seed.clone()
    a1[src[c.gen[dst]]] = True
    a2 = a1.clone()
    a2[src[a1[dst]]] = True
    return int(a1.sum()), int(a2.sum())


def head_rows(c):
    """the rows the listed head walks: lig_flag rows ("lo"), else the support of the score's weights on the logits"""
    if c.wl is None:
        return []
    if c.key.mode == "lo":
        return c.lig.nonzero().flatten().tolist()
    return (c.wl.abs().sum(1) > 0).nonzero().flatten().tolist()




def head_sensitivity(c, res):
    """for every listed head row i: the largest (change of a classifier gradient when row i's contribution dlogits_i (x) act_i is
    removed) / (gerr's tolerance of that entry), over the four tensors.  -> {row: ratio}"""
    k = c.key
    sd = {kk: v.double() for kk, v in state_dict(k.C, k.L).items() if ".classifier." in kk}
    w0, b0, w1 = sd["denoiser.classifier.0.weight"], sd["denoiser.classifier.0.bias"], sd["denoiser.classifier.2.weight"]
    pos = {r: i for i, r in enumerate(res["rows"].tolist())}
    ref = res["ref"]
    tol = {kk: GERR_FLOOR * max(float(ref[kk].abs().max()), 1e-12) + GERR_RTOL * ref[kk].abs()
           for kk in ("classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias")}
    out = {}
    for r in head_rows(c):
        hl = res["h_L"][pos[r]].double()
        dl = c.wl[r].double()
        pre = w0 @ hl + b0
        act = torch.nn.functional.softplus(pre) - math.log(2.0)
        dpre = (w1.t() @ dl) * torch.sigmoid(pre)
        parts = {"classifier.2.weight": torch.outer(dl, act), "classifier.2.bias": dl, "classifier.0.weight": torch.outer(dpre, hl),
                 "classifier.0.bias": dpre}
        out[r] = max(float((parts[kk].abs() / tol[kk]).max()) for kk in parts)
    return out


def row_failures(got, ref, what):
    """the row-wise bound of the larger cases: |got_i - ref_i| <= 1e-2 |ref_i| + 2e-5 max_j |ref_j| (a missing or doubled row is an
    error of order 1 in that row; one flipped ReLU unit moves a row by ~2.4e-4 of its norm).  -> (worst ratio, [messages])"""
    a, b = got.detach().cpu().double(), ref.detach().cpu().double()
    d, nb = (a - b).norm(dim=1), b.norm(dim=1)
    tol = 1e-2 * nb + 2e-5 * max(float(nb.max()), 1e-30)
    bad = (d > tol).nonzero().flatten().tolist()
    msgs = [f"{what} row {i}: |delta| {float(d[i]):.3e} > {float(tol[i]):.3e} (|ref row| {float(nb[i]):.3e})" for i in bad[:4]]
    return float((d / tol).max()) if d.numel() else 0.0, msgs


def units_touching(res, rows):
    """the near-zero units of `res` on an edge that starts or ends in one of `rows` (batch row numbers), or on such a row's query"""
    pos = {r: i for i, r in enumerate(res["rows"].tolist())}
    hit = {pos[r] for r in rows if r in pos}
    src, dst = res["edge_index"].tolist()
    out = []
    for p, lst in res["near"].items():
        for r, u in sorted(set(lst)):
            if (r in hit) if p.endswith("q_func") else (src[r] in hit or dst[r] in hit):
                out.append((p, r, u))
    return out


if __name__ == "__main__":      # (re)derive SEEDS
    print("SEEDS = {")
    import sys
    done = set()
    for key in all_cases():
        if len(sys.argv) > 1 and key.family not in sys.argv[1:]:
            continue
        if input_key(key) not in done and input_key(key) not in SEEDS:
            done.add(input_key(key))
            seed = find_seed(key)
            if seed is not None:
                print(f"    {input_key(key)!r}: {seed},", flush=True)
    print("}")
