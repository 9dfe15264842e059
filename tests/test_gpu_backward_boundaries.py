"""The block backward kernels (csrc/api_train.hip attention_block_backward, both block kinds) and the gate backward at EVERY row count
at which their launchers or kernels change regime, against float64 autograd on the CPU oracle.

Method -- a LOCALISED upstream gradient.  g_out is zero except on a hot set of at most 32 rows, so one dropped or doubled hot row moves
every parameter gradient by several per cent (a dense g_out at N = 16 385 would bury it), every other row must contribute exactly
nothing, and the float64 oracle only needs the ~1000 edges whose centre is hot: edge_index comes from the GPU's nbr / deg
(stages.edge_index_from_nbr), filtered to dst in hot, with the full x and h.  Before every case the training workspace is filled with
0xFF bytes (NaN as float, -1 as int) and every output with NaN, so a slab or row that is read without having been written shows.

Sizes (SIZES): both sides of every switch in n -- slab folds (8 / 9, 64 / 65, 1024 / 1025), the 8 / 16 / 32-row tiles of the node
kernels, wgrad groups 1 -> 2 (128 / 129) and their cap (6528 / 6529), the persistent loops (256 / 257, 2048 / 2049), the XCD-aware
partition of the x2h edge backward (504 / 505 / 512 / 513), its first and second static round (4088 / 4089 / 4097, 6145), the
query-backward grid cap (16384 / 16385), and n = 1, 2.  The h2x backward runs in listed-row mode: its tiles are in the number of gen
rows, swept separately (GEN_COUNTS; hot rows: the `edges` set of the list positions, filled up to 24 with positions drawn at random).

Graphs (graph_sizes): n >= 8 -> graphs of 600 nodes, then the remainder, over the first n - 7 rows, then one graph of 1 node (deg 0)
and one of 6 nodes (deg 5), so that two graph boundaries and short-degree rows lie in the last tile; n < 8 -> one graph.  The 6-node
graph comes LAST: the last row, which is alone in the extra pass / tile / octet at every size one past a boundary (n = 1 mod 8 and
mod 16), and the last listed gen row must have edges, or a kernel that drops that pass would lose nothing.  ~10 % of the rows are
ligand.

Hot sets: `edges` = rows 0, 1, the last three, the rows b - 1 and b at the last multiple b < n of 16, 32 and 128, and, while fewer
than 32 rows are taken, the same pair at the cuts of the x2h edge backward's node partition (ends of the per-XCD ranges and starts of
their dynamic tails, from schedule() of tests/test_bx_partition.py) and at the multiples of wgrad's nodes_per_group once the groups are
capped -- both lists taken from their ends inwards, alternating; `spread` = the first and the last row plus 22 rows drawn uniformly.

No ReLU-flip exception here: every case asserts, as a PRECONDITION on its inputs, that the float64 oracle sees no pre-ReLU value within
FLIP_EPS of zero among the units that carry gradient (k / v MLPs on the filtered edges, q MLP on the hot rows, the gate MLP on the
hot rows' edges).  The per-case seeds in SEEDS were searched on the CPU for that (`python -m tests.test_gpu_backward_boundaries`
prints the table); test_seed_table_is_clean re-derives the condition without a GPU, with OU.knn_graph on the graphs that hold a hot row.

Tolerance: gerr of tests/test_gpu_training.py at its defaults (rtol 2e-4 + 2e-5 x max|ref|) for every tensor; exact zeros where the
mathematics gives zero.  Every case prints its worst error / tolerance ratio.  Wall time of the whole file on an
MI355X (250 GPU cases): 7.6 s, the slowest case 0.8 s (the first launch), every other below 0.1 s (measured with the 1-node graph last)."""
import functools
import math

import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, stages
from oracle import unitransformer as OU
from tests.relu_flip import FLIP_EPS, relu_margins
from tests.test_bx_partition import schedule
from tests.test_gpu_training import MLP_KEYS, edge_rows, gerr

DEV = "cuda:0"
SIZES = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 256, 257, 504, 505, 512, 513, 1024, 1025, 2048, 2049, 4088, 4089,
         4097, 6145, 6528, 6529, 16384, 16385]
HOTSETS = ("edges", "spread")
GEN_COUNTS = [(600, c) for c in (0, 1, 7, 8, 9, 15, 16, 17, 33)] + [(2049, 257)]
GATE_SIZES = [1, 2, 33, 2048, 2049, 4097]      # 2048 nodes = 4096 tiles = one round of GATE_GRID x GATE_WAVES waves
GATE_LISTS = (0, 1, 9, 300)                    # entries of the `rows` list (0: no list); capped at n
MAX_HOT, N_SPREAD = 32, 24
WGRAD_GROUPS_MAX = 51                          # api_train.hip CBGX_WGRAD_GROUPS_MAX
# x2h_edge_grid, WGRAD_GROUPS_MAX and `per` in edge_positions restate launcher arithmetic so that the hot rows sit on the real
# boundaries; LAUNCHER_LINES are the source lines they restate, and test_hot_rows_follow_the_launchers fails when one of them changes
LAUNCHER_LINES = {
    "api_train.hip": ("constexpr int EDGE_GRID = 256;", "#define CBGX_WGRAD_GROUPS_MAX 51", "int g = (n + 127) / 128;",
                      "int eg = gen3 ? edge_grid((n + 7) / 8) : edge_grid(n);", "if (gen3 && eg >= 64) eg &= ~7;"),
    "train_bwd_mfma.hip": ("const int per = ((n_nodes + groups - 1) / groups + 15) / 16 * 16;",),
}

# (kind, n, tag) -> seed of the case's inputs: the first seed >= 0 whose precondition holds (find_seed below)
SEEDS = {
    ('x2h', 1, 'edges'): 0,
    ('x2h', 1, 'spread'): 0,
    ('x2h', 2, 'edges'): 0,
    ('x2h', 2, 'spread'): 0,
    ('x2h', 7, 'edges'): 0,
    ('x2h', 7, 'spread'): 0,
    ('x2h', 8, 'edges'): 0,
    ('x2h', 8, 'spread'): 0,
    ('x2h', 9, 'edges'): 0,
    ('x2h', 9, 'spread'): 0,
    ('x2h', 15, 'edges'): 0,
    ('x2h', 15, 'spread'): 0,
    ('x2h', 16, 'edges'): 0,
    ('x2h', 16, 'spread'): 0,
    ('x2h', 17, 'edges'): 0,
    ('x2h', 17, 'spread'): 0,
    ('x2h', 31, 'edges'): 0,
    ('x2h', 31, 'spread'): 0,
    ('x2h', 32, 'edges'): 0,
    ('x2h', 32, 'spread'): 2,
    ('x2h', 33, 'edges'): 0,
    ('x2h', 33, 'spread'): 1,
    ('x2h', 64, 'edges'): 0,
    ('x2h', 64, 'spread'): 0,
    ('x2h', 65, 'edges'): 0,
    ('x2h', 65, 'spread'): 0,
    ('x2h', 128, 'edges'): 0,
    ('x2h', 128, 'spread'): 0,
    ('x2h', 129, 'edges'): 0,
    ('x2h', 129, 'spread'): 1,
    ('x2h', 256, 'edges'): 0,
    ('x2h', 256, 'spread'): 2,
    ('x2h', 257, 'edges'): 0,
    ('x2h', 257, 'spread'): 0,
    ('x2h', 504, 'edges'): 0,
    ('x2h', 504, 'spread'): 0,
    ('x2h', 505, 'edges'): 0,
    ('x2h', 505, 'spread'): 0,
    ('x2h', 512, 'edges'): 0,
    ('x2h', 512, 'spread'): 0,
    ('x2h', 513, 'edges'): 0,
    ('x2h', 513, 'spread'): 2,
    ('x2h', 1024, 'edges'): 1,
    ('x2h', 1024, 'spread'): 2,
    ('x2h', 1025, 'edges'): 1,
    ('x2h', 1025, 'spread'): 3,
    ('x2h', 2048, 'edges'): 1,
    ('x2h', 2048, 'spread'): 1,
    ('x2h', 2049, 'edges'): 1,
    ('x2h', 2049, 'spread'): 1,
    ('x2h', 4088, 'edges'): 1,
    ('x2h', 4088, 'spread'): 1,
    ('x2h', 4089, 'edges'): 2,
    ('x2h', 4089, 'spread'): 3,
    ('x2h', 4097, 'edges'): 0,
    ('x2h', 4097, 'spread'): 0,
    ('x2h', 6145, 'edges'): 0,
    ('x2h', 6145, 'spread'): 0,
    ('x2h', 6528, 'edges'): 3,
    ('x2h', 6528, 'spread'): 0,
    ('x2h', 6529, 'edges'): 0,
    ('x2h', 6529, 'spread'): 0,
    ('x2h', 16384, 'edges'): 4,
    ('x2h', 16384, 'spread'): 1,
    ('x2h', 16385, 'edges'): 0,
    ('x2h', 16385, 'spread'): 0,
    ('h2x', 1, 'edges'): 0,
    ('h2x', 1, 'spread'): 0,
    ('h2x', 2, 'edges'): 0,
    ('h2x', 2, 'spread'): 0,
    ('h2x', 7, 'edges'): 0,
    ('h2x', 7, 'spread'): 0,
    ('h2x', 8, 'edges'): 0,
    ('h2x', 8, 'spread'): 0,
    ('h2x', 9, 'edges'): 0,
    ('h2x', 9, 'spread'): 0,
    ('h2x', 15, 'edges'): 0,
    ('h2x', 15, 'spread'): 0,
    ('h2x', 16, 'edges'): 0,
    ('h2x', 16, 'spread'): 0,
    ('h2x', 17, 'edges'): 0,
    ('h2x', 17, 'spread'): 0,
    ('h2x', 31, 'edges'): 0,
    ('h2x', 31, 'spread'): 2,
    ('h2x', 32, 'edges'): 0,
    ('h2x', 32, 'spread'): 1,
    ('h2x', 33, 'edges'): 0,
    ('h2x', 33, 'spread'): 0,
    ('h2x', 64, 'edges'): 0,
    ('h2x', 64, 'spread'): 0,
    ('h2x', 65, 'edges'): 0,
    ('h2x', 65, 'spread'): 0,
    ('h2x', 128, 'edges'): 2,
    ('h2x', 128, 'spread'): 0,
    ('h2x', 129, 'edges'): 0,
    ('h2x', 129, 'spread'): 0,
    ('h2x', 256, 'edges'): 0,
    ('h2x', 256, 'spread'): 0,
    ('h2x', 257, 'edges'): 0,
    ('h2x', 257, 'spread'): 2,
    ('h2x', 504, 'edges'): 0,
    ('h2x', 504, 'spread'): 0,
    ('h2x', 505, 'edges'): 0,
    ('h2x', 505, 'spread'): 0,
    ('h2x', 512, 'edges'): 0,
    ('h2x', 512, 'spread'): 1,
    ('h2x', 513, 'edges'): 1,
    ('h2x', 513, 'spread'): 1,
    ('h2x', 1024, 'edges'): 7,
    ('h2x', 1024, 'spread'): 2,
    ('h2x', 1025, 'edges'): 0,
    ('h2x', 1025, 'spread'): 5,
    ('h2x', 2048, 'edges'): 0,
    ('h2x', 2048, 'spread'): 2,
    ('h2x', 2049, 'edges'): 0,
    ('h2x', 2049, 'spread'): 2,
    ('h2x', 4088, 'edges'): 0,
    ('h2x', 4088, 'spread'): 1,
    ('h2x', 4089, 'edges'): 9,
    ('h2x', 4089, 'spread'): 0,
    ('h2x', 4097, 'edges'): 0,
    ('h2x', 4097, 'spread'): 0,
    ('h2x', 6145, 'edges'): 0,
    ('h2x', 6145, 'spread'): 0,
    ('h2x', 6528, 'edges'): 2,
    ('h2x', 6528, 'spread'): 1,
    ('h2x', 6529, 'edges'): 5,
    ('h2x', 6529, 'spread'): 3,
    ('h2x', 16384, 'edges'): 1,
    ('h2x', 16384, 'spread'): 1,
    ('h2x', 16385, 'edges'): 5,
    ('h2x', 16385, 'spread'): 0,
    ('h2x', 600, 'gen0'): 2,
    ('h2x', 600, 'gen1'): 0,
    ('h2x', 600, 'gen7'): 0,
    ('h2x', 600, 'gen8'): 0,
    ('h2x', 600, 'gen9'): 0,
    ('h2x', 600, 'gen15'): 0,
    ('h2x', 600, 'gen16'): 0,
    ('h2x', 600, 'gen17'): 0,
    ('h2x', 600, 'gen33'): 0,
    ('h2x', 2049, 'gen257'): 1,
    ('gate', 1, 'list0'): 0,
    ('gate', 1, 'list1'): 0,
    ('gate', 2, 'list0'): 0,
    ('gate', 2, 'list1'): 0,
    ('gate', 2, 'list2'): 0,
    ('gate', 33, 'list0'): 0,
    ('gate', 33, 'list1'): 0,
    ('gate', 33, 'list9'): 0,
    ('gate', 33, 'list33'): 0,
    ('gate', 2048, 'list0'): 0,
    ('gate', 2048, 'list1'): 0,
    ('gate', 2048, 'list9'): 0,
    ('gate', 2048, 'list300'): 0,
    ('gate', 2049, 'list0'): 0,
    ('gate', 2049, 'list1'): 0,
    ('gate', 2049, 'list9'): 0,
    ('gate', 2049, 'list300'): 0,
    ('gate', 4097, 'list0'): 2,
    ('gate', 4097, 'list1'): 0,
    ('gate', 4097, 'list9'): 2,
    ('gate', 4097, 'list300'): 2,
}


def graph_sizes(n):
    if n < 8:
        return [n]
    main = n - 7
    return [600] * (main // 600) + ([main % 600] if main % 600 else []) + [1, 6]


def x2h_edge_grid(n):
    """workgroups of the x2h edge backward (api_train.hip: edge_grid((n + 7) / 8), a multiple of 8 from 64 on)"""
    eg = min(256, max(1, (n + 7) // 8))
    return eg & ~7 if eg >= 64 else eg


def _ends_inward(v):
    out = []
    while v:
        out.append(v.pop())
        if v:
            out.append(v.pop(0))
    return out


def edge_positions(n):
    """the `edges` hot set of a dimension of n rows (see the module docstring)"""
    rows = [r for r in (0, 1, n - 3, n - 2, n - 1) if 0 <= r < n]
    for m in (16, 32, 128):
        b = (n - 1) // m * m
        rows += [r for r in (b - 1, b) if 0 <= r < n]
    rows = list(dict.fromkeys(rows))
    cuts = _ends_inward(schedule(n, x2h_edge_grid(n), boundaries=True)[2])
    groups = min(WGRAD_GROUPS_MAX, (n + 127) // 128)
    per = ((n + groups - 1) // groups + 15) // 16 * 16           # launch_wgrad_mfma's nodes_per_group
    npg = _ends_inward(list(range(per, n, per))) if n > 128 * WGRAD_GROUPS_MAX else []
    while cuts or npg:
        for lst in (cuts, npg):
            if lst:
                b = lst.pop(0)
                new = [r for r in (b - 1, b) if r not in rows]
                if len(rows) + len(new) <= MAX_HOT:
                    rows += new
    return sorted(rows)


class Case:
    pass


def make_case(kind, n, tag, seed):
    """inputs of one case, all on the CPU in fp32: x, h, lig (bool), gen (bool), batch, graph_ptr, hot (sorted list), gout"""
    g = torch.Generator().manual_seed(1000003 * seed + n)
    c = Case()
    c.kind, c.n, c.tag = kind, n, tag
    sizes = graph_sizes(n)
    c.graph_ptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32)
    c.batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    scale = torch.repeat_interleave(torch.tensor([1.2 * s ** (1.0 / 3.0) for s in sizes]), torch.tensor(sizes))
    c.x = torch.randn(n, 3, generator=g) * scale[:, None]
    c.h = torch.randn(n, 128, generator=g)
    c.lig = torch.rand(n, generator=g) < 0.1
    perm = torch.randperm(n, generator=g).tolist()
    c.gen = torch.zeros(n, dtype=torch.bool)
    c.rows = None
    if tag.startswith("gen"):           # h2x with exactly `count` gen rows; the hot rows by their position in the gen list
        count = int(tag[3:])
        forced = list(dict.fromkeys(r for r in (n - 1, 0, n - 2) if 0 <= r < n))[:count]
        gen_rows = sorted(forced + [r for r in perm if r not in forced][:count - len(forced)])
        c.gen[gen_rows] = True
        pos = edge_positions(count) if count else []
        pos += [p for p in torch.randperm(max(count, 1), generator=g).tolist() if p not in pos][:max(0, N_SPREAD - len(pos))]
        hot = sorted(gen_rows[p] for p in pos) if count else sorted(perm[:N_SPREAD])
    elif tag.startswith("list"):        # gate with a `rows` list of L entries that holds the hot rows (L = 0: no list)
        L = min(int(tag[4:]), n)
        forced = list(dict.fromkeys(r for r in (n - 1, 0) if 0 <= r < n))
        order = forced + [r for r in perm if r not in forced]
        hot = sorted(order[:min(L, N_SPREAD) if L else N_SPREAD])
        c.rows = sorted(order[:L]) if L else None
    elif tag == "edges":
        hot = edge_positions(n)
    else:
        forced = [r for r in (0, n - 1) if 0 <= r < n]
        hot = sorted(set(forced + perm[:N_SPREAD - 2]))
    assert 1 <= len(hot) <= MAX_HOT and len(set(hot)) == len(hot)
    c.hot = hot
    if kind == "h2x" and not tag.startswith("gen"):
        c.gen = c.lig.clone()
        c.gen[hot] = True
    if kind == "h2x" and tag != "gen0":
        c.lig = c.lig | c.gen
    width = {"x2h": 128, "h2x": 3, "gate": 32}[kind]
    c.gout = torch.zeros(n, width)
    c.gout[hot] = torch.randn(len(hot), width, generator=g)
    return c


def cpu_edges(c):
    """the edges whose centre is hot, [2, E] in the reference's order: OU.knn_graph on the graphs that hold a hot row"""
    out = []
    gp = c.graph_ptr.tolist()
    hot = torch.tensor(c.hot)
    for s, e in zip(gp[:-1], gp[1:]):
        if bool(((hot >= s) & (hot < e)).any()):
            out.append(OU.knn_graph(c.x[s:e], torch.zeros(e - s, dtype=torch.long), 32) + s)
    ei = torch.cat(out, 1) if out else torch.zeros(2, 0, dtype=torch.long)
    return ei[:, torch.isin(ei[1], hot)]


@functools.lru_cache(maxsize=None)
def sd64():
    from oracle import weights
    sd = weights.synthetic_state_dict(13, 9, seed=0)
    return {k: v.double() for k, v in sd.items() if k.startswith(("denoiser.blocks.0.", "denoiser.dist_emb.")) and v.is_floating_point()}


FNS = {"x2h": ("hk_func", "hv_func", "hq_func"), "h2x": ("xk_func", "xv_func", "xq_func")}


def param_keys(kind):
    if kind == "gate":
        return [f"denoiser.dist_emb.1.{k}" for k in MLP_KEYS]
    return [f"denoiser.blocks.0.{kind}_layers.0.{fn}.{k}" for fn in FNS[kind] for k in MLP_KEYS]


def oracle(c, ei, e_w=None, backward=True):
    """float64 autograd of the case on the edges `ei` (centres: the hot rows).  e_w [E] (block kinds): the gate values the GPU used,
    else the oracle's own.  -> dict(near = pre-ReLU values within FLIP_EPS of zero on units that carry gradient, gx, gh, gew, pg)"""
    sd = dict(sd64())
    keys = param_keys(c.kind)
    for k in keys:
        sd[k] = sd[k].clone().requires_grad_(True)
    x = c.x.double().requires_grad_(True)
    h = c.h.double().requires_grad_(True)
    hot = set(c.hot)
    if ei.shape[1] == 0:        # no edge has a hot centre (n = 1): the attention sums are empty, only the identity paths remain
        z = torch.zeros(c.n, 3, dtype=torch.float64)
        return {"near": [], "keys": keys, "gx": c.gout.double() if c.kind == "h2x" else z,
                "gh": c.gout.double() if c.kind == "x2h" else torch.zeros_like(h), "gew": torch.zeros(0, dtype=torch.float64),
                "pg": [torch.zeros_like(sd[k]) for k in keys]}
    if c.kind != "gate":
        ew = (OU.edge_gate(sd, "denoiser", x.detach(), ei).detach() if e_w is None else e_w.double()).reshape(-1, 1).requires_grad_(True)
    with relu_margins() as near:
        if c.kind == "gate":
            out = OU.edge_gate(sd, "denoiser", x, ei)                       # [E, 1]
            slot = torch.arange(ei.shape[1]) - torch.searchsorted(ei[1].contiguous(), ei[1].contiguous())
            up = c.gout.double()[ei[1], slot].view(-1, 1)
            leaves = [x]
        else:
            et = OU.build_edge_type(ei, c.lig)
            prefix = f"denoiser.blocks.0.{c.kind}_layers.0"
            if c.kind == "x2h":
                out = OU.x2h_attention(sd, prefix, x, h, et, ei, ew)
            else:
                out = x + OU.h2x_attention(sd, prefix, x, h, et, ei, ew) * c.gen.unsqueeze(-1).double()
            up = c.gout.double()
            leaves = [x, h, ew]
    bad = [(p, r, u) for p, lst in near.items() for r, u in lst if not p.endswith("q_func") or r in hot]
    res = {"near": bad, "keys": keys}
    if backward:
        gs = torch.autograd.grad(out, leaves + [sd[k] for k in keys], up, allow_unused=True)
        gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, leaves + [sd[k] for k in keys])]
        res["gx"] = gs[0]
        if c.kind != "gate":
            res["gh"], res["gew"] = gs[1], gs[2].flatten()
        res["pg"] = gs[len(leaves):]
    return res


def precondition(c, res):
    assert not res["near"], (f"{c.kind} n={c.n} {c.tag}: {len(res['near'])} pre-ReLU value(s) within {FLIP_EPS} of zero on units that carry "
                             f"gradient, e.g. {res['near'][:3]}: pick another seed (python -m tests.test_gpu_backward_boundaries)")


def block_cases():
    return [(k, n, t) for k in ("x2h", "h2x") for n in SIZES for t in HOTSETS] + [("h2x", n, f"gen{c}") for n, c in GEN_COUNTS]


def gate_cases():
    out = []
    for n in GATE_SIZES:
        for L in dict.fromkeys(min(L, n) for L in GATE_LISTS):
            out.append(("gate", n, f"list{L}"))
    return out


def find_seed(kind, n, tag, limit=200):
    for seed in range(limit):
        c = make_case(kind, n, tag, seed)
        if not oracle(c, cpu_edges(c), backward=False)["near"]:
            return seed
    raise RuntimeError((kind, n, tag))


def _id(case):
    return "-".join(str(v) for v in case)


# ---- without a GPU: the committed seeds give inputs on which no ReLU that carries gradient is within rounding of its kink ------------
@pytest.mark.parametrize("case", block_cases() + gate_cases(), ids=_id)
def test_seed_table_is_clean(case):
    c = make_case(*case, SEEDS[case])
    precondition(c, oracle(c, cpu_edges(c), backward=False))


def test_every_boundary_has_a_case_on_each_side():
    assert set(SEEDS) == set(block_cases() + gate_cases())
    for lo in (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4088, 6528, 16384):
        assert lo in SIZES and lo + 1 in SIZES
    for n in SIZES:
        hot = edge_positions(n)
        assert len(hot) <= MAX_HOT and {0, n - 1} <= set(hot)
        if n > 16:
            b = (n - 1) // 16 * 16
            assert {b - 1, b} <= set(hot)
    cuts = schedule(4097, x2h_edge_grid(4097), boundaries=True)[2]
    assert 256 in cuts and {255, 256} <= set(edge_positions(4097))          # the first static round ends at node 256 of XCD 0


def test_hot_rows_follow_the_launchers():
    import os
    csrc = os.path.join(os.path.dirname(os.path.abspath(C.__file__)), "csrc")
    for name, lines in LAUNCHER_LINES.items():
        text = open(os.path.join(csrc, name)).read()
        for line in lines:
            assert line in text, f"{name} no longer has `{line}`: update x2h_edge_grid / edge_positions to the new launcher"


def test_last_rows_carry_gradient():
    """the last row (alone in the extra pass at every size one past a boundary) and the last listed gen row have edges"""
    for n in SIZES:
        if n >= 2:
            assert graph_sizes(n)[-1] >= 2 and sum(graph_sizes(n)) == n
    for n, count in GEN_COUNTS:
        if count:
            c = make_case("h2x", n, f"gen{count}", SEEDS[("h2x", n, f"gen{count}")])
            last = int(c.gen.nonzero().max())
            assert last in c.hot and int((c.batch == c.batch[last]).sum()) >= 2


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed(synthetic_sd):
    m = C.get_model(C.default_targetdiff_config(13)).eval()
    m.load_state_dict(synthetic_sd, strict=True)
    return m.to(DEV).denoiser.packed_weights(torch.device(DEV))


def nan_workspace(n):
    bytes_ = _native.lib().cbgx_train_workspace_bytes(n)
    return torch.full((bytes_,), 0xFF, dtype=torch.uint8, device=DEV)


def ratio(a, b, rtol=2e-4, floor=2e-5):
    """worst |a - b| / tolerance of gerr (its defaults)"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if not a.numel():
        return 0.0
    tol = floor * max(float(b.abs().max()), 1e-12) + rtol * b.abs()
    return float(((a - b).abs() / tol).max())


def check(pairs, label):
    worst, msgs = 0.0, []
    for what, a, b in pairs:
        assert a.numel() == b.numel(), f"{label} {what}: {tuple(a.shape)} against the reference's {tuple(b.shape)}"
        assert bool(torch.isfinite(a).all()), f"{label} {what}: not finite (read before written?)"
        if not a.numel():       # n = 1: no edge at all, so no live slot of grad_e_w to compare (the dead ones are checked for zeros)
            continue
        worst = max(worst, ratio(a, b))
        msg = gerr(a, b, what)
        if msg:
            msgs.append(msg)
    print(f"RATIO {label} worst error / tolerance = {worst:.3f}")
    assert not msgs, (label, msgs)


def gpu_graph(c, packed):
    x = c.x.to(DEV)
    nbr, deg = stages.knn_graph(x, c.graph_ptr.to(DEV))
    e_w = stages.edge_gate(packed, x, nbr, deg)
    hot = torch.tensor(c.hot, device=DEV)
    ei = stages.edge_index_from_nbr(nbr, deg)
    keep = torch.isin(ei[1], hot)
    slot = torch.arange(32, device=DEV)[None, :] < deg[:, None]
    return x, nbr, deg, e_w, ei[:, keep].cpu(), e_w[slot][keep].cpu(), slot


def zero_outside(t, rows, what):
    """exactly zero on every row not in `rows`"""
    m = torch.ones(t.shape[0], dtype=torch.bool, device=t.device)
    m[torch.as_tensor(sorted(rows), dtype=torch.long, device=t.device)] = False
    assert float(t[m].abs().sum()) == 0.0, f"{what}: non-zero outside the rows that can carry gradient"


def run_block(c, packed, label):
    x, nbr, deg, e_w, ei, ew_edges, slot = gpu_graph(c, packed)
    ref = oracle(c, ei, ew_edges)
    precondition(c, ref)
    lig = c.lig.to(DEV).to(torch.uint8)
    args = (packed, 0, x, c.h.to(DEV), nbr, deg, lig)
    kw = dict(ws=nan_workspace(c.n), fill=float("nan"))
    gout = c.gout.to(DEV)
    if c.kind == "x2h":
        gh, gx, gew, pg = stages.x2h_attention_backward(*args, e_w, gout, **kw)
    else:
        gh, gx, gew, pg = stages.h2x_attention_backward(*args, c.gen.to(DEV).to(torch.uint8), e_w, gout, **kw)
    torch.cuda.synchronize()
    hot = torch.tensor(c.hot, device=DEV)
    involved = set(c.hot) | set(ei[0].tolist())
    live = torch.zeros_like(slot)
    live[hot] = slot[hot]
    pairs = [(f"{c.kind} grad_h", gh, ref["gh"]), (f"{c.kind} grad_x", gx, ref["gx"]), (f"{c.kind} grad_e_w", gew[live], ref["gew"])]
    for k, a, b in zip(ref["keys"], pg, ref["pg"]):
        if k.endswith("k_func.net.3.bias"):
            assert float(a.abs().max()) == 0.0      # the key bias cancels in the softmax: exactly zero here, round-off in autograd
            continue
        pairs.append((k, a, b))
    check(pairs, label)
    # exact zeros where the mathematics gives zero: stray writes, stale workspace
    assert float(gew[~live].abs().sum()) == 0.0, "grad_e_w: non-zero on a row that is not hot or a slot >= deg"
    zero_outside(gh, involved, "grad_h")
    zero_outside(gx, involved, "grad_x")        # (h2x: g_out, the identity term, is zero there as well)
    if c.tag == "gen0":
        assert all(float(p.abs().max()) == 0.0 for p in pg) and float(gh.abs().max()) == 0.0
        assert torch.equal(gx, gout) and float(gout.abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["atomics", "edge_rows"])
@pytest.mark.parametrize("hotset", HOTSETS)
@pytest.mark.parametrize("n", SIZES)
def test_x2h_backward_at_regime_boundaries(packed, n, hotset, mode):
    c = make_case("x2h", n, hotset, SEEDS[("x2h", n, hotset)])
    with edge_rows(mode == "edge_rows"):
        run_block(c, packed, f"x2h-{mode} n={n} {hotset}")


@pytest.mark.gpu
@pytest.mark.parametrize("hotset", HOTSETS)
@pytest.mark.parametrize("n", SIZES)
def test_h2x_backward_at_regime_boundaries(packed, n, hotset):
    c = make_case("h2x", n, hotset, SEEDS[("h2x", n, hotset)])
    run_block(c, packed, f"h2x n={n} {hotset}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,count", GEN_COUNTS)
def test_h2x_backward_gen_count_sweep(packed, n, count):
    """the h2x backward's tiles are in the number of listed (gen) rows; count 0: no gradient but the identity term.
    count 1 (the only case whose list does not hold row 0) caught q_backward_mfma_kernel turning the never-written query columns of
    P's row 0, which its padding rows read, into a NaN gamma gradient of the query LayerNorm (0 * NaN instead of a select)."""
    c = make_case("h2x", n, f"gen{count}", SEEDS[("h2x", n, f"gen{count}")])
    assert int(c.gen.sum()) == count
    run_block(c, packed, f"h2x n={n} gen={count}")


@pytest.mark.gpu
@pytest.mark.parametrize("with_grad_x", [False, True], ids=["weights", "weights_and_dx"])
@pytest.mark.parametrize("case", gate_cases(), ids=_id)
def test_gate_backward_stage(packed, case, with_grad_x):
    """gate_bwd_mfma_kernel / gate_bwd_dx_mfma_kernel with their slab fold and reduce-and-store (cbgx_debug_gate_backward of the
    test-only library: the static gate_backward every training step runs) against float64 autograd of OU.edge_gate"""
    c = make_case(*case, SEEDS[case])
    x, nbr, deg, e_w, ei, _, slot = gpu_graph(c, packed)
    ref = oracle(c, ei)
    precondition(c, ref)
    rows = None if c.rows is None else torch.tensor(c.rows, dtype=torch.int32, device=DEV)
    gx = torch.zeros_like(x) if with_grad_x else None
    with _native.first_generation_kernels(0):
        pg = stages.gate_backward(packed, x, nbr, deg, c.gout.to(DEV), rows=rows, grad_x=gx, ws=nan_workspace(c.n), fill=float("nan"))
        torch.cuda.synchronize()
    pairs = [(k, a.reshape(b.shape), b) for k, a, b in zip(ref["keys"], pg, ref["pg"])]
    if with_grad_x:
        pairs.append(("gate grad_x", gx, ref["gx"]))
        zero_outside(gx, set(c.hot) | set(ei[0].tolist()), "gate grad_x")
    check(pairs, f"gate n={c.n} {c.tag} {'dx' if with_grad_x else 'w'}")


if __name__ == "__main__":      # (re)derive SEEDS
    print("SEEDS = {")
    for case in block_cases() + gate_cases():
        print(f"    {case!r}: {find_seed(*case)},", flush=True)
    print("}")
