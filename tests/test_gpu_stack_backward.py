"""The whole training backward (csrc/api_train.hip cbgx_unitransformer_backward_ex) BETWEEN its blocks -- listed launches whose grid
comes from n and whose partition from the device-side count, the classifier head's listed and dense backward, the support marking, the
gh / gx ping-pong, the depth switches and every class count -- against float64 autograd on the CPU oracle, through the public module
(UniTransformer with num_layers = L and out_classes = C, x and h requiring grad, a random-weighted score of the outputs).
tests/test_gpu_backward_boundaries.py pins the same kernels one block at a time, with no row list and `count == n`.

Cases, inputs, oracle and criterion: tests/stack_cases.py.  In short: at most 65 hot rows -- gerr on every tensor, without any flip
under the no-near-ReLU precondition where a seed exists (STRICT: 122 of the 234 cases), else against the oracle with ONE verified ReLU
flip, or, where no single flip explains every tensor, with the SET of flips that the LayerNorm-bias gradients name, verified together
in one oracle run (every unit of the set lies inside FLIP_EPS).  On the MI355X 2 of the 102 such cases needed a set, of two units
(grid-2100-3-13-lo-63-0 / -1: blocks.0 hv_func edge 14548 unit 102 with blocks.1 hk_func edge 17123 unit 44; each alone leaves 6 - 62
entries of the other MLP's first-Linear gradient at 2 - 5 x gerr's floor), 21 ONE flip, the others none.  2048 / 2049 hot rows --
relative L2 plus the row-wise bound (which is what sees one missing or doubled row there), with ONE verified flip in the one-layer
head cases and ONE flip or the verified SET in the three-layer list cases (2048 rows: sets of four to six).  The head sensitivity precondition of
tests/test_stack_cases.py covers the lists of at most 65 rows.

Three breaks of the sources, by reading, and the cases that catch them.  (1) ssp_backward_rows_kernel without its last listed row: that
row of dpre keeps the 0xFF fill, the listed wgrad / colsum / dgrad read it, and every head case with R >= 1 fails on a non-finite
gradient (head-600-1-13-lo-1: the only row).  (2) `n_nodes` for `count` in the listed x2h partition (train_bwd_x2h.hip, `const int
count = rows ? *n_rows_ptr : n_nodes`): the waves walk list entries past the count, which hold the 0xFF fill, so every grid case with
R < n fails (grid-600-3-13-lo-9-0: 591 such entries).  (3) cls_w1_grad_rows_kernel without its remainder loop: below 25 rows every row
is in the remainder, classifier.2.weight comes back zero (head-600-1-13-lo-1 ... -17), and from 25 rows on the rows after the last
full group of 32 are lost (R = 31, 33, 63, 65), which gerr sees under the sensitivity precondition.

Poison: module.train_workspace(N) is filled with 0xFF bytes before the forward and again between the forward and the backward
(include/cbgx.h: the backward takes everything from the tape); every gradient output is a torch.empty of the autograd bridge.  Graphs
without a hot row must come back with exactly zero x.grad / h.grad, every value must be finite.

Not covered (n <= 4200 here): the MAX_SPLITS cap at 65 536 rows and the node-GEMM grid switch at 8193 rows need an oracle that
evaluates the receptive field only.  The DiffBP h2x stack driver and the inference forward are pinned elsewhere.

Wall time of the whole file on an MI355X with 16 CPU threads for the oracle (234 cases): about 100 s.  A case of 600 rows and three
layers takes 1.3 s (the float64 oracle), and one more oracle run when it has to verify a flip; the six three-layer cases of 2048 /
2049 rows 5 - 10 s each (the oracle on all 2100 rows: 5 s a run)."""
import contextlib
import functools
import os

import pytest
import torch

import cbgbench_amd as CB
from cbgbench_amd.unitransformer import UniTransformer
from tests import stack_cases as S
from tests.test_gpu_backward_boundaries import ratio
from tests.test_gpu_coord_grad import TOL, env, failures, rel_err
from tests.test_gpu_parity import close
from tests.test_gpu_training import gerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=3)
def module(C, L):
    cfg = CB.get_model(CB.default_targetdiff_config(13)).denoiser.cfg
    d = dict(cfg)
    d.update(num_layers=L, num_classes=C)
    den = UniTransformer(type(cfg)(d))
    den.load_state_dict({k[len("denoiser."):]: v for k, v in S.state_dict(C, L).items()}, strict=True)
    return den.to(DEV)


@functools.lru_cache(maxsize=2)
def reference(input_key, seed):
    """(case, plain oracle result): shared by the variants (edge rows, dense head) and modes that have the same inputs"""
    k = S.StackKey(*input_key[:7], "", input_key[7])
    c = S.build(k, seed)
    return c, S.oracle(c)


def variant_env(k):
    if k.variant == "edge_rows":
        return env(CBGX_BX_EDGE_ROWS="1")
    if k.variant == "dense":
        return env(CBGX_TRAIN_PRUNE_GH="0")
    return contextlib.nullcontext()


def gpu_run(k, c):
    """forward + backward through the module on a poisoned workspace -> (got {"x", "h", parameter name: gradient}, logits)"""
    den = module(k.C, k.L)
    den.zero_grad(set_to_none=True)
    x = c.x.to(DEV).clone().requires_grad_(True)
    h = c.h.to(DEV).clone().requires_grad_(True)
    kw = {"lo": {"ligand_outputs_only": True}, "src": {"h_on_sources": True}, "full": {}}[k.mode]
    ws = den.train_workspace(c.n, torch.device(DEV))
    with variant_env(k):
        ws.fill_(0xFF)
        xo, ho, lo = den(x, h, c.batch.to(DEV), c.lig.to(DEV), c.gen.to(DEV), graph_ptr=c.graph_ptr.to(DEV), **kw)
        assert den.train_workspace(c.n, torch.device(DEV)) is ws
        ws.fill_(0xFF)
        s = S.score(xo, None if k.mode == "lo" else ho, lo, (c.wx, c.wl, None if k.mode == "lo" else c.wh))
        s.backward()
        torch.cuda.synchronize()
    got = {"x": x.grad, "h": h.grad}
    got.update({name: p.grad for name, p in den.named_parameters()})
    return got, lo.detach()


def l2_deviations(got, ref):
    """messages of `failures` (relative L2: TOL for x / h, 1e-3 for parameters) and of the row-wise bound on x.grad and h.grad"""
    out = list(failures(got, ref).values())
    for name in ("x", "h"):
        out += S.row_failures(got[name], ref[name], f"{name}.grad")[1]
    return out


def gerr_deviations(got, ref):
    """messages of gerr at its defaults, every tensor"""
    out = []
    for name, b in ref.items():
        if name.endswith("k_func.net.3.bias"):      # the key bias cancels in the softmax: exactly zero here, round-off in autograd
            if float(got[name].abs().max()) != 0.0:
                out.append(f"{name}: not exactly zero")
            continue
        msg = gerr(got[name], b, name)
        if msg:
            out.append(msg)
    return out


def worst_ratio(got, ref, elementwise):
    if elementwise:
        return max(ratio(got[name], b) for name, b in ref.items() if not name.endswith("k_func.net.3.bias"))
    worst = max([rel_err(got[name], b) / (TOL if name in ("x", "h") else S.PARAM_TOL) for name, b in ref.items()
                 if float(b.double().norm()) >= 1e-9], default=0.0)
    return max([worst] + [S.row_failures(got[name], ref[name], name)[0] for name in ("x", "h")])


def check_with_flips(got, c, res, label, deviations, allow_set):
    """plain comparison, or verified ReLU flips.  The near-zero units that flipped are named by S.select_flips.  ONE of them on the other
    side of zero in the oracle must reproduce every tensor within the plain tolerances (each is tried alone, heaviest first); where
    `allow_set`, else all of them together in ONE oracle run."""
    bad = deviations(got, res["ref"])
    if not bad:
        return res["ref"]
    force = S.select_flips(got, res)
    units = sorted(((p, r, u) for p, lst in force.items() for r, u in lst), key=lambda t: -abs(res["flipdelta"][t]))
    assert units, f"{label}: {bad[:6]} (and the LayerNorm-bias gradients show no flipped near-zero unit)"
    still = bad
    for p, r, u in units if len(units) <= 2 or not allow_set else []:      # (three or more named: no single one can explain all)
        ref = S.oracle(c, force={p: [(r, u)]})["ref"]
        still = deviations(got, ref)
        if not still:
            print(f"ReLU flips verified: {label}: ONE unit {(p, r, u)} explains {len(bad)} deviation(s) ({len(units)} named)")
            return ref
    assert allow_set and len(units) > 1, f"{label}: {still[:6]} (not explained by ONE flip among {units[:6]}; plain: {bad[:3]})"
    ref = S.oracle(c, force=force)["ref"]
    still = deviations(got, ref)
    assert not still, f"{label}: {still[:6]} (not explained by flipping {units[:8]} together; plain: {bad[:3]})"
    print(f"ReLU flips verified: {label}: the SET of {len(units)} units {units[:8]} explains {len(bad)} deviation(s)")
    return ref


def run_case(k):
    seed = S.seed_of(k)
    c, res = reference(S.input_key(k), seed)
    a1, a2 = S.list_sizes(c)
    label = S.key_id(k)
    print(f"LISTS {label}: |A1| = {a1} |A2| = {a2} head rows = {len(S.head_rows(c))} gen rows = {int(c.gen.sum())} seed = {seed}")
    got, logits = gpu_run(k, c)
    ref = res["ref"]
    for name, t in got.items():
        assert t is not None, f"{label} {name}: no gradient"
        assert bool(torch.isfinite(t).all()), f"{label} {name}: not finite (read before written?)"
    # graphs without a hot row carry an exactly zero gradient
    cold = torch.ones(c.n, dtype=torch.bool)
    cold[res["rows"]] = False
    if bool(cold.any()):
        for name in ("x", "h"):
            assert float(got[name][cold.to(DEV)].abs().sum()) == 0.0, f"{label} {name}.grad: non-zero in a graph without a hot row"
    elementwise = k.R <= S.STRICT_MAX_HOT
    if S.is_strict(k):
        assert not S.carrying_near(c, res), f"{label}: the seed table is stale (python -m tests.stack_cases)"
        msgs = gerr_deviations(got, ref)
        print(f"RATIO {label} worst error / tolerance (gerr, strict) = {worst_ratio(got, ref, True):.3f}")
        assert not msgs, (label, msgs)
    else:
        # <= 65 hot rows: gerr with ONE flip, else the set; 2048 / 2049: relative L2 + rows with ONE flip, three layers: else the set
        ref = check_with_flips(got, c, res, label, gerr_deviations if elementwise else l2_deviations, elementwise or k.L > 1)
        print(f"RATIO {label} worst error / tolerance ({'gerr' if elementwise else 'relative L2, rows'}) = "
              f"{worst_ratio(got, ref, elementwise):.3f}")
    return c, res, got, logits


def exactly_zero(got, names, label):
    for name in names:
        assert float(got[name].abs().max()) == 0.0 and bool(torch.isfinite(got[name]).all()), f"{label} {name}: not exactly zero"


@pytest.mark.parametrize("k", S.cases_list_vs_grid(), ids=S.key_id)
def test_list_count_against_grid(k):
    """three layers, ligand_outputs_only: the last two x2h blocks walk A1 / A2 with a grid sized from n (6, 72, 256 workgroups) and a
    partition computed from the device-side count; g > 0 gives the h2x blocks and dp_rows work; edge_rows: the listed blocks keep
    atomics, the full-launch block uses edge rows"""
    run_case(k)


@pytest.mark.parametrize("k", S.cases_head_listed(), ids=S.key_id)
def test_classifier_head_backward_listed(k):
    """one layer: cls_w1_grad_rows_kernel (8 row groups, 4 at a time), ssp_backward_rows_kernel (2048-row grid cap), the listed node
    GEMMs, colsum, wgrad and dgrad on the lig_flag rows ("lo") or on the marked support of grad_logits ("full": protein rows too).
    2048 / 2049 rows: a missing row shows in the row-wise bound on h.grad."""
    c, res, got, _ = run_case(k)
    if k.mode == "full" and k.R:
        assert bool((~c.lig[c.hot]).any())


@pytest.mark.parametrize("k", S.cases_head_dense(), ids=S.key_id)
def test_classifier_head_backward_dense(k):
    """CBGX_TRAIN_PRUNE_GH=0, a caller gradient on h_out: sgemm with M = C / K = C, splits_for(n), colsum's second pass, node_grid's cap"""
    run_case(k)


@pytest.mark.parametrize("k", S.cases_classes(), ids=S.key_id)
def test_every_class_count(k):
    """C on both sides of sgemm's 16-wide K staging and 64-wide tiles, node_linear_kernel's 16-column tiles and the two 64-lane halves
    of mark_nonzero_rows_kernel; the taped forward's logits against the oracle on the rows that are defined"""
    c, res, got, logits = run_case(k)
    rows = torch.tensor(S.head_rows(c) if k.mode == "lo" else res["rows"].tolist())
    pos = {r: i for i, r in enumerate(res["rows"].tolist())}
    close(logits[rows.to(DEV)], res["logits"][[pos[r] for r in rows.tolist()]], f"taped logits [C={k.C} {k.mode}]")


@pytest.mark.parametrize("k", S.cases_depth(), ids=S.key_id)
def test_depth_switches(k):
    """L < 3: no pruning; L = 10 / 11: one / two weight-pack passes; L = 33: the shared query-LayerNorm slot, auxiliary stream off"""
    run_case(k)


@pytest.mark.parametrize("k", S.cases_absent(), ids=S.key_id)
def test_absent_gradients(k):
    """NULL grad_logits / grad_x_out branches and an empty head list: the tensors that cannot get a gradient are exactly zero"""
    c, res, got, _ = run_case(k)
    label = S.key_id(k)
    cls = [n for n in got if n.startswith("classifier.")]
    assert len(cls) == 4
    if "l" not in k.loss:
        exactly_zero(got, cls, label)
    if k.loss == "l" and k.L == 1:
        h2x = [n for n in got if ".h2x_layers." in n]
        assert len(h2x) == 18
        exactly_zero(got, h2x, label)
    if k.R == 0:
        exactly_zero(got, list(got), label)
