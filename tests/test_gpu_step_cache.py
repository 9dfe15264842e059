"""The step cache of the static-context forward (cbgx_unitransformer_forward_step_cached, include/cbgx.h): a trajectory of denoiser
calls on one sampling state, with the block, against the same calls without it (cbgx_unitransformer_forward_cached: the launches that
CBGX_STEP_CACHE=0 selects).  Every comparison is torch.equal.

Shapes: 20 synthetic pockets of 450 - 550 atoms, one sample each -- about 10.5 k nodes, the smallest round size above the 8 192 rows at
which the large-input schedule (and with it the cache) begins.  Between calls the test moves the ligands itself: a jitter (rows enter
and leave D1 / D2), two compact placements at opposite ends of the pocket (the protein parts of D1(t) and D1(t-1) are disjoint), a
placement 100 A away (D1 = the ligand rows alone), back to the start (rows enter again) and a repeat (nothing changes).  Every call gets
a fresh workspace of 0xFF bytes; every block is filled with 0xFF before its reset.  D1(t) / D2(t) are read from the block's own flag
arrays after the call, for the coverage assertions and for the rows to poison only."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, stages, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CALLS = 7
# the flag combinations with which the three samplers reach the cached path (TargetDiff and DiffSBDD: pruned, no h'; DiffBP: h' on the
# CoM stack's source rows), and the unpruned call, whose h' and logits are defined on every row
COMBOS = {"targetdiff_diffsbdd": dict(need_h=False), "diffbp": dict(need_h=True, h_on_sources=True), "unpruned": dict(need_h=True)}


@pytest.fixture(scope="module")
def model(synthetic_sd):
    m = C.get_model(C.default_targetdiff_config(13)).eval()
    m.load_state_dict(synthetic_sd, strict=True)
    return m.to(DEV)


def poisoned_workspace(st):
    return torch.full((int(_native.lib().cbgx_workspace_bytes(st["N"], st["B"])),), 0xFF, dtype=torch.uint8, device=DEV)


def poisoned_block(model, st):
    """a block whose memory held 0xFF bytes (NaN) before the reset: a fresh state must not read a previous run's rows"""
    lib = _native.lib()
    need = lib.cbgx_step_cache_bytes(st["N"])
    if need == 0 and os.environ.get("CBGX_STEP_CACHE", "1") == "0":
        pytest.skip("CBGX_STEP_CACHE=0 in the environment: no block to test")
    assert need > 0, "the test shape must take the large-input schedule"
    block = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    _native.check(lib.cbgx_step_cache_reset(_native.ptr(block), need, st["N"], _native.current_stream(torch.device(DEV))), "reset")
    return block


def block_views(block, n):
    off = (ctypes.c_size_t * 9)()
    _native.check(_native.lib().cbgx_step_cache_layout(n, off), "layout")
    f32 = lambda o, cols: block[o:o + n * cols * 4].view(torch.float32).view(n, cols)
    names = ["P0", "q0", "h1", "P1", "q1", "h2"]
    v = {k: f32(off[i], 640 if k[0] == "P" else 128) for i, k in enumerate(names)}
    v.update({k: block[off[6 + i]:off[6 + i] + n] for i, k in enumerate(["fresh0", "prevD1", "prevD2"])})
    return v


_STATES = {}


def state(model, seed):
    """a TargetDiff sampling state on the test shape (made once per seed, left unchanged) and the ligand placements of the trajectory"""
    if seed in _STATES:
        return _STATES[seed]
    batch = synthetic.batch_to(synthetic.denovo_batch(20, seed=seed, n_rec_range=(450, 550), n_lig_range=(10, 20)), DEV)
    with torch.no_grad():
        st = model.begin_sampling(batch, keep_trajectory=False)
    assert st["static_h"] is not None and st["N"] > 8192 and st["gen_is_ligand"]
    rows = st["lig_rows"]
    g = torch.Generator().manual_seed(100 + seed)
    x0 = st["x_lig"].clone()
    unit = torch.randn(x0.shape, generator=g).to(DEV)
    com = torch.zeros(st["B"], 3, device=DEV).index_add_(0, st["bl"], x0) / torch.bincount(st["bl"], minlength=st["B"]).clamp(min=1)[:, None]
    compact = 0.3 * (x0 - com[st["bl"]])
    shift = lambda dx: compact + torch.tensor([dx, 0.0, 0.0], device=DEV)
    placements = [x0, x0 + 0.7 * unit, shift(9.0), shift(-9.0), shift(100.0), x0, x0]
    with torch.no_grad():      # (the state's own ligand rows of h are written by its first step: not yet)
        emb = model.context_embedder.embed_ligand(st["c_lig"]).float()
    assert bool(torch.isfinite(emb).all()) and bool(torch.isfinite(st["x"][st["rec_rows"]]).all()) and bool(torch.isfinite(st["h"][st["rec_rows"]]).all())
    h_lig = [emb * (1.0 + 0.05 * k) for k in range(N_CALLS)]
    st["_x0"], st["_h0"], st["_placements"], st["_h_lig"] = st["x"].clone(), st["h"].clone(), placements, h_lig
    _STATES[seed] = st
    return st


def call(model, st, k, block, combo, x=None, h=None):
    """call k of the trajectory on a fresh poisoned workspace -> (x', h', logits)"""
    rows = st["lig_rows"]
    x = st["_x0"].clone() if x is None else x
    h = st["_h0"].clone() if h is None else h
    x[rows] = st["_placements"][k]
    h[rows] = st["_h_lig"][k]
    with torch.no_grad():
        return model.denoiser(x=x, h=h, batch_idx=st["batch_idx"], lig_flag=st["lig_flag"], gen_flag=st["gen_flag"], graph_ptr=st["graph_ptr"],
                              static_h=st["static_h"], workspace=poisoned_workspace(st), gen_is_ligand=True, step_cache=block, **COMBOS[combo])


def a1_rows(st, k):
    """gen | lig | in-neighbours of gen rows in call k's graph: where an h_on_sources call defines h' (include/cbgx.h)"""
    x = st["_x0"].clone()
    x[st["lig_rows"]] = st["_placements"][k]
    nbr, deg = stages.knn_graph(x, st["graph_ptr"])
    gen = st["gen_flag"].bool()
    src = nbr[gen][torch.arange(32, device=DEV)[None, :] < deg[gen][:, None]].long()
    a1 = gen | st["lig_flag"].bool()
    a1[src] = True
    return a1


def assert_same(got, ref, st, combo, what, k):
    (x2, h2, l2), (x1, h1, l1) = got, ref
    lig = st["lig_flag"]
    assert torch.equal(x2, x1), f"{what}: x_out differs on {int((x2 != x1).any(1).sum())} rows"
    assert torch.equal(l2[lig], l1[lig]), f"{what}: ligand logits differ"
    if combo == "unpruned":
        assert torch.equal(h2, h1) and torch.equal(l2, l1), f"{what}: h_out / logits of the unpruned call differ"
    elif combo == "diffbp":
        a1 = a1_rows(st, k)      # (rows outside A1 are left unwritten)
        assert bool(a1[lig].all()) and torch.equal(h2[a1], h1[a1]), f"{what}: h_out differs on {int((h2[a1] != h1[a1]).any(1).sum())} rows of A1"
    else:
        assert h2 is None and h1 is None


_REFERENCE = {}


def reference(model, st, seed, combo):
    """the trajectory without the block, computed once per (state, flags) and shared"""
    key = (seed, combo)
    if key not in _REFERENCE:
        _REFERENCE[key] = [call(model, st, k, None, combo) for k in range(N_CALLS)]
        for xo, _, lo in _REFERENCE[key]:
            assert bool(torch.isfinite(xo).all()) and bool(torch.isfinite(lo[st["lig_flag"]]).all())
    return _REFERENCE[key]


@pytest.mark.parametrize("combo", list(COMBOS))
def test_trajectory_is_bit_equal_to_the_calls_without_the_block(model, combo):
    st = state(model, 1)
    ref = reference(model, st, 1, combo)
    block = poisoned_block(model, st)
    v = block_views(block, st["N"])
    lig = st["lig_flag"]
    d1, d2 = [], []
    for k in range(N_CALLS):
        assert_same(call(model, st, k, block, combo), ref[k], st, combo, f"call {k}", k)
        d1.append(v["prevD1"].bool().clone())
        d2.append(v["prevD2"].bool().clone())
        assert not bool(v["fresh0"].any())
        assert bool(d1[k][lig].all()) and bool(d2[k][d1[k]].all())
    if combo == "targetdiff_diffsbdd":      # what the placements were chosen for
        prot = ~lig
        assert bool((d1[1] & ~d1[0] & prot).any()) and bool((d1[0] & ~d1[1] & prot).any()), "the jitter moves rows into and out of D1"
        assert bool((d1[2] & prot).any()) and bool((d1[3] & prot).any()) and not bool((d1[2] & d1[3] & prot).any()), "disjoint D1(t), D1(t-1)"
        assert bool((d2[3] & ~d2[2]).any()) and bool((d2[2] & ~d2[3]).any())
        assert torch.equal(d1[4], lig), "a ligand far from every protein atom: D1 holds the ligand rows only"
        assert torch.equal(d1[5], d1[0]) and torch.equal(d1[6], d1[0]) and bool((d1[5] & prot).any())


def test_rows_a_call_recomputes_do_not_need_their_old_values(model):
    """before call t the block's rows that the call computes or places again are overwritten with NaN: P1 / q1 / h1 on D1(t-1) | D1(t), h2
    on D2(t-1) | D2(t), P0 / q0 on the ligand rows.  (Every other row is the cache: it is needed.)"""
    combo = "targetdiff_diffsbdd"
    st = state(model, 1)
    ref = reference(model, st, 1, combo)
    block = poisoned_block(model, st)
    v = block_views(block, st["N"])
    d1, d2 = [], []
    for k in range(N_CALLS):      # first run: the sets of every call
        call(model, st, k, block, combo)
        d1.append(v["prevD1"].bool().clone())
        d2.append(v["prevD2"].bool().clone())
    block = poisoned_block(model, st)
    v = block_views(block, st["N"])
    nan = float("nan")
    for k in range(N_CALLS):
        if k > 0:
            r1, r2 = d1[k - 1] | d1[k], d2[k - 1] | d2[k]
            for name in ("P1", "q1", "h1"):
                v[name][r1] = nan
            v["h2"][r2] = nan
            v["P0"][st["lig_flag"]] = nan
            v["q0"][st["lig_flag"]] = nan
        assert_same(call(model, st, k, block, combo), ref[k], st, combo, f"call {k}", k)


@pytest.mark.parametrize("two_streams", [False, True])
def test_two_states_stepped_alternately_give_the_bits_of_each_alone(model, two_streams):
    combo = "targetdiff_diffsbdd"
    sts = [state(model, 1), state(model, 2)]
    refs = [reference(model, st, seed, combo) for st, seed in zip(sts, (1, 2))]
    blocks = [poisoned_block(model, st) for st in sts]
    cur = torch.cuda.current_stream(torch.device(DEV))
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)] if two_streams else [cur, cur]
    for s in streams:
        s.wait_stream(cur)
    outs = [[], []]
    for k in range(N_CALLS):
        for i, st in enumerate(sts):
            with torch.cuda.stream(streams[i]):
                outs[i].append(call(model, st, k, blocks[i], combo))
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    for i, st in enumerate(sts):
        for k in range(N_CALLS):
            assert_same(outs[i][k], refs[i][k], st, combo, f"state {i} call {k}", k)


def test_a_new_state_gets_a_new_block_and_the_samplers_pass_it(model):
    st = state(model, 1)
    poisoned_block(model, st)
    assert st["step_cache"] is not None and st["step_cache"].numel() == _native.lib().cbgx_step_cache_bytes(st["N"])
    v = block_views(st["step_cache"], st["N"])
    assert bool(v["fresh0"].all()) and bool(v["prevD1"].all()) and bool(v["prevD2"].all()), "reset: every row is still to compute"
    batch = synthetic.batch_to(synthetic.denovo_batch(2, seed=3, n_rec_range=(120, 160), n_lig_range=(8, 14)), DEV)
    with torch.no_grad():
        assert model.begin_sampling(batch, keep_trajectory=False)["step_cache"] is None, "small inputs take the fused schedule: no block"


_KNOB_SCRIPT = """
import hashlib, sys, torch
sys.path.insert(0, {root!r})
from tests import test_gpu_step_cache as T
from oracle import weights as W
import cbgbench_amd as C
m = C.get_model(C.default_targetdiff_config(13)).eval()
m.load_state_dict(W.synthetic_state_dict(13, 9, seed=0), strict=True)
m = m.to(T.DEV)
batch = T.synthetic.batch_to(T.synthetic.denovo_batch(20, seed=1, n_rec_range=(450, 550), n_lig_range=(10, 20)), T.DEV)
with torch.no_grad():
    st = m.begin_sampling(batch, keep_trajectory=False)
print("BLOCK", st["step_cache"] is not None)
hsh = hashlib.sha256()
for t in (3, 2, 1):
    m.denoise_step(st, t, noise=(torch.zeros_like(st["x_lig"]), torch.full_like(st["c_lig"], 0.5)))
    hsh.update(st["x_lig"].cpu().numpy().tobytes()); hsh.update(st["c_lig"].cpu().numpy().tobytes())
print("DIGEST", hsh.hexdigest())
"""


def test_knob_off_gives_the_same_sampler_steps(synthetic_sd):
    """three TargetDiff steps on the test shape in two fresh processes, default and CBGX_STEP_CACHE=0 (read once per process): the knob
    drops the block, and the ligand states after every step have the same bytes"""
    from oracle import weights as W
    assert all(torch.equal(v, synthetic_sd[k]) for k, v in W.synthetic_state_dict(13, 9, seed=0).items()), "the script's weights"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for knob in ("1", "0"):
        env = dict(os.environ, CBGX_STEP_CACHE=knob)
        r = subprocess.run([sys.executable, "-c", _KNOB_SCRIPT.format(root=root)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[knob] = dict(line.split(" ", 1) for line in r.stdout.splitlines() if line.startswith(("BLOCK", "DIGEST")))
    assert out["1"]["BLOCK"] == "True" and out["0"]["BLOCK"] == "False"
    assert out["1"]["DIGEST"] == out["0"]["DIGEST"]
