"""node_query_kernel (q straight from h, no q-hidden columns in P; cbgbench_amd/csrc/node_mfma.hip) against the chain it replaces on
inputs above 8192 rows (node_proj_kernel with the q-hidden chunks -> node_qmlp_kernel): every bit of q, of the eight remaining column
chunks of P, of the folded query and of the denoiser's outputs must be the same.  The forward is compared between fresh child
processes with CBGX_NODE_QDIRECT=1 / 0 (the knob is read once per process), the node stage alone through cbgx_node_stage, whose
``q_direct`` argument selects the kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import stages

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8193              # one row above NODE_STAGE_MAX_ROWS: the smallest input that takes the throughput kernels
FILL = 7.0            # what a node stage does not write keeps this value

_PROBE = r"""
import hashlib, numpy as np, torch
import cbgbench_amd as C
from cbgbench_amd import synthetic
from oracle import weights as W
dev = "cuda:0"
m = C.get_model(C.default_targetdiff_config(13)).eval()
m.load_state_dict(W.synthetic_state_dict(13, 9, seed=0), strict=True)
m = m.to(dev)
def digest(ts):
    torch.cuda.synchronize()
    return " ".join(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16] for t in ts)
# 18 real-size pockets: just above 8192 nodes
batch = synthetic.batch_to(synthetic.denovo_batch(18, seed=5), dev)
st = m.begin_sampling(batch, keep_trajectory=False)
kw = dict(x=st["x"], h=st["h"], batch_idx=st["batch_idx"], lig_flag=st["lig_flag"], gen_flag=st["gen_flag"], graph_ptr=st["graph_ptr"])
n_nodes = st["x"].shape[0]
with torch.no_grad():
    print("PROBE plain", n_nodes, digest(m.denoiser(**kw)))
    xp, hp, lp = m.denoiser(need_h=False, **kw)
    print("PROBE pruned", n_nodes, digest((xp, lp[st["lig_flag"].bool()])))
# three cached sampling steps, part of every ligand fixed (gen_flag False)
rng = np.random.default_rng(6)
pockets = [synthetic.make_pocket(rng, int(n)) for n in rng.integers(420, 560, size=18)]
n_lig = rng.integers(12, 40, size=18)
batch = synthetic.batch_to(synthetic.make_batch(pockets, n_lig, rng, 13, n_ctx_list=rng.integers(1, 9, size=18)), dev)
st = m.begin_sampling(batch, keep_trajectory=False, static_cache=True)
assert st["static_h"] is not None and not bool(st["gen_flag"][st["lig_flag"].bool()].all())
g = torch.Generator(device=dev).manual_seed(9)
nl = batch["ligand_pos"].shape[0]
for t in (999, 998, 400):
    m.denoise_step(st, t, noise=(torch.randn(nl, 3, device=dev, generator=g), torch.rand(nl, 13, device=dev, generator=g)))
print("PROBE cached", st["x"].shape[0], digest((st["x_lig"], st["c_lig"])))
"""


@pytest.fixture(scope="module")
def probes():
    """the probe's lines with the direct kernel and with the chain: {knob: {case: (n_nodes, digests)}}"""
    out = {}
    for knob in ("1", "0"):
        env = dict(os.environ, CBGX_NODE_QDIRECT=knob)
        r = subprocess.run([sys.executable, "-c", _PROBE], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
        out[knob] = {ln[1]: (int(ln[2]), ln[3:]) for ln in lines}
    return out


@pytest.mark.parametrize("case,n_out", [("plain", 3), ("cached", 2), ("pruned", 2)])
def test_forward_is_bit_identical_with_and_without_the_direct_query(probes, case, n_out):
    n_nodes, direct = probes["1"][case]
    assert n_nodes > 8192                      # above NODE_STAGE_MAX_ROWS: the schedules that take the knob
    assert len(direct) == n_out
    assert probes["0"][case] == (n_nodes, direct)


@pytest.fixture(scope="module")
def stage_inputs(synthetic_sd):
    m = C.get_model(C.default_targetdiff_config(13)).eval()
    m.load_state_dict(synthetic_sd, strict=True)
    packed = m.to(DEV).denoiser.packed_weights(torch.device(DEV))
    g = torch.Generator().manual_seed(21)
    h = torch.randn(N, 128, generator=g) * torch.exp(torch.empty(N, 1).uniform_(-2.0, 2.0, generator=g))
    h[5] *= 2.0 ** 20                          # far outside f16's range before the row scale
    h[11] = 0.0                                # the row scale's clamp
    h[N - 1] *= 2.0 ** -20
    lig = (torch.rand(N, generator=g) < 0.3).to(torch.uint8)
    lig[5], lig[11] = 1, 0
    return packed, h.to(DEV), lig.to(DEV)


def _row_lists():
    rng = np.random.default_rng(3)
    special = [5, 11, N - 1]
    lists = {n: np.concatenate([special[:min(n, 3)], rng.choice(np.arange(12, N - 1), size=max(n - 3, 0), replace=False)])[:n]
             for n in (1, 15, 16, 17, 127, 129, 1000)}
    lists[N] = rng.permutation(N)              # every row, gathered through a list
    return lists


ROW_LISTS = _row_lists()
BLOCKS = [(0, True), (4, False), (8, True)]     # (layer, x2h): x2h and h2x blocks of the model


def _check(packed, h, lig, layer, x2h, rows):
    r = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows)).to(torch.int32).to(DEV)
    Pc, qc, Qtc = stages.node_stage(packed, layer, x2h, h, lig, rows=r, q_direct=False, fill=FILL)
    Pd, qd, Qtd = stages.node_stage(packed, layer, x2h, h, lig, rows=r, q_direct=True, fill=FILL)
    torch.cuda.synchronize()
    listed = torch.zeros(N, dtype=torch.bool, device=DEV)
    listed[torch.arange(N, device=DEV) if r is None else r.long()] = True
    assert bool((Pd[:, 512:] == FILL).all())                 # the direct stage does not produce the q-hidden columns ...
    assert not bool((Pc[listed][:, 512:] == FILL).all())     # ... the chain does
    assert torch.equal(qd, qc) and torch.equal(Pd[:, :512], Pc[:, :512]) and torch.equal(Qtd, Qtc)
    assert bool(torch.isfinite(qd).all())
    assert not bool((qd[listed] == FILL).all(1).any())       # every listed row was written,
    assert bool((qd[~listed] == FILL).all())                 # no other row was
    if bool(lig[listed].any()) and not bool(lig[listed].all()):
        return "mixed"
    return "one class"


@pytest.mark.parametrize("layer,x2h", BLOCKS)
def test_node_stage_on_all_rows(stage_inputs, layer, x2h):
    assert _check(*stage_inputs, layer, x2h, None) == "mixed"


@pytest.mark.parametrize("n_rows", sorted(ROW_LISTS))
def test_node_stage_on_a_work_list(stage_inputs, n_rows):
    """lists shorter than one 16-row tile, one tile, one row more, just under and over a workgroup's 128 rows, and all rows permuted;
    from three rows on they hold ligand and protein rows"""
    rows = ROW_LISTS[n_rows]
    assert len(rows) == n_rows == len(set(rows.tolist()))
    for layer, x2h in BLOCKS[:2]:
        kind = _check(*stage_inputs, layer, x2h, rows)
        assert kind == "mixed" or n_rows < 3
