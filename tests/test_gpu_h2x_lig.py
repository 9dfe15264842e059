"""The ligand-row h2x edge kernel (csrc/edge_h2x_lig.hip: the query folded in registers, no folded rows Qt) against the general h2x
kernel behind node_qfold_kernel, through the C ABI: `stages.h2x_attention(..., gen_is_ligand=True)` (cbgx_h2x_attention_v2) and one whole
4-layer forward (`stages.unitransformer_forward`, cbgx_unitransformer_forward_v2) with CBGX_FWD_GEN_IS_LIGAND.

CBGX_H2X_FOLD is read once per process, so the two kernels run in two child processes (one for the whole module): this file run as
a script computes every case with and without the flag and writes the results to an .npz file.

Shapes: one graph of 34 nodes with one movable atom; a 20-node graph (degree 19: invalid slots point at the node itself); ligand atoms
whose 32 neighbours are all ligand atoms (no protein-source pass) / all protein atoms (no ligand-source pass); work lists of 0, 1,
255, 256 and 257 rows; a linker batch (some ligand atoms fixed); and the flag not set, where the general kernel and the fold kernel
run whatever CBGX_H2X_FOLD says.

Yardstick.  The two paths are not bit-identical on the MI355X: node_qfold_kernel sums the eight products of a folded value in two
16x16x4 fp32 MFMA steps (d = 0, 2, 4, 6, then d = 1, 3, 5, 7), the register fold as one FMA chain over d = 0 .. 7 -- the outputs differ
in the last bit or two (max |difference| 4e-9 .. 1.2e-7 on displacements of order 1, 2.4e-7 on the coordinates of a 4-layer
forward).  So both paths are compared with the CPU oracle in fp64 on the same inputs, and the fold path's maximum error may be at
most 1.5 x the general path's (one extra rounding).  Measured figures: DESIGN.md 9."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
LIST_LENGTHS = (0, 1, 255, 256, 257)
BLOCK_CASES = ("one_movable_34", "deg19", "all_lig_nbrs", "all_prot_nbrs", "linker") + tuple(f"list{k}" for k in LIST_LENGTHS)
FORWARD_CASES = ("fwd_2graphs", "fwd_linker")

pytestmark = pytest.mark.gpu


# ---- inputs (CPU tensors; the same in every process) ------------------------------------------------------------------------------
def _cloud(gen, n, centre, sigma):
    return torch.tensor(centre) + torch.randn(n, 3, generator=gen) * sigma


def _shell(gen, n, centre, r0, r1):
    d = torch.randn(n, 3, generator=gen)
    return torch.tensor(centre) + d / d.norm(dim=1, keepdim=True) * (r0 + (r1 - r0) * torch.rand(n, 1, generator=gen))


def block_inputs():
    """name -> (x, h, lig, gen, batch): layer-0 h2x block inputs"""
    gen = torch.Generator().manual_seed(11)
    out = {}

    def add(name, x, lig, movable, batch):
        out[name] = (x.float(), torch.randn(x.shape[0], 128, generator=gen), lig, movable & lig, batch)

    lig = torch.zeros(34, dtype=torch.bool); lig[30:] = True
    mov = torch.zeros(34, dtype=torch.bool); mov[31] = True
    add("one_movable_34", _cloud(gen, 34, [0.0, 0.0, 0.0], 2.5), lig, mov, torch.zeros(34, dtype=torch.long))
    lig = torch.zeros(20, dtype=torch.bool); lig[15:] = True
    add("deg19", _cloud(gen, 20, [0.0, 0.0, 0.0], 2.5), lig, lig.clone(), torch.zeros(20, dtype=torch.long))
    # 40 ligand atoms in a tight cluster, 25 protein atoms on a shell 8 - 10 A away: every ligand atom's 32 neighbours are ligand atoms
    x = torch.cat([_shell(gen, 25, [0.0, 0.0, 0.0], 8.0, 10.0), _cloud(gen, 40, [0.0, 0.0, 0.0], 0.6)])
    lig = torch.zeros(65, dtype=torch.bool); lig[25:] = True
    add("all_lig_nbrs", x, lig, lig.clone(), torch.zeros(65, dtype=torch.long))
    # one ligand atom inside 45 protein atoms
    x = torch.cat([_cloud(gen, 45, [0.0, 0.0, 0.0], 2.5), torch.zeros(1, 3)])
    lig = torch.zeros(46, dtype=torch.bool); lig[45] = True
    add("all_prot_nbrs", x, lig, lig.clone(), torch.zeros(46, dtype=torch.long))
    z = np.load(os.path.join(GOLDEN, "denoiser_linker.npz"))
    out["linker"] = tuple(torch.from_numpy(z[k]) for k in ("x", "h_layer0", "lig_flag", "gen_flag", "batch_idx"))
    # nine graphs of 12 protein + 30 ligand atoms: 270 ligand atoms, of which the first k move
    xs, ligs, batch = [], [], []
    for b in range(9):
        xs += [_cloud(gen, 12, [40.0 * b, 0.0, 0.0], 2.5), _cloud(gen, 30, [40.0 * b, 0.0, 0.0], 1.5)]
        ligs += [torch.zeros(12, dtype=torch.bool), torch.ones(30, dtype=torch.bool)]
        batch += [b] * 42
    x, lig, batch = torch.cat(xs), torch.cat(ligs), torch.tensor(batch)
    h = torch.randn(x.shape[0], 128, generator=gen)
    rows = torch.nonzero(lig).flatten()
    for k in LIST_LENGTHS:
        mov = torch.zeros_like(lig); mov[rows[:k]] = True
        out[f"list{k}"] = (x.float(), h, lig, mov, batch)
    return out


def forward_inputs():
    out = {}
    for name, case in (("fwd_2graphs", "denoiser_2graphs"), ("fwd_linker", "denoiser_linker")):
        z = np.load(os.path.join(GOLDEN, case + ".npz"))
        out[name] = tuple(torch.from_numpy(z[k]) for k in ("x", "h", "lig_flag", "gen_flag", "batch_idx"))
    return out


def h2x_qt_region(n):
    """byte range of the folded rows the h2x blocks of a fused-schedule forward use (csrc/api.hip carve: 256-byte aligned regions
    nbr | deg | e_w | three sets of (P, Qt, q); the h2x blocks take set 2): pinned by tests/golden/workspace_layout.json"""
    a = lambda v: (v + 255) & ~255
    sets = a(n * 32 * 4) + a(n * 4) + a(n * 32 * 4)
    one = a(n * 640 * 4) + a(n * 16 * 128 * 4) + a(n * 128 * 4)
    begin = sets + 2 * one + a(n * 640 * 4)
    return begin, begin + n * 16 * 128 * 4


# ---- the child process ------------------------------------------------------------------------------------------------------------
def _worker(path):
    import cbgbench_amd as C
    from cbgbench_amd import _native, stages
    from cbgbench_amd.unitransformer import graph_ptr_from_batch
    from oracle import weights
    res = {}
    u8 = lambda t: t.to(DEV).to(torch.uint8)
    m = C.get_model(C.default_targetdiff_config(13, num_layers=4)).eval()
    m.load_state_dict(weights.synthetic_state_dict(13, 4, seed=0), strict=True)
    m = m.to(DEV)
    packed = m.denoiser.packed_weights(torch.device(DEV))
    graphs = {}
    for name, (x, h, lig, mov, batch) in block_inputs().items():
        xd = x.to(DEV)
        key = (x.shape[0], float(x.sum()))
        if key not in graphs:       # (the list-length cases share one graph)
            nbr, deg = stages.knn_graph(xd, graph_ptr_from_batch(batch.to(DEV)))
            graphs[key] = (nbr, deg, stages.edge_gate(packed, xd, nbr, deg))
        nbr, deg, e_w = graphs[key]
        res[f"{name}.nbr"], res[f"{name}.deg"], res[f"{name}.e_w"] = nbr.cpu().numpy(), deg.cpu().numpy(), e_w.cpu().numpy()
        for flag in (1, 0):
            xo, dx = stages.h2x_attention(packed, 0, xd, h.to(DEV), nbr, deg, u8(lig), u8(mov), e_w, gen_is_ligand=bool(flag))
            res[f"{name}.x_out.{flag}"], res[f"{name}.dx.{flag}"] = xo.cpu().numpy(), dx.cpu().numpy()
    for name, (x, h, lig, mov, batch) in forward_inputs().items():
        n = x.shape[0]
        gp = graph_ptr_from_batch(batch.to(DEV))
        lo, hi = h2x_qt_region(n)
        for flag in (1, 0):
            ws = torch.full((_native.lib().cbgx_workspace_bytes(n, int(gp.numel()) - 1),), 0xFF, dtype=torch.uint8, device=DEV)
            xo, ho, lg = stages.unitransformer_forward(packed, 4, 13, x.to(DEV), h.to(DEV), gp, u8(lig), u8(mov), ws=ws,
                                                       gen_is_ligand=bool(flag))
            res[f"{name}.x_out.{flag}"], res[f"{name}.h_out.{flag}"] = xo.cpu().numpy(), ho.cpu().numpy()
            res[f"{name}.logits.{flag}"] = lg.cpu().numpy()
            res[f"{name}.qt_untouched.{flag}"] = np.array(bool((ws[lo:hi] == 0xFF).all()))
    np.savez(path, **res)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{"fold": results of a process with the default, "plain": of one with CBGX_H2X_FOLD=0}"""
    out = {}
    for key, knob in (("fold", None), ("plain", "0")):
        path = str(tmp_path_factory.mktemp("h2x_lig") / f"{key}.npz")
        env = {k: v for k, v in os.environ.items() if k != "CBGX_H2X_FOLD"}
        if knob is not None:
            env["CBGX_H2X_FOLD"] = knob
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, cwd=ROOT, timeout=300)
        out[key] = dict(np.load(path))
    return out


# ---- the fp64 oracle of a block case (CPU) ------------------------------------------------------------------------------------------
MARGIN = 1.5      # new path's max error <= MARGIN x the old path's: one extra rounding


def assert_no_worse(new, old, ref64, what):
    if new.numel() == 0:      # an empty work list: nothing moved
        assert old.numel() == 0 and ref64.numel() == 0, what
        return
    e_new, e_old = float((new.double() - ref64).abs().max()), float((old.double() - ref64).abs().max())
    print(f"{what}: max |fold - plain| {float((new - old).abs().max()):.3e}; error against fp64: fold {e_new:.3e}, plain {e_old:.3e}")
    assert bool(torch.isfinite(new).all()), what
    assert e_new <= MARGIN * e_old, f"{what}: fold path {e_new:.3e} against fp64, general path {e_old:.3e}"


def oracle_dx(runs, name):
    """fp64 displacement of the movable rows of a block case, on the graph and gate values the GPU run used"""
    from cbgbench_amd import stages
    from oracle import unitransformer as OU, weights
    x, h, lig, mov, _ = block_inputs()[name]
    r = runs["fold"]
    nbr, deg, e_w = torch.from_numpy(r[f"{name}.nbr"]), torch.from_numpy(r[f"{name}.deg"]), torch.from_numpy(r[f"{name}.e_w"])
    ei = stages.edge_index_from_nbr(nbr, deg)
    mask = torch.arange(32)[None, :] < deg[:, None]
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in weights.synthetic_state_dict(13, 4, seed=0).items()
          if k.startswith("denoiser")}
    dx = OU.h2x_attention(sd, "denoiser.blocks.0.h2x_layers.0", x.double(), h.double(), OU.build_edge_type(ei, lig), ei,
                          e_w[mask][:, None].double())
    return dx[mov]


@pytest.fixture(scope="module")
def oracle_forward():
    from oracle import unitransformer as OU, weights
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in weights.synthetic_state_dict(13, 4, seed=0).items()}
    return {name: OU.unitransformer_forward(sd, x.double(), h.double(), batch, lig, mov)
            for name, (x, h, lig, mov, batch) in forward_inputs().items()}


# ---- tests --------------------------------------------------------------------------------------------------------------------------
def test_shapes_are_what_they_claim(runs):
    r, cases = runs["fold"], block_inputs()
    _, _, lig, mov, _ = cases["one_movable_34"]
    assert lig.shape[0] == 34 and int(mov.sum()) == 1
    assert set(r["deg19.deg"].tolist()) == {19}
    _, _, lig, mov, _ = cases["all_lig_nbrs"]
    rows = torch.nonzero(mov).flatten()
    assert bool(lig[torch.from_numpy(r["all_lig_nbrs.nbr"])[rows].long()].all()) and set(r["all_lig_nbrs.deg"][rows.numpy()].tolist()) == {32}
    _, _, lig, mov, _ = cases["all_prot_nbrs"]
    rows = torch.nonzero(mov).flatten()
    assert not bool(lig[torch.from_numpy(r["all_prot_nbrs.nbr"])[rows].long()].any()) and r["all_prot_nbrs.deg"][rows.numpy()].tolist() == [32]
    for k in LIST_LENGTHS:
        assert int(cases[f"list{k}"][3].sum()) == k
    _, _, lig, mov, _ = cases["linker"]
    assert 0 < int(mov.sum()) < int(lig.sum()) and not bool((mov & ~lig).any())


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_block_is_no_worse_than_the_general_kernel(runs, name):
    """flag set: the fold kernel (default) and the general kernel behind node_qfold_kernel (CBGX_H2X_FOLD=0) against the fp64 oracle"""
    x, _, _, mov, _ = block_inputs()[name]
    fold, plain = runs["fold"], runs["plain"]
    ref = oracle_dx(runs, name)
    assert_no_worse(torch.from_numpy(fold[f"{name}.dx.1"])[mov], torch.from_numpy(plain[f"{name}.dx.1"])[mov], ref, f"{name} dx")
    assert_no_worse(torch.from_numpy(fold[f"{name}.x_out.1"])[mov], torch.from_numpy(plain[f"{name}.x_out.1"])[mov],
                    x[mov].double() + ref, f"{name} x_out")
    xo, dx = torch.from_numpy(fold[f"{name}.x_out.1"]), torch.from_numpy(fold[f"{name}.dx.1"])
    assert torch.equal(xo[~mov], x[~mov]) and not bool(dx[~mov].any())          # fixed rows: copied, zero displacement
    if int(mov.sum()):
        assert bool((dx[mov].abs().sum(-1) > 0).all())


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_block_without_the_flag_is_unchanged(runs, name):
    """flag not set: the general kernel in both processes; and CBGX_H2X_FOLD=0 with the flag is that same path"""
    fold, plain = runs["fold"], runs["plain"]
    for what in ("x_out", "dx"):
        assert np.array_equal(fold[f"{name}.{what}.0"], plain[f"{name}.{what}.0"])
        assert np.array_equal(plain[f"{name}.{what}.1"], plain[f"{name}.{what}.0"])


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_whole_forward(runs, oracle_forward, name):
    fold, plain = runs["fold"], runs["plain"]
    for k, what in enumerate(("x_out", "h_out", "logits")):
        assert_no_worse(torch.from_numpy(fold[f"{name}.{what}.1"]), torch.from_numpy(plain[f"{name}.{what}.1"]), oracle_forward[name][k],
                        f"{name} {what}")
        assert np.array_equal(fold[f"{name}.{what}.0"], plain[f"{name}.{what}.0"])          # flag not set: unchanged
        assert np.array_equal(plain[f"{name}.{what}.1"], plain[f"{name}.{what}.0"])
    # the launches: with the flag and the fold kernel no h2x block writes its folded rows (no qfold job in the node stage); in every
    # other combination they are written as before
    assert bool(fold[f"{name}.qt_untouched.1"])
    assert not bool(fold[f"{name}.qt_untouched.0"]) and not bool(plain[f"{name}.qt_untouched.1"]) and not bool(plain[f"{name}.qt_untouched.0"])


def test_unknown_flags_are_refused():
    from cbgbench_amd import _native
    lib = _native.lib()
    one = torch.zeros(64, device=DEV)
    p = _native.ptr(one)
    assert lib.cbgx_h2x_attention_v2(p, 0, p, p, p, p, p, p, p, 1, p, None, 4, p, 64, None) == -1
    assert lib.cbgx_h2x_stack_forward_v2(p, 1, p, p, p, p, p, 1, 1, p, 1, p, 64, None) == -1
    assert lib.cbgx_unitransformer_forward_v2(p, 4, 13, p, p, p, p, p, 1, 1, p, p, p, 8, p, 64, None) == -1


if __name__ == "__main__":
    _worker(sys.argv[1])
