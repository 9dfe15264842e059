"""Cost of the aromatic report on one MI355X (profiles/aromatic_measure.log):
sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs) with --aromatic, stats["aromatic"] next to
stats["sample"]; then the launch alone, from HIP events after a warm-up launch, with cbgx_ligand_rings on the same bond list for scale: on
the job's own 1000 bond graphs, on 1000 molecule-like graphs of 10 - 45 atoms (a chain with 0 - 4 ring closures of size 3 - 7, mostly 5
and 6, a third of the atoms flagged: what a trained model's samples look like; random weights give collapsed samples), and on 1000 copies of
graphs at the limits and of the layered worst case of csrc/aromatic.hip.

    python scripts/aromatic_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, _native, geometry as G
from tests import aromatic_model as AM, rings_model as RM

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="aromatic_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
print("device", torch.cuda.get_device_name(0), flush=True)
# a small run first: code objects are loaded and the allocator is warm before the timed run
sample_cli.main(["--config", cfg, "--synthetic", "10", "--num_samples", "10", "--random_init", "--no_translate", "--aromatic", "--bonds",
                 "--out_root", os.path.join(out, "warmup")])
stats = {}
torch.manual_seed(0)
t0 = time.perf_counter()
sample_cli.main(["--config", cfg, "--synthetic", "100", "--num_samples", "10", "--random_init", "--no_translate", "--aromatic", "--bonds",
                 "--out_root", os.path.join(out, "aromatic")], stats=stats)
torch.cuda.synchronize()
res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
res["wall"] = round(time.perf_counter() - t0, 4)
print("job", json.dumps(res), flush=True)
d = os.path.join(out, "aromatic", "targetdiff_test")
print(open(os.path.join(d, "aromatic_summary.json")).read())


def collate(graphs):
    lig_ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int32)
    idx = np.concatenate([np.array(p, np.int32).reshape(-1, 2).T + lig_ptr[g] for g, (_, p) in enumerate(graphs)]
                         + [np.zeros((2, 0), np.int32)], axis=1).astype(np.int32)
    bond_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx[0], minlength=int(lig_ptr[-1])))]).astype(np.int32)
    return lig_ptr, int(lig_ptr[-1]), bond_ptr, idx


def timed(call, reps):
    assert call() == 0                               # warm-up launch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert call() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def launch_time(name, batch, z, flags, check=0, reps=10):
    lig_ptr, n_lig, bond_ptr, idx = batch
    B = len(lig_ptr) - 1
    lp, bp, bi, zz, ff = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (lig_ptr, bond_ptr, idx, z, flags))
    rmin = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    rgc = torch.empty(B, RM.COLS, dtype=torch.int32, device=dev)
    atom, bond = torch.empty(n_lig, dtype=torch.uint8, device=dev), torch.empty(idx.shape[1], dtype=torch.uint8, device=dev)
    gc = torch.empty(B, AM.COLS, dtype=torch.int32, device=dev)
    p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
    us_rings = timed(lambda: lib.cbgx_ligand_rings(p(lp), n_lig, B, p(bp), p(bi), idx.shape[1], p(rmin), p(rgc), st), reps)
    us = timed(lambda: lib.cbgx_ligand_aromatic(p(zz), p(ff), p(rmin), p(lp), n_lig, B, p(bp), p(bi), idx.shape[1], p(atom), p(bond),
                                                p(gc), st), reps)
    g = gc.cpu().numpy()
    ok = g[:, -1] == 0
    line = (f"{name}: {B} graphs, {n_lig} atoms, {idx.shape[1]} bonds; HIP events, mean of {reps} launches after a warm-up launch: "
            f"cbgx_ligand_aromatic {us:.1f} us, cbgx_ligand_rings on the same list {us_rings:.1f} us; evaluated {int(ok.sum())}, "
            f"not evaluated {int((~ok).sum())}, cycles56 / aromatic / flagged / closure / unsupported "
            f"{g[ok][:, [2, 3, 4, 5, 8]].sum(0).tolist()}")
    if check:
        count = check
        n, nb = int(lig_ptr[count]), int(bond_ptr[lig_ptr[count]])
        want = AM.batch_aromatic(z[:n], flags[:n], rmin.cpu().numpy()[:n], lig_ptr[:count + 1], n, bond_ptr[:n + 1], idx[:, :nb])
        same = (np.array_equal(g[:count], want[2]) and np.array_equal(atom.cpu().numpy()[:n], want[0])
                and np.array_equal(bond.cpu().numpy()[:nb], want[1]))
        line += f"; first {check} graphs equal the model: {same}"
    print(line, flush=True)


# (1) the job's own graphs: the files' bond lists, elements and flags
samples = [s for i in range(100) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
launch_time("job graphs (random weights: collapsed samples)", collate([(len(s["atom"]), s["bond_index"].numpy().T) for s in samples]),
            np.array([a for s in samples for a in s["atom"]], np.uint8), np.array([a for s in samples for a in s["aromatic"]], np.uint8))

# (2) molecule-like graphs
rng = np.random.default_rng(0)


def molecule(n):
    pairs = {(i, i + 1) for i in range(n - 1)}
    for _ in range(int(rng.integers(0, 5))):
        k = int(rng.choice([3, 4, 5, 5, 5, 6, 6, 6, 6, 7]))
        if n > k:
            i = int(rng.integers(0, n - k + 1))
            pairs.add((i, i + k - 1))
    return n, sorted(pairs)


def atoms(n_lig, share=1 / 3):
    return rng.choice(np.array([6, 6, 6, 6, 7, 8, 16], np.uint8), n_lig), (rng.random(n_lig) < share).astype(np.uint8)


batch = collate([molecule(int(rng.integers(10, 46))) for _ in range(1000)])
launch_time("molecule-like graphs of 10 - 45 atoms", batch, *atoms(batch[1]), check=100)

# (3) graphs at the limits and the layered worst case, 1000 copies of each
ring = [(i, i + 1) for i in range(255)] + [(0, 255)]
layers = [[0]] + [list(range(1 + 7 * k, 8 + 7 * k)) for k in range(4)]
acene = 33
width = 2 * acene + 1
worst = {
    "ring of 256 atoms with 126 chords (251 cycles)": (256, sorted(ring + [(i, i + 4) for i in range(0, 252, 2)])),
    "triangle strip of 130 atoms": (130, sorted([(i, i + 1) for i in range(129)] + [(i, i + 2) for i in range(128)])),
    "K17": (17, [(i, j) for i in range(17) for j in range(i + 1, 17)]),
    "K(2,120)": (122, [(h, 2 + k) for h in (0, 1) for k in range(120)]),
    "layers 1-7-7-7-7, complete between neighbours (154 bonds)": (29, sorted((a, b) for k in range(4) for a in layers[k] for b in layers[k + 1])),
    "33 fused hexagons": (2 * width, sorted([(i, i + 1) for i in range(width - 1)] + [(width + i, width + i + 1) for i in range(width - 1)]
                                            + [(2 * k, width + 2 * k) for k in range(acene + 1)])),
}
for name, graph in worst.items():
    batch = collate([graph] * 1000)
    z, flags = atoms(graph[0])
    if name.startswith("33 fused"):      # ring 0 flagged and one outer atom per ring: the closure takes one sweep per ring
        z[:] = 6
        flags[:] = 0
        flags[[0, 1, 2, width, width + 1, width + 2] + [2 * k + 1 for k in range(1, acene)]] = 1
    launch_time("worst case, " + name, batch, np.tile(z, 1000), np.tile(flags, 1000), check=1)
print("RESULT", json.dumps(res))
