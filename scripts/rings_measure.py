"""Cost of the ring report on one MI355X (profiles/rings_measure.log):
sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs) with --bonds --rings, stats["rings"] next to
stats["bonds"] and stats["sample"]; then the launch alone, from HIP events, on the job's own 1000 bond graphs, on 1000 molecule-like graphs
of 10 - 45 atoms (a chain with 0 - 4 ring closures of size 3 - 7, mostly 5 and 6: what a trained model's table bonds look like; random
weights give collapsed samples far over the limits), and on 1000 copies of four graphs at the limits.

    python scripts/rings_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, _native, geometry as G
from tests import rings_model as RM

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="rings_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
# a small run first: code objects are loaded and the allocator is warm before the timed run
sample_cli.main(["--config", cfg, "--synthetic", "10", "--num_samples", "10", "--random_init", "--no_translate", "--bonds", "--rings",
                 "--out_root", os.path.join(out, "warmup")])
stats = {}
torch.manual_seed(0)
t0 = time.perf_counter()
sample_cli.main(["--config", cfg, "--synthetic", "100", "--num_samples", "10", "--random_init", "--no_translate", "--bonds", "--rings",
                 "--out_root", os.path.join(out, "rings")], stats=stats)
torch.cuda.synchronize()
res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
res["wall"] = round(time.perf_counter() - t0, 4)
print("job", json.dumps(res), flush=True)
d = os.path.join(out, "rings", "targetdiff_test")
print(open(os.path.join(d, "rings_summary.json")).read())


def collate(graphs):
    lig_ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])]).astype(np.int32)
    idx = np.concatenate([np.array(p, np.int32).reshape(-1, 2).T + lig_ptr[g] for g, (_, p) in enumerate(graphs)]
                         + [np.zeros((2, 0), np.int32)], axis=1).astype(np.int32)
    bond_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx[0], minlength=int(lig_ptr[-1])))]).astype(np.int32)
    return lig_ptr, int(lig_ptr[-1]), bond_ptr, idx


def launch_time(name, batch, check=0, reps=5):
    lig_ptr, n_lig, bond_ptr, idx = batch
    B = len(lig_ptr) - 1
    lp, bp, bi = (torch.from_numpy(a).to(dev) for a in (lig_ptr, bond_ptr, idx))
    rmin = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    gc = torch.empty(B, RM.COLS, dtype=torch.int32, device=dev)
    p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
    call = lambda: lib.cbgx_ligand_rings(p(lp), n_lig, B, p(bp), p(bi), idx.shape[1], p(rmin), p(gc), st)
    assert call() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert call() == 0
    e1.record(); torch.cuda.synchronize()
    g = gc.cpu().numpy()
    ok = g[:, -1] == 0
    line = (f"{name}: {B} graphs, {n_lig} atoms, {idx.shape[1]} bonds; cbgx_ligand_rings, HIP events, per launch: "
            f"{e0.elapsed_time(e1) / reps * 1e3:.1f} us; evaluated {int(ok.sum())}, over a limit {int((~ok).sum())}, "
            f"rings_3..9 + larger {g[ok][:, 3:11].sum(0).tolist()}")
    if check:
        sub = collate_slice(batch, check)
        want = RM.batch_rings(*sub)
        line += f"; first {check} graphs equal the model: {np.array_equal(g[:check], want[1]) and np.array_equal(rmin.cpu().numpy()[:sub[1]], want[0])}"
    print(line, flush=True)


def collate_slice(batch, count):
    lig_ptr, _, bond_ptr, idx = batch
    n, nb = int(lig_ptr[count]), int(bond_ptr[lig_ptr[count]])
    return lig_ptr[:count + 1], n, bond_ptr[:n + 1], idx[:, :nb]


# (1) the job's own graphs: the files' bond lists
samples = [s for i in range(100) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
launch_time("job graphs (random weights: collapsed samples)", collate([(len(s["atom"]), s["bond_index"].numpy().T) for s in samples]))

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


launch_time("molecule-like graphs of 10 - 45 atoms", collate([molecule(int(rng.integers(10, 46))) for _ in range(1000)]), check=100)

# (3) graphs at the limits, 1000 copies of each
ring = [(i, i + 1) for i in range(255)] + [(0, 255)]
dense = {(int(rng.integers(0, i)), i) for i in range(1, 256)}
while len(dense) < 383:
    a, b = sorted(int(v) for v in rng.integers(0, 256, 2))
    if a != b:
        dense.add((a, b))
worst = {
    "ring of 256 atoms with 126 chords (127 cycles)": (256, sorted(ring + [(i, i + 4) for i in range(0, 252, 2)])),
    "triangle strip of 130 atoms (128 cycles)": (130, sorted([(i, i + 1) for i in range(129)] + [(i, i + 2) for i in range(128)])),
    "random connected graph of 256 atoms and 383 bonds (128 cycles)": (256, sorted(dense)),
    "K17 (120 cycles)": (17, [(i, j) for i in range(17) for j in range(i + 1, 17)]),
}
for name, graph in worst.items():
    launch_time("worst case, " + name, collate([graph] * 1000), check=1)
print("RESULT", json.dumps(res))
