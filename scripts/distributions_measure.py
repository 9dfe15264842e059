"""Cost of the distributions report on one MI355X (profiles/distributions_measure.log):
sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs) with --bonds --distributions,
stats["distributions"] next to stats["bonds"] and stats["sample"]; then the two entries alone, from HIP events, on the job's own 1000
graphs (random weights: collapsed samples with ten bonds per atom), on 1000 molecule-like zigzag chains of 10 - 45 carbons, and on 1000
copies of graphs at the limits (1024 atoms for the pair histogram, 14 880 angles in a collapsed 32-atom graph for the angles), each
checked against the numpy model on its first graphs.

    python scripts/distributions_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, geometry as G
from tests import distributions_model as DM

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="distributions_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
flags = ["--random_init", "--no_translate", "--bonds", "--distributions"]
# a small run first: code objects are loaded and the allocator is warm before the timed run
sample_cli.main(["--config", cfg, "--synthetic", "10", "--num_samples", "10", "--out_root", os.path.join(out, "warmup")] + flags)
stats = {}
torch.manual_seed(0)
t0 = time.perf_counter()
sample_cli.main(["--config", cfg, "--synthetic", "100", "--num_samples", "10", "--out_root", os.path.join(out, "job")] + flags, stats=stats)
torch.cuda.synchronize()
res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
res["wall"] = round(time.perf_counter() - t0, 4)
print("job", json.dumps(res), flush=True)
d = os.path.join(out, "job", "targetdiff_test")
summary = json.load(open(os.path.join(d, "distributions_summary.json")))
print("summary counts", json.dumps(summary["counts"]), "bond types", len(summary["bond_length"]), "angle types", len(summary["bond_angle"]))
print("files", sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".pt")), "bytes")


def timed(call, reps=5):
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for _ in range(reps):
        r = call()
    e1.record(); torch.cuda.synchronize()
    return r, e0.elapsed_time(e1) / reps, (time.perf_counter() - t) / reps * 1e3


def measure(name, graphs, check=2):
    """graphs: [(x [n, 3] float32, z [n])]; the three calls of batch_distributions' device side, HIP events and wall per call"""
    x = torch.from_numpy(np.concatenate([g[0] for g in graphs]).astype(np.float32)).to(dev)
    z = torch.from_numpy(np.concatenate([g[1] for g in graphs]).astype(np.int64)).to(dev)
    sizes = np.array([len(g[1]) for g in graphs])
    b = torch.from_numpy(np.repeat(np.arange(len(graphs)), sizes)).to(dev)
    B = len(graphs)
    bonds, ev_b, wall_b = timed(lambda: G.ligand_bonds(x, z, b, B))
    hist, ev_p, wall_p = timed(lambda: G.ligand_pair_hist(x, z, b, B))
    ang, ev_a, wall_a = timed(lambda: G.ligand_angles(x, z, b, B, bonds))
    gc = ang["graph_counts"].cpu().numpy()
    n = int(sizes[:check].sum())
    want = DM.batch_distributions(x[:n].cpu().numpy(), z[:n].cpu().numpy(), np.concatenate([[0], np.cumsum(sizes[:check])]))
    m = int(want["angle_index"].shape[1])
    ok = (np.array_equal(hist[:check].cpu().numpy(), want["pair_hist"]) and np.array_equal(gc[:check], want["graph_counts"])
          and np.array_equal(ang["angle_index"][:, :m].cpu().numpy(), want["angle_index"])
          and np.array_equal(ang["angle_cos"][:m].cpu().numpy(), want["angle_cos"], equal_nan=True)
          and np.array_equal(ang["angle_bin"][:m].cpu().numpy(), want["angle_bin"])
          and np.array_equal(ang["angle_type"][:m].cpu().numpy(), want["angle_type"]))
    pairs = int((sizes.astype(np.int64) * (sizes - 1) // 2).sum())
    print(f"{name}: {B} graphs, {int(sizes.sum())} atoms, {pairs} pairs, {int(gc[:, 1].sum())} bonds, {int(gc[:, 2].sum())} angles, "
          f"{int((gc[:, 4] != 0).sum())} over the limit; per call, HIP events / wall: ligand_bonds {ev_b:.3f} / {wall_b:.3f} ms, "
          f"ligand_pair_hist {ev_p:.3f} / {wall_p:.3f} ms, ligand_angles (adjacency, prefix sums, launch, counts) {ev_a:.3f} / {wall_a:.3f} ms; "
          f"first {check} graphs equal the model: {ok}", flush=True)


# (1) the job's own graphs
samples = [s for i in range(100) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
measure("job graphs (random weights: collapsed samples)", [(s["pos"].numpy(), np.asarray(s["atom"])) for s in samples])

# (2) molecule-like graphs: zigzag chains, 1.5 A bonds, n - 2 angles
rng = np.random.default_rng(0)


def zigzag(n):
    i = np.arange(n)
    return np.stack([1.3 * i, 0.75 * (i % 2), 0 * i], 1).astype(np.float32), np.full(n, 6)


measure("zigzag chains of 10 - 45 carbons", [zigzag(int(rng.integers(10, 46))) for _ in range(1000)])

# (3) at the limits
measure("1024-atom zigzag chains (523 776 pairs each)", [zigzag(1024)] * 1000, check=1)
x = rng.uniform(0, 0.5, size=(32, 3)).astype(np.float32)
measure("32 carbons within 0.9 A: every pair bonded, 32 C(31, 2) = 14 880 angles", [(x, np.full(32, 6))] * 1000, check=1)
print("RESULT", json.dumps(res))
