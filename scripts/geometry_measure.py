"""Cost of the geometry report on one MI355X (profiles/geometry_measure.log):
sample_cli --synthetic 100 --num_samples 10 --geometry (the BASELINE configs[1] job shape) with stats["geometry"] next to stats["sample"],
the numpy model's time on one of its batches, and the launch's own time on that batch.

    python scripts/geometry_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, synthetic, geometry as G
from cbgbench_amd.priors import PROTEIN_ELEMENTS
from tests import geometry_model as GM

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="geometry_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
res = {}
for tag, extra in (("geo", ["--geometry"]),):
    stats = {}
    torch.manual_seed(0)
    sample_cli.main(["--config", cfg, "--synthetic", "100", "--num_samples", "10", "--random_init", "--no_translate", "--out_root",
                     os.path.join(out, tag)] + extra, stats=stats)
    res[tag] = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
    print(tag, json.dumps(res[tag]), flush=True)
d = os.path.join(out, "geo", "targetdiff_test")
print(open(os.path.join(d, "geometry_summary.json")).read())
# one batch = 10 pockets x 10 samples: the model on it
rng0 = np.random.default_rng(2024)
pockets = [synthetic.make_pocket(rng0, int(rng0.integers(350, 651))) for _ in range(100)]
graphs = []
for i in range(10):
    rec = torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)
    z_rec = PROTEIN_ELEMENTS.numpy()[pockets[i][1][:, :6].argmax(-1)]
    for s in rec["samples"]:
        graphs.append((s["pos"].numpy(), np.asarray(s["atom"]), pockets[i][0], z_rec, s))
t0 = time.perf_counter()
model = [GM.graph_geometry(*g[:4]) for g in graphs]
t_model = time.perf_counter() - t0
ok = all(np.array_equal(m[0], g[4]["nr_bonds"].numpy()) and np.array_equal((m[1] & 1) != 0, g[4]["atom_stable"].numpy())
         and np.array_equal((m[1] & 2) != 0, g[4]["inter_clash"].numpy()) for m, g in zip(model, graphs))
print(f"numpy model on one batch (100 graphs, {sum(len(g[1]) for g in graphs)} ligand atoms, {sum(len(g[3]) for g in graphs)} protein atoms): "
      f"{t_model * 1e3:.1f} ms; equals the files' fields: {ok}")
dev = torch.device("cuda:0")
cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(g[k]) for g in graphs]).astype(dt)).to(dev)
x_lig, z_lig, x_rec, z_rec = cat(0, np.float32), cat(1, np.int64), cat(2, np.float32), cat(3, np.int64)
lb = torch.from_numpy(np.repeat(np.arange(100), [len(g[1]) for g in graphs])).to(dev)
rb = torch.from_numpy(np.repeat(np.arange(100), [len(g[3]) for g in graphs])).to(dev)
G.ligand_geometry(x_lig, z_lig, lb, x_rec, z_rec, rb, 100)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(20):
    G.ligand_geometry(x_lig, z_lig, lb, x_rec, z_rec, rb, 100)
torch.cuda.synchronize()
print(f"ligand_geometry (CSR build + launch, wall, per call): {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms")
# the launch alone: raw entry on prepared buffers, HIP events
from cbgbench_amd import _native
lp, rp = G._csr(lb, 100, "l"), G._csr(rb, 100, "r")
zl, zr = z_lig.to(torch.uint8), z_rec.to(torch.uint8)
nr = torch.empty(x_lig.shape[0], dtype=torch.int32, device=dev); fl = torch.empty(x_lig.shape[0], dtype=torch.uint8, device=dev)
gc = torch.empty(100, 6, dtype=torch.int32, device=dev)
p = _native.ptr
call = lambda: _native.lib().cbgx_ligand_geometry(p(x_lig), p(zl), p(lp), x_lig.shape[0], p(x_rec), p(zr), p(rp), x_rec.shape[0], 100,
                                                  p(nr), p(fl), p(gc), _native.current_stream(dev))
call(); torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    assert call() == 0
e1.record(); torch.cuda.synchronize()
print(f"cbgx_ligand_geometry (lig_ptr read-back + kernel, HIP events, per call): {e0.elapsed_time(e1) / 20 * 1e3:.1f} us")
print("RESULT", json.dumps(res))
