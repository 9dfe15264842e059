"""Cost of the bond report on one MI355X (profiles/bonds_measure.log):
sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs) without and with --bonds, wall time of each
run and stats["bonds"] next to stats["sample"]; then, on one of its batches (100 graphs), the two launches and the prefix sum between them
from HIP events, and how the bytes the report downloads split into the bond list and the rest.

    python scripts/bonds_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, _native, geometry as G
from tests import bonds_model as BM

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="bonds_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
res = {}
# a small run first: code objects are loaded and the allocator is warm before either timed run
sample_cli.main(["--config", cfg, "--synthetic", "10", "--num_samples", "10", "--random_init", "--no_translate", "--bonds", "--out_root",
                 os.path.join(out, "warmup")])
for tag, extra in (("plain", []), ("bonds", ["--bonds"])):
    stats = {}
    torch.manual_seed(0)
    t0 = time.perf_counter()
    sample_cli.main(["--config", cfg, "--synthetic", "100", "--num_samples", "10", "--random_init", "--no_translate", "--out_root",
                     os.path.join(out, tag)] + extra, stats=stats)
    torch.cuda.synchronize()
    res[tag] = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
    res[tag]["wall"] = round(time.perf_counter() - t0, 4)
    print(tag, json.dumps(res[tag]), flush=True)
d = os.path.join(out, "bonds", "targetdiff_test")
print(open(os.path.join(d, "bonds_summary.json")).read())
# one batch = 10 pockets x 10 samples: the model on it, and the files' fields against it
samples = [s for i in range(10) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
t0 = time.perf_counter()
model = [BM.graph_bonds(s["pos"].numpy(), np.asarray(s["atom"])) for s in samples]
t_model = time.perf_counter() - t0
ok = all(np.array_equal(m["bond_index"], s["bond_index"].numpy()) and np.array_equal(m["bond_order"], s["bond_order"].numpy())
         and np.array_equal(m["bond_length"].view(np.int64), s["bond_length"].numpy().view(np.int64))
         and np.array_equal(m["fragment"], s["fragment"].numpy()) for m, s in zip(model, samples))
n_atoms = sum(len(s["atom"]) for s in samples)
print(f"numpy model on one batch (100 graphs, {n_atoms} ligand atoms, {sum(m['bond_index'].shape[1] for m in model)} bonds): "
      f"{t_model * 1e3:.1f} ms; equals the files' fields: {ok}")
dev = torch.device("cuda:0")
x = torch.cat([s["pos"] for s in samples]).to(torch.float32).to(dev)
z = torch.from_numpy(np.concatenate([np.asarray(s["atom"]) for s in samples]).astype(np.int64)).to(dev)
lb = torch.from_numpy(np.repeat(np.arange(100), [len(s["atom"]) for s in samples])).to(dev)
rep = G.ligand_bonds(x, z, lb, 100)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(20):
    G.ligand_bonds(x, z, lb, 100)
torch.cuda.synchronize()
print(f"ligand_bonds (CSR build + count + cumsum and its read-back + fill + bond_graph, wall, per call): "
      f"{(time.perf_counter() - t0) / 20 * 1e3:.3f} ms")
size = {k: v.numel() * v.element_size() for k, v in rep.items()}
lists = sum(size[k] for k in ("bond_index", "bond_order", "bond_length", "bond_graph"))
print(f"bytes downloaded per batch: {json.dumps(size)}; the bond list is {lists} of {sum(size.values())} = "
      f"{100.0 * lists / sum(size.values()):.1f} %")
# the launches alone: raw entries on prepared buffers, HIP events around 20 calls of each step
n, lp, zb = x.shape[0], G._csr(lb, 100, "l"), z.to(torch.uint8)
deg = torch.empty(n, dtype=torch.int32, device=dev); frag = torch.empty_like(deg)
gc = torch.empty(100, 6, dtype=torch.int32, device=dev)
p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
count = lambda: lib.cbgx_ligand_bonds_count(p(x), p(zb), p(lp), n, 100, p(deg), p(frag), p(gc), st)
assert count() == 0
scan = lambda: torch.cat([deg.new_zeros(1, dtype=torch.int64), deg.cumsum(0, dtype=torch.int64)]).to(torch.int32)
bp = scan()
nb = int(bp[-1])
bi = torch.empty(2, nb, dtype=torch.int32, device=dev); bo = torch.empty(nb, dtype=torch.uint8, device=dev)
bl = torch.empty(nb, dtype=torch.float64, device=dev)
fill = lambda: lib.cbgx_ligand_bonds_fill(p(x), p(zb), p(lp), n, 100, p(bp), nb, p(bi), p(bo), p(bl), st)
assert fill() == 0
torch.cuda.synchronize()
for name, step in (("cbgx_ligand_bonds_count (lig_ptr read-back + kernel)", count), ("torch.cumsum + cat + cast (no read-back)", scan),
                   ("cbgx_ligand_bonds_fill (lig_ptr read-back + kernel)", fill)):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        r = step()
        assert torch.is_tensor(r) or r == 0
    e1.record(); torch.cuda.synchronize()
    print(f"{name}, HIP events, per call: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us")
print("RESULT", json.dumps(res))
