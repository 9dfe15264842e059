"""Cost of the valence report on one MI355X (profiles/valence_measure.log):
sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs) with --valence, stats["valence"] next to
stats["sample"] -- alone (the report then pays for the bond list, the ring report and the aromatic report it is computed from) and beside
--bonds --rings --aromatic (its own launch and download); then the launch alone, from HIP events after a warm-up launch, with
cbgx_ligand_aromatic's measured times for scale (profiles/aromatic_measure.log): on the job's own 1000 bond graphs (random weights:
collapsed samples), on the 1000 seeded molecule-like graphs of 10 - 45 atoms of tests/test_valence.py (fused 5- and 6-rings, whole rings
aromatic: what a trained model's samples look like), and on 1000 copies of the worst cases within the limits: the 16-hexagon system under
its most expensive labelling inside the step budget, 128 two-atom systems in one graph, and (100 copies) a complete graph on 256 atoms.

    python scripts/valence_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, _native, geometry as G
from tests import valence_model as VM
from tests.test_valence import collate, graph, seeded_sets
from tests.test_gpu_valence import model_steps, polyhex

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="valence_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
print("device", torch.cuda.get_device_name(0), flush=True)
common = ["--config", cfg, "--num_samples", "10", "--random_init", "--no_translate"]
# a small run first: code objects are loaded and the allocator is warm before the timed runs
sample_cli.main(common + ["--synthetic", "10", "--valence", "--aromatic", "--bonds", "--out_root", os.path.join(out, "warmup")])
results = {}
for tag, flags in (("alone", ["--valence"]), ("beside", ["--valence", "--bonds", "--rings", "--aromatic"])):
    stats = {}
    torch.manual_seed(0)
    t0 = time.perf_counter()
    sample_cli.main(common + ["--synthetic", "100", "--out_root", os.path.join(out, tag)] + flags, stats=stats)
    torch.cuda.synchronize()
    res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
    res["wall"] = round(time.perf_counter() - t0, 4)
    results[tag] = res
    print(f"job, --valence {tag}", json.dumps(res), flush=True)
d = os.path.join(out, "beside", "targetdiff_test")
print(open(os.path.join(d, "valence_summary.json")).read())


def timed(call, reps):
    assert call() == 0                               # warm-up launch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert call() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def launch_time(name, args, check=0, reps=10):
    z, lig_ptr, n_lig, bond_ptr, idx, order, aro = args
    B, nb = len(lig_ptr) - 1, idx.shape[1]
    zz, lp, bp, bi, bo, ba = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (z, lig_ptr, bond_ptr, idx, order, aro))
    h, f = torch.empty(n_lig, dtype=torch.uint8, device=dev), torch.empty(n_lig, dtype=torch.uint8, device=dev)
    k, gc = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(B, VM.COLS, dtype=torch.int32, device=dev)
    p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
    us = timed(lambda: lib.cbgx_ligand_valence(p(zz), p(lp), n_lig, B, p(bp), p(bi), p(bo), p(ba), nb, VM.MAX_STEPS, p(h), p(f), p(k), p(gc),
                                               st), reps)
    g = gc.cpu().numpy()
    ok = g[:, -1] == 0
    line = (f"{name}: {B} graphs, {n_lig} atoms, {nb} bonds; HIP events, mean of {reps} launches after a warm-up launch: "
            f"cbgx_ligand_valence {us:.1f} us; evaluated {int(ok.sum())}, not evaluated {int((~ok).sum())} (status bits "
            f"{sorted(set(g[~ok][:, -1].tolist()))}), systems / failed / doubles / implicit H / exceeded "
            f"{g[ok][:, [3, 4, 5, 6, 7]].sum(0).tolist()}, largest step count {int(g[ok][:, 20].max()) if ok.any() else 0}")
    if check:
        n, m = int(lig_ptr[check]), int(bond_ptr[lig_ptr[check]])
        want = VM.batch_valence(z[:n], lig_ptr[:check + 1], n, bond_ptr[:n + 1], idx[:, :m], order[:m], aro[:m])
        same = (np.array_equal(g[:check], want[3]) and np.array_equal(h.cpu().numpy()[:n], want[0])
                and np.array_equal(f.cpu().numpy()[:n], want[1]) and np.array_equal(k.cpu().numpy()[:m], want[2]))
        line += f"; first {check} graphs equal the model: {same}"
    print(line, flush=True)


# (1) the job's own graphs: the files' bond lists, elements and aromatic bonds
samples = [s for i in range(100) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
cases = [(len(s["atom"]), [tuple(e) for e in s["bond_index"].numpy().T.tolist()], s["atom"], s["bond_order"].tolist(),
          np.where(s["bond_type"].numpy() == 255, 255, s["aromatic_bond"].numpy().astype(np.uint8)).tolist()) for s in samples]
launch_time("job graphs (random weights: collapsed samples)", collate(cases))

# (2) molecule-like graphs
launch_time("molecule-like graphs of 10 - 45 atoms", collate(list(seeded_sets()[0])), check=100)

# (3) the worst cases within the limits, 1000 copies of each
labellings = [(model_steps(polyhex(4, 4, 0, s)), s) for s in [None] + list(range(12))]
steps, seed = max((st[0], -1 if s is None else s) for st, s in labellings if st)
worst = {
    f"16 fused hexagons, the labelling of 13 with the longest search inside the budget ({steps} steps)": polyhex(4, 4, 0, None if seed < 0 else seed),
    "128 two-atom systems in one graph of 256 atoms": graph([6, 7] * 128, [(2 * t, 2 * t + 1) for t in range(128)]),
    "complete graph on 256 atoms, no aromatic bond (32 640 bonds: every atom exceeded)":
        graph([6] * 256, [], plain=[(i, j) for i in range(256) for j in range(i + 1, 256)]),
}
for name, case in worst.items():
    copies = 100 if case[0] == 256 and len(case[1]) > 1000 else 1000
    launch_time("worst case, " + name, collate([case] * copies), check=1)
print("RESULT", json.dumps(results))
