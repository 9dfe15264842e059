"""Cost of the functional-group report on one MI355X (profiles/groups_measure.log):
sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs) with --groups, stats["groups"] next to
stats["sample"] and stats["write"] -- alone (the report then pays for the bond list, the ring report and the aromatic report it is
computed from) and beside --bonds --rings --aromatic --valence (its own launch and download); then the launch alone, from HIP events after
a warm-up launch, beside cbgx_ligand_valence on the same inputs: on the job's own 1000 bond graphs (random weights: collapsed samples), on
the 1000 seeded molecule-like graphs of 10 - 45 atoms of tests/test_valence.py (what a trained model's samples look like), on the 480
decorated graphs of tests/test_groups.py (two to five template groups or near misses each), and on copies of the worst cases within the
limits: 85 nitro groups in one graph (every group through the isomorphism test, more groups than lanes), 256 unbonded oxygens, 25
azulenes in one graph (the longest failing search: ten equal labels) and (100 copies) a complete graph on 256 atoms.

    python scripts/groups_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, _native, geometry as G
from tests import groups_model as GM, valence_model as VM
from tests.test_valence import collate, graph, seeded_sets
from tests.test_groups import mol, seeded_set

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="groups_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
print("device", torch.cuda.get_device_name(0), flush=True)
common = ["--config", cfg, "--num_samples", "10", "--random_init", "--no_translate"]
# a small run first: code objects are loaded and the allocator is warm before the timed runs
sample_cli.main(common + ["--synthetic", "10", "--groups", "--valence", "--aromatic", "--bonds", "--out_root", os.path.join(out, "warmup")])
results = {}
for tag, flags in (("alone", ["--groups"]), ("beside", ["--groups", "--bonds", "--rings", "--aromatic", "--valence"])):
    stats = {}
    torch.manual_seed(0)
    t0 = time.perf_counter()
    sample_cli.main(common + ["--synthetic", "100", "--out_root", os.path.join(out, tag)] + flags, stats=stats)
    torch.cuda.synchronize()
    res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
    res["wall"] = round(time.perf_counter() - t0, 4)
    results[tag] = res
    print(f"job, --groups {tag}", json.dumps(res), flush=True)
d = os.path.join(out, "beside", "targetdiff_test")
print(open(os.path.join(d, "groups_summary.json")).read())


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
    grp, cls = torch.empty(n_lig, dtype=torch.int32, device=dev), torch.empty(n_lig, dtype=torch.uint8, device=dev)
    gc = torch.empty(B, GM.COLS, dtype=torch.int32, device=dev)
    h, f = torch.empty(n_lig, dtype=torch.uint8, device=dev), torch.empty(n_lig, dtype=torch.uint8, device=dev)
    k, vc = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(B, VM.COLS, dtype=torch.int32, device=dev)
    p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
    nul = lambda t: p(t) if nb else None
    us = timed(lambda: lib.cbgx_ligand_groups(p(zz), p(lp), n_lig, B, p(bp), nul(bi), nul(bo), nul(ba), nb, p(grp), p(cls), p(gc), st), reps)
    us_val = timed(lambda: lib.cbgx_ligand_valence(p(zz), p(lp), n_lig, B, p(bp), nul(bi), nul(bo), nul(ba), nb, VM.MAX_STEPS, p(h), p(f),
                                                   nul(k), p(vc), st), reps)
    g = gc.cpu().numpy()
    ok = g[:, -1] == 0
    line = (f"{name}: {B} graphs, {n_lig} atoms, {nb} bonds; HIP events, mean of {reps} launches after a warm-up launch: "
            f"cbgx_ligand_groups {us:.1f} us, cbgx_ligand_valence on the same inputs {us_val:.1f} us; evaluated {int(ok.sum())}, not "
            f"evaluated {int((~ok).sum())} (status bits {sorted(set(g[~ok][:, -1].tolist()))}), groups / group atoms / named / other "
            f"{g[ok][:, [2, 3, 4, 31]].sum(0).tolist()}, largest group {int(g[ok][:, 5].max()) if ok.any() else 0}")
    if check:
        n, m = int(lig_ptr[check]), int(bond_ptr[lig_ptr[check]])
        want = GM.batch_groups(z[:n], lig_ptr[:check + 1], n, bond_ptr[:n + 1], idx[:, :m], order[:m], aro[:m])
        same = (np.array_equal(g[:check], want[2]) and np.array_equal(grp.cpu().numpy()[:n], want[0])
                and np.array_equal(cls.cpu().numpy()[:n], want[1]))
        line += f"; first {check} graphs equal the model: {same}"
    print(line, flush=True)


# (1) the job's own graphs: the files' bond lists, elements and aromatic bonds
samples = [s for i in range(100) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
cases = [(len(s["atom"]), [tuple(e) for e in s["bond_index"].numpy().T.tolist()], s["atom"], s["bond_order"].tolist(),
          np.where(s["bond_type"].numpy() == 255, 255, s["aromatic_bond"].numpy().astype(np.uint8)).tolist()) for s in samples]
launch_time("job graphs (random weights: collapsed samples)", collate(cases), check=20)

# (2) molecule-like graphs, and the decorated ones of the tests
launch_time("molecule-like graphs of 10 - 45 atoms", collate(list(seeded_sets()[0])), check=100)
launch_time("decorated graphs of tests/test_groups.py", collate(list(seeded_set())), check=100)

# (3) the worst cases within the limits
nitro_z, nitro_double = [8], []
for t in range(85):
    nitro_z += [7, 8, 8]
    nitro_double += [(1 + 3 * t, 2 + 3 * t), (1 + 3 * t, 3 + 3 * t)]
worst = {
    "85 nitro groups and an oxygen in one graph of 256 atoms": graph(nitro_z, [], double=nitro_double),
    "256 unbonded oxygens (256 groups)": graph([8] * 256, []),
    "25 azulenes in one graph of 250 atoms (ten equal labels, no template fits)": mol(".".join(["c1ccc2cccc2cc1"] * 25)),
    "complete graph on 128 C and 128 O, no aromatic bond (32 640 bonds: one group of 256)":
        graph([6, 8] * 128, [], plain=[(i, j) for i in range(256) for j in range(i + 1, 256)]),
}
for name, case in worst.items():
    copies = 100 if case[0] == 256 and len(case[1]) > 1000 else 1000
    launch_time("worst case, " + name, collate([case] * copies), check=1)
print("RESULT", json.dumps(results))
