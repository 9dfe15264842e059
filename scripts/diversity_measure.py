"""Cost of the diversity report on one MI355X (profiles/diversity_measure.log), on the recipe of
scripts/groups_measure.py: sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs, 100 pockets of 10)
with --diversity, stats["diversity"] next to stats["sample"] and stats["write"] -- alone (the report then pays for the bond list, the ring
report and the aromatic report it is computed from) and beside --bonds --rings --aromatic (its own two launches and downloads); then each
launch alone, from HIP events after a warm-up launch, with cbgx_ligand_groups timed on the same inputs beside them: on the 1000 seeded
molecule-like graphs of 10 - 45 atoms of tests/test_valence.py in groups of 10 (what a trained model's samples look like), on the job's own
1000 bond graphs (random weights: collapsed samples), on one group of 1024 graphs, and on the largest graphs within the limits.

    python scripts/diversity_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, _native, geometry as G
from tests import diversity_model as DM, groups_model as GM
from tests.test_valence import seeded_sets
from tests.test_diversity import case, collate, typed

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="diversity_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
print("device", torch.cuda.get_device_name(0), flush=True)
common = ["--config", cfg, "--num_samples", "10", "--random_init", "--no_translate"]
# a small run first: code objects are loaded and the allocator is warm before the timed runs
sample_cli.main(common + ["--synthetic", "10", "--diversity", "--aromatic", "--rings", "--bonds", "--out_root", os.path.join(out, "warmup")])
results = {}
for tag, flags in (("alone", ["--diversity"]), ("beside", ["--diversity", "--bonds", "--rings", "--aromatic"])):
    stats = {}
    torch.manual_seed(0)
    t0 = time.perf_counter()
    sample_cli.main(common + ["--synthetic", "100", "--out_root", os.path.join(out, tag)] + flags, stats=stats)
    torch.cuda.synchronize()
    res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
    res["wall"] = round(time.perf_counter() - t0, 4)
    results[tag] = res
    print(f"job, --diversity {tag}", json.dumps(res), flush=True)
d = os.path.join(out, "beside", "targetdiff_test")
print(open(os.path.join(d, "diversity_summary.json")).read())


def timed(call, reps):
    assert call() == 0                               # warm-up launch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert call() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def launch_time(name, args, group_ptr, check=0, reps=10):
    z, lig_ptr, n_lig, bond_ptr, idx, types, rmin = args
    B, nb, P = len(lig_ptr) - 1, idx.shape[1], len(group_ptr) - 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zz, lp, bp, bi, bt, rm = (up(a) for a in (z, lig_ptr, bond_ptr, idx, types, rmin))
    order, aro = up(np.where(types == 4, 1, types).astype(np.uint8)), up(np.where(types == 255, 255, types == 4).astype(np.uint8))
    fp, h = torch.empty(B, 32, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    gc = torch.empty(B, DM.COLS, dtype=torch.int32, device=dev)
    pair_ptr = G.group_pair_ptr(group_ptr, B)
    gp, pp = up(np.asarray(group_ptr, np.int32)), up(np.asarray(pair_ptr, np.int64))
    pairs = torch.empty(max(pair_ptr[-1], 1), dtype=torch.int32, device=dev)
    per = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3)]
    go = torch.empty(P, DM.GROUP_COLS, dtype=torch.int64, device=dev)
    grp, cls = torch.empty(n_lig, dtype=torch.int32, device=dev), torch.empty(n_lig, dtype=torch.uint8, device=dev)
    ggc = torch.empty(B, GM.COLS, dtype=torch.int32, device=dev)
    p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
    nul = lambda t: p(t) if nb else None
    us_fp = timed(lambda: lib.cbgx_ligand_fingerprints(p(zz), p(lp), n_lig, B, p(bp), nul(bi), nul(bt), p(rm), nb, p(fp), p(h), p(gc), st), reps)
    status = gc[:, 4].contiguous()
    us_dv = timed(lambda: lib.cbgx_group_diversity(p(fp), p(h), p(status), p(gp), p(pp), B, P, pair_ptr[-1], p(pairs), *[p(t) for t in per],
                                                   p(go), st), reps)
    us_grp = timed(lambda: lib.cbgx_ligand_groups(p(zz), p(lp), n_lig, B, p(bp), nul(bi), nul(order), nul(aro), nb, p(grp), p(cls), p(ggc), st), reps)
    g, s = gc.cpu().numpy(), G.summarise_diversity(go)
    ok = g[:, 4] == 0
    line = (f"{name}: {B} graphs in {P} groups, {n_lig} atoms, {nb} bonds, {pair_ptr[-1]} pairs; HIP events, mean of {reps} launches after a "
            f"warm-up launch: cbgx_ligand_fingerprints {us_fp:.1f} us, cbgx_group_diversity {us_dv:.1f} us, cbgx_ligand_groups on the same "
            f"inputs {us_grp:.1f} us; evaluated {int(ok.sum())}, not evaluated {int((~ok).sum())} (status bits "
            f"{sorted(set(g[~ok][:, 4].tolist()))}), rounds up to {int(g[:, 3].max())}, bits set {int(g[ok][:, 2].sum()) if ok.any() else 0}; "
            f"unique_mol_ratio {s['unique_mol_ratio']:.4f}, mean_pocket_diversity {s['mean_pocket_diversity']:.4f}")
    if check:
        n, m = int(lig_ptr[check]), int(bond_ptr[lig_ptr[check]])
        want = DM.batch_fingerprints(z[:n], lig_ptr[:check + 1], n, bond_ptr[:n + 1], idx[:, :m], types[:m], rmin[:n])
        same = (np.array_equal(fp.cpu().numpy()[:check].view(np.uint32), want[0]) and np.array_equal(h.cpu().numpy()[:check].view(np.uint64), want[1])
                and np.array_equal(g[:check], want[2]))
        line += f"; first {check} graphs equal the model: {same}"
    print(line, flush=True)


def with_rings(args):
    """atom_ring_min of the graphs, from the ring kernel"""
    z, lig_ptr, n_lig, bond_ptr, idx, types, _ = args
    lig_b = torch.from_numpy(np.repeat(np.arange(len(lig_ptr) - 1), np.diff(lig_ptr))).to(dev)
    rings = G.ligand_rings(torch.from_numpy(idx).to(dev), lig_b, len(lig_ptr) - 1)
    return z, lig_ptr, n_lig, bond_ptr, idx, types, rings["atom_ring_min"].cpu().numpy()


tens = lambda B: list(range(0, B + 1, 10))
# (1) molecule-like graphs in groups of 10
like = [case(z, [(i, j, 4 if a else o) for (i, j), o, a in zip(pairs, order, aro)], [0] * n) for n, pairs, z, order, aro in seeded_sets()[0]]
launch_time("molecule-like graphs of 10 - 45 atoms", with_rings(collate(like)), tens(len(like)), check=50)

# (2) the job's own graphs: the files' bond lists, elements, bond types and ring bytes
samples = [s for i in range(100) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
job = [(len(s["atom"]), [(i, j, int(t)) for (i, j), t in zip(s["bond_index"].numpy().T.tolist(), s["bond_type"].tolist())], list(s["atom"]),
        s["atom_ring_min"].tolist()) for s in samples]
args = collate(job)
launch_time("job graphs (random weights: collapsed samples)", args, tens(len(job)), check=20)
want = DM.batch_fingerprints(*args)
print("the records' fingerprints and hashes equal the model on the records' graphs:",
      all(np.array_equal(s["fingerprint"].numpy().view(np.uint32), want[0][g]) and s["mol_hash"] == int(want[1][g]) for g, s in enumerate(samples)))

# (3) one group of 1024 graphs, and the largest graphs within the limits
launch_time("one group of 1024 molecule-like graphs", with_rings(collate((like * 2)[:1024])), [0, 1024])
chain = case([7] + [6] * 255, typed([(a, (a + 1) % 6) for a in range(6)], 4) + [(max(a - 1, 5), a, 1) for a in range(6, 256)], [6] * 6 + [0] * 250)
launch_time("worst case, a ring with a tail of 256 atoms (256 rounds)", collate([chain] * 1000), tens(1000), check=1)
print("RESULT", json.dumps(results))
