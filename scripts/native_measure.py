"""Cost of the comparison with the native ligands on one MI355X (profiles/native_measure.log), on the recipe of
scripts/diversity_measure.py: sample_cli on a pockets file of 100 synthetic pockets of 350 - 650 atoms, each with a native ligand of 8
atoms beside its innermost atom (the pockets are filled balls: the ligand clashes, its score is positive and every pocket is skipped
by the reference's condition -- the cost is what is measured here, not the numbers), --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs, 100 pockets of 10) with --native,
stats["native"] next to stats["sample"] and stats["write"] -- alone (the report then pays for everything it is computed from, for the
samples and for the 100 native ligands) and beside --bonds --rings --aromatic --valence --interactions --diversity (the samples'
dependencies are then the other reports' time; the native ligands' stay its own); then the two launches alone, from HIP events after a
warm-up launch, with cbgx_ligand_geometry (the same pocket stream) timed on the same inputs beside them: on 1000 seeded ligands of 10 - 45
atoms in pockets of 350 - 650 atoms in groups of 10, on one pocket of 1024 samples, and on the largest ligands (1024 atoms) in pockets of
8192 atoms.

    python scripts/native_measure.py [out_dir]"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, synthetic, _native, geometry as G
from tests import native_model as NM

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="native_measure_")
os.makedirs(out, exist_ok=True)
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
print("device", torch.cuda.get_device_name(0), flush=True)


def toluene_like(centre):
    ang = np.arange(6) * np.pi / 3
    ring = np.stack([1.40 * np.cos(ang), 1.40 * np.sin(ang), np.zeros(6)], 1)
    return (np.concatenate([ring, [[2.91, 0, 0]], [[-2.76, 0, 0]]]) + np.asarray(centre)).astype(np.float32), np.array([2] * 6 + [1, 5], np.int64)


rng = np.random.default_rng(0)
raw = []
for _ in range(100):
    pos, feat, aa = synthetic.make_pocket(rng, int(rng.integers(350, 651)))
    lig = toluene_like(pos[np.argmin(np.linalg.norm(pos, axis=1))] + 1.9)
    raw.append({"protein_pos": pos, "protein_atom_feature": feat, "protein_aa_type": aa, "ligand_pos": lig[0], "ligand_atom_type": lig[1]})
torch.save(raw, os.path.join(out, "pockets_100.pt"))
torch.save(raw[:10], os.path.join(out, "pockets_10.pt"))
common = ["--config", cfg, "--num_samples", "10", "--random_init", "--no_translate"]
others = ["--bonds", "--rings", "--aromatic", "--valence", "--interactions", "--diversity"]
# a small run first: code objects are loaded and the allocator is warm before the timed runs
sample_cli.main(common + ["--pockets", os.path.join(out, "pockets_10.pt"), "--native", "--out_root", os.path.join(out, "warmup")] + others)
results = {}
for tag, flags in (("alone", ["--native"]), ("beside", ["--native"] + others)):
    stats = {}
    torch.manual_seed(0)
    t0 = time.perf_counter()
    sample_cli.main(common + ["--pockets", os.path.join(out, "pockets_100.pt"), "--out_root", os.path.join(out, tag)] + flags, stats=stats)
    torch.cuda.synchronize()
    res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
    res["wall"] = round(time.perf_counter() - t0, 4)
    results[tag] = res
    print(f"job, --native {tag}", json.dumps(res), flush=True)
d = os.path.join(out, "beside", "targetdiff_test")
print(open(os.path.join(d, "native_summary.json")).read())
recs = [torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False) for i in range(100)]
print("native_summary.json equals summarise_native of the records:",
      open(os.path.join(d, "native_summary.json")).read() == json.dumps(G.summarise_native([r["native_comparison"] for r in recs]), indent=1, sort_keys=True))


def timed(call, reps):
    assert call() == 0                               # warm-up launch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert call() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def launch_time(name, lig_sizes, rec_sizes, group_sizes, check=0, reps=10):
    """B ligands of ``lig_sizes`` atoms in pockets of ``rec_sizes`` atoms, the first graph of every group standing in for its native"""
    B, P = len(lig_sizes), len(group_sizes)
    lig_ptr, rec_ptr = (np.concatenate([[0], np.cumsum(s)]).astype(np.int32) for s in (lig_sizes, rec_sizes))
    group_ptr = np.concatenate([[0], np.cumsum(group_sizes)]).astype(np.int32)
    n_lig, n_rec = int(lig_ptr[-1]), int(rec_ptr[-1])
    x_lig, x_rec = (rng.normal(size=(n_lig, 3)) * 2.5).astype(np.float32), rng.uniform(-12, 12, size=(n_rec, 3)).astype(np.float32)
    z_lig, z_rec = rng.choice([6, 6, 7, 8, 1], n_lig).astype(np.uint8), rng.choice([6, 6, 7, 8, 16, 1], n_rec).astype(np.uint8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xl, zl, lp, xr, zr, rp, gp = (up(a) for a in (x_lig, z_lig, lig_ptr, x_rec, z_rec, rec_ptr, group_ptr))
    rc, lc = torch.empty(n_rec, dtype=torch.uint8, device=dev), torch.empty(n_lig, dtype=torch.uint8, device=dev)
    cen, gc = torch.empty(B, 3, dtype=torch.float64, device=dev), torch.empty(B, NM.CONTACT_COLS, dtype=torch.int32, device=dev)
    nrb, fl, ggc = torch.empty(n_lig, dtype=torch.int32, device=dev), torch.empty(n_lig, dtype=torch.uint8, device=dev), torch.empty(B, 6, dtype=torch.int32, device=dev)
    p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
    us_pc = timed(lambda: lib.cbgx_pocket_contacts(p(xl), p(zl), p(lp), n_lig, p(xr), p(zr), p(rp), n_rec, B, 16.0, p(rc), p(lc), p(cen), p(gc), st), reps)
    us_geo = timed(lambda: lib.cbgx_ligand_geometry(p(xl), p(zl), p(lp), n_lig, p(xr), p(zr), p(rp), n_rec, B, p(nrb), p(fl), p(ggc), st), reps)
    # fingerprints: random rows; the natives: the first graph of every group, with a pocket range of its own of the same length
    first = group_ptr[:-1]
    fp = up(rng.integers(0, 2 ** 32, (B, 32), dtype=np.uint64).astype(np.uint32).view(np.int32) & rng.integers(0, 2 ** 32, (B, 32), dtype=np.uint64).astype(np.uint32).view(np.int32))
    h, fs = up(rng.integers(0, 4, B).astype(np.int64)), torch.zeros(B, dtype=torch.int32, device=dev)
    status = gc[:, 5].contiguous()
    nat_len = (rec_ptr[1:] - rec_ptr[:-1])[first]
    rp_nat = up(np.concatenate([[0], np.cumsum(nat_len)]).astype(np.int32))
    rc_host = rc.cpu().numpy()
    rc_nat = up(np.concatenate([rc_host[rec_ptr[g]:rec_ptr[g + 1]] for g in first] + [np.zeros(0, np.uint8)]))
    idx = torch.from_numpy(first.astype(np.int64)).to(dev)
    fp_nat, h_nat, fs_nat, cen_nat, st_nat = fp[idx].contiguous(), h[idx].contiguous(), fs[idx].contiguous(), cen[idx].contiguous(), status[idx].contiguous()
    so, d2 = torch.empty(B, NM.SAMPLE_COLS, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
    go = torch.empty(P, NM.GROUP_COLS, dtype=torch.int64, device=dev)
    us_nc = timed(lambda: lib.cbgx_native_compare(p(fp), p(h), p(fs), p(rc), p(rp), p(cen), p(status), B, n_rec, p(fp_nat), p(h_nat), p(fs_nat),
                                                  p(rc_nat), p(rp_nat), p(cen_nat), p(st_nat), P, int(rc_nat.shape[0]), p(gp), p(so), p(d2), p(go), st), reps)
    g = gc.cpu().numpy()
    line = (f"{name}: {B} graphs in {P} groups, {n_lig} ligand atoms, {n_rec} pocket atoms; HIP events, mean of {reps} launches after a "
            f"warm-up launch: cbgx_pocket_contacts {us_pc:.1f} us, cbgx_native_compare {us_nc:.1f} us, cbgx_ligand_geometry on the same inputs "
            f"{us_geo:.1f} us; pocket atoms in contact {int(g[:, 3].sum())}, ligand atoms in contact {int(g[:, 4].sum())}, "
            f"mean contact Jaccard index {float(go[:, 6].sum()) / max(float(go[:, 5].sum()), 1) / 1e6:.4f}")
    if check:
        nl, nr = int(lig_ptr[check]), int(rec_ptr[check])
        want = NM.pocket_contacts(x_lig[:nl], z_lig[:nl], lig_ptr[:check + 1], x_rec[:nr], z_rec[:nr], rec_ptr[:check + 1], check)
        same = (np.array_equal(rc_host[:nr], want[0]) and np.array_equal(lc.cpu().numpy()[:nl], want[1])
                and NM.same_floats(cen.cpu().numpy()[:check], want[2]) and np.array_equal(g[:check], want[3]))
        line += f"; first {check} graphs equal the model: {same}"
    print(line, flush=True)


launch_time("ligands of 10 - 45 atoms in pockets of 350 - 650 atoms", rng.integers(10, 46, 1000), rng.integers(350, 651, 1000), [10] * 100, check=20)
launch_time("one pocket of 1024 samples", rng.integers(10, 46, 1024), [500] * 1024, [1024])
launch_time("worst case, ligands of 1024 atoms in pockets of 8192 atoms", [1024] * 100, [8192] * 100, [10] * 10, check=1)
print("RESULT", json.dumps(results))
