"""Cost of the interaction report on one MI355X (profiles/interactions_measure.log):
sample_cli --synthetic 100 --num_samples 10 (the BASELINE configs[1] job shape: 1000 graphs) with --interactions, stats["interactions"]
next to stats["sample"] -- alone (the report then pays for the bond list, the ring, aromatic and valence reports it is computed from) and
beside --bonds --rings --aromatic --valence (its own two launches and its download); then both launches alone, from HIP events after a
warm-up launch: on the job's own 1000 graphs in their own pockets (random weights: collapsed samples), and on the 1000 seeded
molecule-like graphs of 10 - 45 atoms of tests/test_valence.py in seeded residue-shaped pockets of 350 - 650 atoms (what a trained
model's samples look like), the first 50 of them held against the model.

    python scripts/interactions_measure.py [out_dir]"""
import os, sys, time, json, random, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cbgbench_amd import sample_cli, _native, geometry as G, synthetic
from tests import interactions_model as IM
from tests.test_interactions import assemble, ligand_coordinates, make_pocket
from tests.test_valence import seeded_sets

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="interactions_measure_")
cfg = os.path.join("tests", "fixtures", "targetdiff_test.yml")
dev = torch.device("cuda:0")
print("device", torch.cuda.get_device_name(0), flush=True)
common = ["--config", cfg, "--num_samples", "10", "--random_init", "--no_translate"]
# a small run first: code objects are loaded and the allocator is warm before the timed runs
sample_cli.main(common + ["--synthetic", "10", "--interactions", "--valence", "--bonds", "--out_root", os.path.join(out, "warmup")])
results = {}
for tag, flags in (("alone", ["--interactions"]), ("beside", ["--interactions", "--bonds", "--rings", "--aromatic", "--valence"])):
    stats = {}
    torch.manual_seed(0)
    t0 = time.perf_counter()
    sample_cli.main(common + ["--synthetic", "100", "--out_root", os.path.join(out, tag)] + flags, stats=stats)
    torch.cuda.synchronize()
    res = {k: round(float(v), 4) for k, v in stats.items() if isinstance(v, (int, float))}
    res["wall"] = round(time.perf_counter() - t0, 4)
    results[tag] = res
    print(f"job, --interactions {tag}", json.dumps(res), flush=True)
d = os.path.join(out, "beside", "targetdiff_test")
print(open(os.path.join(d, "interactions_summary.json")).read())


def timed(call, reps):
    assert call() == 0                               # warm-up launch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        assert call() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def launch_times(name, args, pocket, check=0, reps=10):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)
    n_lig, n_rec, B, nb = len(args["z_lig"]), len(pocket["z_rec"]), len(args["lig_ptr"]) - 1, args["bond_index"].shape[1]
    xr, zr, rp, aa, bb = (t(pocket[k], dt) for k, dt in (("x_rec", np.float32), ("z_rec", np.uint8), ("rec_ptr", np.int32),
                                                         ("rec_aa", np.uint8), ("rec_backbone", np.uint8)))
    xl, zl, lp, bp, bi, bk, ih, af, vs = (t(args[k], dt) for k, dt in (
        ("x_lig", np.float32), ("z_lig", np.uint8), ("lig_ptr", np.int32), ("bond_ptr", np.int32), ("bond_index", np.int32),
        ("bond_kekule", np.uint8), ("implicit_h", np.uint8), ("atom_flags", np.uint8), ("valence_status", np.int32)))
    rt = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    at, gt = torch.empty(n_lig, 5, dtype=torch.float64, device=dev), torch.empty(B, 5, dtype=torch.float64, device=dev)
    lt, br = torch.empty(n_lig, dtype=torch.uint8, device=dev), torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    gc = torch.empty(B, IM.COLS, dtype=torch.int32, device=dev)
    p, lib, st = _native.ptr, _native.lib(), _native.current_stream(dev)
    us_pocket = timed(lambda: lib.cbgx_pocket_types(p(xr), p(zr), p(rp), n_rec, B, p(aa), p(bb), p(rt), st), reps)
    us_lig = timed(lambda: lib.cbgx_ligand_interactions(p(xl), p(zl), p(lp), n_lig, p(xr), p(rt), p(rp), n_rec, B, p(bp), p(bi) if nb else None,
                                                        p(bk) if nb else None, None, nb, p(ih), p(af), p(vs), p(at), p(lt), p(br), p(gt), p(gc),
                                                        st), reps)
    g, terms = gc.cpu().numpy(), gt.cpu().numpy()
    ok = g[:, -1] == 0
    s = G.summarise_interactions(g, terms)
    line = (f"{name}: {B} graphs, {n_lig} ligand atoms, {n_rec} pocket atoms, {nb} bonds; HIP events, mean of {reps} launches after a "
            f"warm-up launch: cbgx_pocket_types {us_pocket:.1f} us, cbgx_ligand_interactions {us_lig:.1f} us; evaluated {int(ok.sum())}, not "
            f"evaluated {int((~ok).sum())} (status bits {sorted(set(g[~ok][:, -1].tolist()))}); pairs within 8 A {int(g[ok][:, 6].sum())}, "
            f"mean_score {s['mean_score']:.4f}, hbond / hydrophobic / close pairs per molecule {s['hbond_pairs_per_mol']:.2f} / "
            f"{s['hydrophobic_pairs_per_mol']:.2f} / {s['close_pairs_per_mol']:.2f}, rotatable per molecule {s['rotatable_per_mol']:.2f}")
    if check:
        n, m, r = int(args["lig_ptr"][check]), int(args["bond_ptr"][args["lig_ptr"][check]]), int(pocket["rec_ptr"][check])
        want = IM.batch_interactions(args["x_lig"][:n], args["z_lig"][:n], args["lig_ptr"][:check + 1], pocket["x_rec"][:r], rt.cpu().numpy()[:r],
                                     pocket["rec_ptr"][:check + 1], args["bond_ptr"][:n + 1], args["bond_index"][:, :m], args["bond_kekule"][:m],
                                     None, args["implicit_h"][:n], args["atom_flags"][:n], args["valence_status"][:check])
        types = IM.pocket_types(pocket["x_rec"][:r], pocket["z_rec"][:r], pocket["rec_ptr"][:check + 1], pocket["rec_aa"][:r],
                                pocket["rec_backbone"][:r])
        err = np.abs(terms[:check] - want["graph_terms"])
        same = (np.array_equal(g[:check], want["graph_out"]) and np.array_equal(lt.cpu().numpy()[:n], want["lig_type"])
                and np.array_equal(rt.cpu().numpy()[:r], types) and bool((err <= 1e-9 * want["graph_abs"]).all()))
        line += (f"; first {check} graphs equal the model (integers ==, terms within 1e-9 of sum|addends|): {same}; largest "
                 f"|device - model| / sum|addends| {float((err / np.maximum(want['graph_abs'], 1e-300)).max()):.2e}")
    print(line, flush=True)


# (1) molecule-like graphs in residue-shaped pockets of the job's size
rng = random.Random(2025)
cases = list(seeded_sets()[0])
pockets = [make_pocket(rng, rng.randint(350, 650), ("Se",) if g == 0 else ()) for g in range(len(cases))]
args, pocket = assemble(cases, pockets, [ligand_coordinates(rng, c[0]) for c in cases])
launch_times("molecule-like graphs of 10 - 45 atoms in residue-shaped pockets of 350 - 650 atoms", args, pocket, check=50)

# (2) the job's own graphs (random weights: collapsed samples) in the job's own kind of pocket: the files hold the ligands and the
# valence fields; the pockets are made again as the driver makes them
samples = [s for i in range(100) for s in torch.load(os.path.join(d, f"pocket_{i:05d}.pt"), weights_only=False)["samples"]]
job_cases = [(len(s["atom"]), [tuple(e) for e in s["bond_index"].numpy().T.tolist()], s["atom"], s["bond_order"].tolist(),
              np.where(s["bond_type"].numpy() == 255, 255, s["aromatic_bond"].numpy().astype(np.uint8)).tolist()) for s in samples]
np_rng = np.random.default_rng(0)
job_pockets = []
for g in range(len(samples)):
    if g % 10 == 0:
        pos, feat, aa = synthetic.make_pocket(np_rng, int(np_rng.integers(350, 651)))
        z = np.array([1, 6, 7, 8, 16, 34])[feat[:, :6].argmax(1)]
    job_pockets.append((pos, z, aa, feat[:, 6]))
valence = (np.concatenate([s["implicit_h"].numpy() for s in samples]), np.concatenate([s["valence_flags"].numpy() for s in samples]),
           np.concatenate([s["bond_kekule"].numpy() for s in samples]),
           np.array([[0] * 21 + [s["valence_status"]] for s in samples], np.int32))
args, pocket = assemble(job_cases, job_pockets, [s["pos"].numpy() for s in samples], valence=valence)
launch_times("job graphs (random weights: collapsed samples) in synthetic lattice pockets of 350 - 650 atoms", args, pocket)
print("RESULT", json.dumps(results))
