"""A/B of sample_cli's report path between two checkouts of cbgbench_amd/ that share one libcbgx.so (CBGX_LIBRARY): whichever package
is first on PYTHONPATH runs.  The T = 20 fixture config, three synthetic pockets x two samples, --noise counter, one pocket per batch.

    python scripts/ab_sample_reports.py ckpt CKPT                       one random checkpoint for every run
    python scripts/ab_sample_reports.py run OUT CKPT [report flags]     one sample_cli job: OUT/<files>, OUT/stdout.txt, OUT/stats.json
    python scripts/ab_sample_reports.py compare OUT_A OUT_B             files, key order, tensors, bytes and printed report lines
    python scripts/ab_sample_reports.py times OUT ...                   the write phase and every report's seconds of each run

(profiles/ab_sample_reports.log)"""
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
REPORTS = ("geometry", "bonds", "rings", "aromatic", "distributions")


def same(a, b, where, out):
    """walk two saved objects: same types, same key order, tensors equal in dtype, shape and value (nan == nan: the cosine of a
    degenerate angle); every difference is appended to ``out``"""
    if type(a) is not type(b):
        out.append(f"{where}: {type(a).__name__} vs {type(b).__name__}")
    elif isinstance(a, dict):
        if list(a) != list(b):
            out.append(f"{where}: keys {list(a)} vs {list(b)}")
        for k in a:
            if k in b:
                same(a[k], b[k], f"{where}.{k}", out)
    elif isinstance(a, (list, tuple)):
        if len(a) != len(b):
            out.append(f"{where}: {len(a)} vs {len(b)} entries")
        for k, (u, v) in enumerate(zip(a, b)):
            same(u, v, f"{where}[{k}]", out)
    elif torch.is_tensor(a):
        ok = a.dtype == b.dtype and a.shape == b.shape and (
            torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()) if a.is_floating_point() else torch.equal(a, b))
        if not ok:
            out.append(f"{where}: tensors differ")
    elif a != b and not (isinstance(a, float) and a != a and b != b):
        out.append(f"{where}: {a!r} vs {b!r}")


def main(argv):
    what = argv[0]
    if what == "ckpt":
        import cbgbench_amd as C
        config, _ = C.load_config(CFG)
        C.set_num_atom_type(config)
        torch.manual_seed(123)
        torch.save({"model": C.get_model(config.model).state_dict()}, argv[1])
    elif what == "run":
        from cbgbench_amd import sample_cli
        out, stats = argv[1], {}
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "stdout.txt"), "w") as f, contextlib.redirect_stdout(f):
            sample_cli.main(["--config", CFG, "--synthetic", "3", "--num_samples", "2", "--checkpoint", argv[2], "--seed", "2024", "--noise",
                             "counter", "--no_translate", "--pockets_per_batch", "1", "--streams", "1", "--out_root", out, "--tag", "job"]
                            + argv[3:], stats=stats)
        with open(os.path.join(out, "stats.json"), "w") as f:
            json.dump(stats, f)
    elif what == "compare":
        a, b = (os.path.join(d, "job") for d in argv[1:3])
        names, diffs = sorted(os.listdir(a)), []
        if names != sorted(os.listdir(b)):
            diffs.append(f"files {names} vs {sorted(os.listdir(b))}")
        for name in names:
            if name.endswith(".pt"):
                same(torch.load(os.path.join(a, name), weights_only=False), torch.load(os.path.join(b, name), weights_only=False), name, diffs)
            else:
                with open(os.path.join(a, name), "rb") as fa, open(os.path.join(b, name), "rb") as fb:
                    if fa.read() != fb.read():
                        diffs.append(f"{name}: bytes differ")
        lines = []
        for d in argv[1:3]:
            with open(os.path.join(d, "stdout.txt")) as f:
                lines.append([ln for ln in f.read().split("\n") if ln.split(":")[0] in REPORTS + ("sdf",)])
        if lines[0] != lines[1]:
            diffs.append("printed report lines differ")
        n = {s: sum(name.endswith(s) for name in names) for s in (".pt", ".sdf", "_summary.json")}
        print(f"{argv[1]} vs {argv[2]}: {n['.pt']} records (key order, dtypes, torch.equal), {n['.sdf']} .sdf and {n['_summary.json']} "
              f"summaries (bytes), {len(lines[0])} printed report lines: " + ("identical" if not diffs else "DIFFERENT"))
        for d in diffs:
            print("  " + d)
        return 1 if diffs else 0
    elif what == "times":
        for d in argv[1:]:
            with open(os.path.join(d, "stats.json")) as f:
                stats = json.load(f)
            print(f"{d}: " + ", ".join(f"{k} {1e3 * stats[k]:.2f} ms" for k in ("write",) + REPORTS if k in stats))
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
