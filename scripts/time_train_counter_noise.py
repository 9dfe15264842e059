"""Time training steps with the torch generator (default) and in counter mode (times and noise as functions of (seed, example,
iteration), cbgbench_amd/noise.py) on one build: steps of 32 graphs of real-size pockets, all three model classes, the two modes
ALTERNATING `--rounds` times per class.  Prints one JSON line per (model, round, mode) and a summary line per model with the median ms per
step of each mode, their ratio (counter / torch) and the spread of each mode (max - min over its rounds, relative to the median).
The batch is bench.py's training batch plus what train_cli's collate adds in counter mode (example indices on the host, the ligand CSR
on the device); counter mode builds a fresh CounterNoise every step, as the driver does.

    python scripts/time_train_counter_noise.py --steps 20 --warmup 5 --rounds 5
    rocprofv3 --kernel-trace --stats -- python scripts/time_train_counter_noise.py --models targetdiff --modes counter --rounds 1   # launches of one mode"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cbgbench_amd import noise as N, synthetic, train as TRN  # noqa: E402


def run_steps(model, batch, opt, fg, weights, mode, steps, warmup, it0):
    def step(it):
        kw = {"noise": N.training_noise(2022, batch["example_index"], it)} if mode == "counter" else {}
        TRN.train_step(model, batch, opt, fg, weights, 8.0, **kw)
    for k in range(warmup):
        step(it0 + k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(it0 + warmup + k)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--models", default="targetdiff,diffbp,diffsbdd")
    ap.add_argument("--modes", default="torch,counter", help="one mode alone: for a kernel trace of that mode (rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.models.split(","):
        model = bench.make_model(dev, name=name).train()
        fg = TRN.FlatGradients(model)
        opt = TRN.get_optimizer(types.SimpleNamespace(type="adam", lr=5e-4, weight_decay=0.0, beta1=0.95, beta2=0.999), model)
        weights = {"pos": 1.0, "atom": 100.0} if name == "targetdiff" else None
        batch = synthetic.batch_to(bench.build_batch(args.graphs, 1, seed=3000, num_classes=model.num_classes), dev)
        counts = torch.bincount(batch["ligand_element_batch"], minlength=args.graphs).cpu()
        batch["num_graphs"], batch["max_ligand_atoms"] = args.graphs, int(counts.max())
        batch["example_index"] = np.arange(args.graphs)
        batch["ligand_ptr"] = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).to(torch.int32).to(dev)
        modes = args.modes.split(",")
        ms = {m: [] for m in modes}
        it = 1
        for m in modes:                                  # every mode warm before the first timed round
            run_steps(model, batch, opt, fg, weights, m, 3, 3, it)
        for r in range(args.rounds):
            for m in modes:
                torch.manual_seed(2024 + r)
                v = run_steps(model, batch, opt, fg, weights, m, args.steps, args.warmup, it)
                it += args.steps + args.warmup
                ms[m].append(v)
                print(json.dumps({"model": name, "round": r, "mode": m, "ms_per_step": round(v, 4)}), flush=True)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"model": name, "graphs": args.graphs,
                          "nodes": int(batch["protein_pos"].shape[0] + batch["ligand_pos"].shape[0]),
                          "median_ms_per_step": {k: round(v, 4) for k, v in med.items()},
                          "ratio_counter_over_torch": round(med["counter"] / med["torch"], 4) if len(med) == 2 else None,
                          "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                          "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}), flush=True)


if __name__ == "__main__":
    main()
