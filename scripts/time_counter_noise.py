"""Time TargetDiff's reverse steps with the torch generator (default) and in counter mode (noise generated inside the step kernels,
cbgbench_amd/noise.py) on one build: one graph, the reference's 10-graph batch and one 340-graph batch of real-size pockets,
the two modes ALTERNATING `--rounds` times per shape.  Prints one JSON line per (shape, round, mode) and a summary line per shape
with the median ms per step of each mode, their ratio (counter / torch) and the spread of each mode (max - min over its rounds,
relative to the median).

    python scripts/time_counter_noise.py --steps 60 --warmup 10 --rounds 5
    rocprofv3 --kernel-trace --stats -- python scripts/time_counter_noise.py --shapes 1x1 --modes counter    # per-kernel times of one mode"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cbgbench_amd import noise as N, synthetic  # noqa: E402


def run_steps(model, batch, noise, steps, warmup, T):
    st = model.begin_sampling(batch, keep_trajectory=False, noise=noise)
    t = T - 1
    for _ in range(warmup):
        model.denoise_step(st, t)
        t -= 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.denoise_step(st, t)
        t -= 1
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1x1,1x10,34x10", help="pockets x samples per shape")
    ap.add_argument("--modes", default="torch,counter", help="one mode alone: for a kernel trace of that mode (rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    T = 1000
    assert args.steps + args.warmup <= T
    dev = torch.device("cuda:0")
    model = bench.make_model(dev, T=T)
    for shape in args.shapes.split(","):
        P, S = (int(v) for v in shape.split("x"))
        batch = synthetic.batch_to(bench.build_batch(P, S, seed=1000), dev)
        counter = N.CounterNoise(2024, [p for p in range(P) for _ in range(S)], [s for _ in range(P) for s in range(S)])
        modes = [(m, counter if m == "counter" else None) for m in args.modes.split(",")]
        ms = {m: [] for m, _ in modes}
        for _, noise in modes:                           # every mode warm before the first timed round
            run_steps(model, batch, noise, 5, 5, T)
        for r in range(args.rounds):
            for mode, noise in modes:
                torch.manual_seed(2024 + r)
                v = run_steps(model, batch, noise, args.steps, args.warmup, T)
                ms[mode].append(v)
                print(json.dumps({"graphs": P * S, "round": r, "mode": mode, "ms_per_step": round(v, 4)}), flush=True)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"graphs": P * S, "nodes": int(batch["protein_pos"].shape[0] + batch["ligand_pos"].shape[0]),
                          "median_ms_per_step": {k: round(v, 4) for k, v in med.items()},
                          "ratio_counter_over_torch": round(med["counter"] / med["torch"], 4) if len(med) == 2 else None,
                          "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                          "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}), flush=True)


if __name__ == "__main__":
    main()
