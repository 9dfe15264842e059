"""bench.py as the driver runs it: the JSON contract, and the N-rank path on the hardware at hand (two ranks sharing
the one GPU of a gpurun box over gloo -- RCCL needs one GPU per rank; the 8-GPU run is the driver's)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=600):
    e = dict(os.environ)
    for k in ("MASTER_ADDR", "MASTER_PORT", "CBGX_RDZV_FILE", "RANK", "WORLD_SIZE", "LOCAL_RANK"):   # no rendezvous leaks in from outside
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e,
                       timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_contract_small_job():
    out = _run(["--full", "--steps", "2", "--warmup", "1", "--pockets", "4", "--graphs-per-batch", "20", "--no-cpu-baseline"])
    assert "secondary" not in out          # only the default (driver) workload carries the secondary block
    assert "profiles/traffic_x2h.json" in out["roofline"]["traffic_source"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1 and out["dtype"] == "f32"
    cfg = out["config"]
    assert cfg["graphs_per_gpu"] == 40 and cfg["denoising_steps_per_bench_step"] == 5 and cfg["ranks_seen"] == 1
    # value is consistent with ms_per_step: graphs x 5 denoising steps per bench step
    assert abs(out["value"] - 40 * 5 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    r = out["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1.5 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4



@pytest.mark.parametrize("workload", ["denovo", "train"])
def test_plain_bench_line_and_dumped_outputs(workload, tmp_path):
    """a plain run (no --full) measures the headline only; --dump-outputs writes what the last timed step computed, as float32"""
    args = ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    args += ["--pockets", "4", "--graphs-per-batch", "20"] if workload == "denovo" else ["--workload", "train", "--pockets", "4"]
    out = _run(args)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["dtype"] == "f32"
    for k in ("roofline", "cpu_baseline", "secondary"):
        assert k not in out, k
    import numpy as np
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    if workload == "denovo":
        assert sorted(got) == ["c_lig", "x_lig"]
        n_lig = got["x_lig"].shape[0]
        assert got["x_lig"].shape == (n_lig, 3) and got["c_lig"].shape == (n_lig, 13) and 40 * 10 <= n_lig <= 40 * 45
    else:
        assert {"loss", "grad_norm", "grads", "params"} <= set(got) and got["grads"].shape == got["params"].shape
        assert got["params"].size > 1_000_000 and got["loss"].shape == (1,)

def test_bench_one_rank_through_rccl():
    """the collectives of the N-GPU job on the backend the driver's run uses: a one-rank RCCL group (CBGX_DIST_FORCE=1) takes
    bench.py through init_process_group('nccl'), the device identity all-gather, both barriers and the max / sum / count
    all-reduces on the GPU"""
    out = _run(["--steps", "2", "--warmup", "1", "--pockets", "2", "--graphs-per-batch", "20", "--no-cpu-baseline", "--no-roofline"],
               env={"CBGX_DIST_FORCE": "1", "CBGX_DIST_BACKEND": "nccl", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert out["n_gpus"] == 1 and "ranks" not in out and out["config"]["ranks_seen"] == 1
    assert out["config"]["collective_backend"] == "nccl"
    assert abs(out["value"] - 20 * 5 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]


def test_bench_train_one_rank_through_rccl():
    """the flat-buffer gradient all-reduce (cbgbench_amd/train.py FlatGrads.all_reduce_mean) on RCCL, one rank"""
    out = _run(["--workload", "train", "--steps", "2", "--warmup", "1", "--pockets", "4", "--no-cpu-baseline", "--no-roofline"],
               env={"CBGX_DIST_FORCE": "1", "CBGX_DIST_BACKEND": "nccl", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert out["n_gpus"] == 1 and out["config"]["ranks_seen"] == 1 and out["config"]["collective_backend"] == "nccl"
    assert out["config"]["allreduce_ms_per_step"] > 0


def test_bench_two_ranks_on_one_gpu_gloo():
    """`python bench.py --gpus 2` launches two ranks itself; both take part (ranks_seen from an all-reduce), the value is
    the whole-job aggregate.  gloo because both ranks share this box's single GPU."""
    out = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--pockets", "2", "--graphs-per-batch", "20",
                "--no-cpu-baseline", "--no-roofline"], env={"CBGX_DIST_BACKEND": "gloo"})
    # two ranks, ONE physical GPU: the line says so instead of claiming n_gpus = 2
    assert out["n_gpus"] == 1 and out["ranks"] == 2 and out["config"]["ranks_seen"] == 2
    assert abs(out["value"] - 2 * 20 * 5 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]


def test_bench_split_job_two_ranks_gloo():
    """--split-job: ONE job's pockets dealt over the ranks (strong scaling, what sample.py:159's pocket loop gives a user who adds
    GPUs): 5 pockets x 10 samples over two ranks = 3 + 2 pockets, 50 graphs in total, not 50 per rank"""
    out = _run(["--gpus", "2", "--split-job", "--steps", "2", "--warmup", "1", "--pockets", "5", "--graphs-per-batch", "20",
                "--no-cpu-baseline", "--no-roofline"], env={"CBGX_DIST_BACKEND": "gloo"})
    assert out["ranks"] == 2 and out["config"]["ranks_seen"] == 2 and out["scaling"] == "strong"
    assert out["config"]["graphs_per_gpu"] == 30            # rank 0 holds pockets 0, 2, 4
    assert abs(out["value"] - 50 * 5 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]


def test_bench_train_two_ranks_on_one_gpu_gloo():
    out = _run(["--gpus", "2", "--workload", "train", "--steps", "2", "--warmup", "1", "--pockets", "4",
                "--no-cpu-baseline", "--no-roofline"], env={"CBGX_DIST_BACKEND": "gloo"})
    assert out["n_gpus"] == 1 and out["ranks"] == 2 and out["config"]["ranks_seen"] == 2
    assert out["config"]["allreduce_ms_per_step"] > 0


def test_bench_refuses_shared_gpus_without_the_gloo_declaration():
    """RCCL needs one GPU per rank: two ranks on this box's single GPU must be refused, not reported as n_gpus = 2"""
    e = dict(os.environ)
    e.pop("CBGX_DIST_BACKEND", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--pockets",
                        "1", "--graphs-per-batch", "10", "--no-cpu-baseline", "--no-roofline"], capture_output=True, text=True,
                       env=e, timeout=600, cwd=ROOT)
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("workload", ["denovo", "train"])
def test_bench_eight_ranks_dry_run_gloo(workload):
    """the driver's 8-GPU entry (`python bench.py --gpus 8 ...`) on the one GPU at hand, tiny job: eight ranks start, build their
    own jobs, meet at the barriers, all take part in the reductions (and, training, in the gradient all-reduce)"""
    args = ["--gpus", "8", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-roofline"]
    args += ["--pockets", "1", "--graphs-per-batch", "10"] if workload == "denovo" else ["--workload", "train", "--pockets", "2"]
    out = _run(args, env={"CBGX_DIST_BACKEND": "gloo"}, timeout=900)
    assert out["ranks"] == 8 and out["n_gpus"] == 1 and out["config"]["ranks_seen"] == 8
    per_rank = 10 * 5 if workload == "denovo" else 2
    assert abs(out["value"] - 8 * per_rank / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]


def test_sample_cli_two_ranks_write_disjoint_pocket_files(tmp_path):
    """sample.py:159's pocket loop sharded over two ranks (gloo, one GPU): every pocket is written exactly once, by the rank
    that owns it (round-robin), and both ranks' files are complete"""
    import torch
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    e = dict(os.environ, CBGX_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "cbgbench_amd.launch", "--nproc", "2", "-m", "cbgbench_amd.sample_cli", "--config", cfg, "--out_root",
           str(tmp_path), "--synthetic", "5", "--pockets_per_batch", "2", "--random_init"]
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    files = sorted(os.listdir(tmp_path / "targetdiff_T20"))
    assert files == [f"pocket_{i:05d}.pt" for i in range(5)]
    for i, f in enumerate(files):
        rec = torch.load(tmp_path / "targetdiff_T20" / f, weights_only=False)
        assert rec["pocket_index"] == i and len(rec["samples"]) == 4
    assert "on 2 rank(s)" in p.stdout


def test_two_bench_launches_at_once_on_one_box():
    """the collision case that stopped round 5's suite: two `bench.py --gpus 2` jobs started in the same instant.  The launcher's
    rendezvous is a FileStore path per job (cbgbench_amd/launch.py), so there is no port for the two to race for"""
    import threading
    res = [None, None]

    def go(i):
        try:
            res[i] = _run(["--gpus", "2", "--steps", "1", "--warmup", "1", "--pockets", "1", "--graphs-per-batch", "10",
                           "--no-cpu-baseline", "--no-roofline"], env={"CBGX_DIST_BACKEND": "gloo"})
        except BaseException as e:      # noqa: BLE001 -- reported by the assert below, in the main thread
            res[i] = e

    th = [threading.Thread(target=go, args=(i,)) for i in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    for out in res:
        assert isinstance(out, dict), out
        assert out["ranks"] == 2 and out["config"]["ranks_seen"] == 2


def test_bench_under_the_drivers_torchrun_entry():
    """the driver's own N-GPU command line (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...`): RANK / WORLD_SIZE / MASTER_* come from that launcher and bench.py must not start ranks of
    its own.  The port is the caller's to choose (here: the test standing in for the driver, so the test retries a taken port)"""
    import socket
    err = ""
    for _ in range(3):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        e = dict(os.environ, CBGX_DIST_BACKEND="gloo")
        for k in ("CBGX_RDZV_FILE", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
            e.pop(k, None)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--pockets",
               "1", "--graphs-per-batch", "10", "--no-cpu-baseline", "--no-roofline"]
        p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
        err = p.stderr[-2000:]
        if p.returncode == 0 or "EADDRINUSE" not in p.stderr:
            break
    assert p.returncode == 0, err
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["ranks"] == 2 and out["config"]["ranks_seen"] == 2 and out["config"]["collective_backend"] == "gloo"
