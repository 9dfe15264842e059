"""Counter-based noise of training and validation (cbgbench_amd/noise.py TRAIN_* purposes, ``train_cli --noise counter``), the parts that
need no GPU: the time function of csrc/rng.h built by the host compiler against the numpy model bit for bit, uniqueness of the addresses a
training call and a validation call of each model class draw from, the positioned loader (resume, world sizes), and the refusals."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import noise as N, synthetic, train_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_build_of_the_time_function_equals_the_numpy_model(tmp_path):
    """rng::train_time / rng::scale_word compiled by the host compiler into a stand-alone program
    (tests/train_counter_noise/train_time_host_main.cpp, address and undefined-behaviour sanitizers; nothing is loaded into Python)
    against noise.train_times / noise.scale_word: 1000 seeded keys x n_t in {5, 1000, 1001} at both purpose bases, and the extreme
    words 0 and 0xFFFFFFFF, which give 0 and n_t - 1 (never n_t)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++) to build rng.h with")
    exe = str(tmp_path / "train_time_host")
    src = os.path.join(ROOT, "tests", "train_counter_noise", "train_time_host_main.cpp")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "cbgbench_amd", "csrc"), src, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    keys = N.stream_keys(20241019, np.arange(1000) % 37, np.arange(1000))
    assert np.unique(keys).size == 1000
    lines, expect = [], []
    for n_t in (5, 1000, 1001):
        for base in (0, N.PURPOSE_STRIDE):
            t = N.train_times(keys, n_t, base)
            assert t.dtype == np.int64 and t.min() >= 0 and t.max() < n_t
            lines += [f"T {int(k):x} {base:x} {n_t:x}" for k in keys]
            expect += [f"T {int(v):x}" for v in t]
        for w in (0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF):
            lines.append(f"W {w:x} {n_t:x}")
            expect.append(f"W {int(N.scale_word(w, n_t)):x}")
        assert int(N.scale_word(0, n_t)) == 0 and int(N.scale_word(0xFFFFFFFF, n_t)) == n_t - 1
    # the two bases are different draws
    assert not np.array_equal(N.train_times(keys, 1000, 0), N.train_times(keys, 1000, N.PURPOSE_STRIDE))
    inp = tmp_path / "requests.txt"
    inp.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(inp)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert p.stdout.split("\n")[:-1] == expect


def _distinct(rows):
    return np.unique(rows, axis=0).shape[0] == rows.shape[0]


@pytest.mark.parametrize("C_", [13, 8])
@pytest.mark.parametrize("model_type", ["targetdiff", "diffbp", "diffsbdd"])
def test_no_two_draws_of_a_call_share_an_address(model_type, C_):
    """one training call (iteration 3) and one validation call (T = 20, eval_interval 10) of each class on three graphs, through the
    Python model of the addressing: pairwise distinct, DiffSBDD's four draws per evaluation time included.  The documented exception:
    evaluation times that coincide after truncation to an integer draw at the same addresses -- at T = 20 with 10 times TargetDiff's and
    DiffBP's linspace(0, 19, 10) and DiffSBDD's linspace(1, 20, 10) truncate to distinct integers, so here nothing repeats at all;
    T = 4 shows the exception.  Training (purpose base 0) and validation (base 16) are disjoint even for the same keys."""
    T, lig_ptr = 20, np.array([0, 1, 6, 17])
    nblk_b = 1 if model_type == "diffbp" else (C_ + 3) // 4
    keys = N.training_noise(2024, [7, 30, 3], 3).keys
    tr = N.train_addresses(model_type, keys, lig_ptr, T, C_)
    assert tr.shape == (3 + 17 * (1 + nblk_b), 5) and _distinct(tr)
    assert (tr[:, 3] < N.PURPOSE_STRIDE).all() and set(tr[:, 3].tolist()) == {N.TRAIN_TIME, N.TRAIN_POS_NORMAL, N.TRAIN_PURPOSE_B[model_type]}
    # a given time draws no time, and its per-atom addresses carry it as the step
    given = N.train_addresses(model_type, keys, lig_ptr, T, C_, t_in=[4, 0, 19])
    assert given.shape[0] == tr.shape[0] - 3 and sorted(set(given[:, 2].tolist())) == [0, 4, 19]
    vn = N.validation_noise(2024, [7, 30, 3])
    assert vn.purpose_base == N.PURPOSE_STRIDE and vn.sample_index.tolist() == [0, 0, 0]
    calls = N.validation_addresses(model_type, vn.keys, lig_ptr, T, C_, 10)
    times = N.eval_times(model_type, T, 10)
    assert len(set(times)) == 10 and len(calls) == (20 if model_type == "diffsbdd" else 10)
    if model_type == "diffsbdd":
        assert 0 not in times          # step 0 belongs to the second network call
        # the second call of every evaluation time is the same time-0 draw by definition (the reference draws it afresh; its loss term
        # does not depend on the evaluation time): one copy enters the uniqueness check, the ten copies are equal
        assert all(np.array_equal(calls[1], c) for c in calls[3::2])
        calls = calls[0::2] + calls[1:2]
    va = np.concatenate(calls)
    assert _distinct(va) and (va[:, 3] >= N.PURPOSE_STRIDE).all()
    # validation against training with the SAME keys: disjoint through the purpose base
    same = np.concatenate(N.validation_addresses(model_type, keys, lig_ptr, T, C_, 10)[:1])
    assert _distinct(np.concatenate([tr, same]))
    # the exception: T = 4, ten evaluation times -> repeated integers -> repeated addresses, and only those
    few = N.eval_times(model_type, 4, 10)
    assert len(set(few)) < 10
    calls4 = N.validation_addresses(model_type, vn.keys, lig_ptr, 4, C_, 10)
    if model_type == "diffsbdd":
        calls4 = calls4[0::2]
    for i in range(10):
        for j in range(i):
            both = np.concatenate([calls4[i], calls4[j]])
            assert (np.array_equal(calls4[i], calls4[j]) if few[i] == few[j] else _distinct(both)), (i, j)


def test_numpy_model_of_the_draw_call():
    keys = N.stream_keys(5, [0, 1, 2], [9, 9, 9])
    lig_ptr = np.array([0, 2, 2, 7])
    t, a, b = N.train_draw_model(keys, lig_ptr, 20, 0, 13, N.TRAIN_TYPE_UNIFORM, True)
    assert t.shape == (3,) and a.shape == (7, 3) and b.shape == (7, 13) and b.dtype == np.float32
    # atom 0 of graph 2 at its graph's time = a one-graph call on that graph alone with the time given
    t2, a2, b2 = N.train_draw_model(keys[2:], np.array([0, 5]), 20, 0, 13, N.TRAIN_TYPE_UNIFORM, True, t_in=t[2:])
    assert np.array_equal(a[2:], a2) and np.array_equal(b[2:], b2) and t2.tolist() == t[2:].tolist()
    w = N.words(keys[2:], np.array([0, 5]), int(t[2]), N.TRAIN_TYPE_UNIFORM, 13)
    assert np.array_equal(b2, N.uniforms(w))


# ---- loader and keys ---------------------------------------------------------------------------------------------------------------
def _ids_keys(loaders, it, seed=2022):
    ids = [i for ld in loaders for i in ld.batch(it)]
    return ids, N.training_noise(seed, ids, it).keys.tolist()


def test_positioned_loader_resumes_and_is_world_size_invariant():
    """37 examples (no multiple of anything).  (ids, keys) of iterations 1 .. 40 from a loader that starts at it_first in {2, 13, 38}
    equal those of a loader that has walked from iteration 1.  For a global batch of 8 the union over the ranks of world 2 (batch
    size 4) and of world 4 (batch size 2) is world 1's batch at every iteration, with the same key per example."""
    n = 37
    fresh = train_cli.PositionedLoader(n, 8, seed=2022)
    walked = {it: _ids_keys([fresh], it) for it in range(1, 41)}
    seen = set()
    for it in range(1, 41):
        ids = walked[it][0]
        assert len(ids) == 8 and len(set(ids)) == 8 and all(0 <= i < n for i in ids)
        seen.update(ids)
    assert seen == set(range(n))
    assert fresh.steps == 5 and fresh.position(5) == (0, 4) and fresh.position(6) == (1, 0)
    # every epoch covers every example; different epochs are different permutations
    assert set(sum((walked[it][0] for it in range(1, 6)), [])) == set(range(n))
    assert walked[1][0] != walked[6][0]
    for it_first in (2, 13, 38):
        resumed = train_cli.PositionedLoader(n, 8, seed=2022)
        for it in range(it_first, 41):
            assert _ids_keys([resumed], it) == walked[it], (it_first, it)
    # the same example at another iteration has another key
    ex = walked[1][0][0]
    later = next(it for it in range(2, 41) if ex in walked[it][0])
    assert walked[1][1][0] != walked[later][1][walked[later][0].index(ex)]
    for world, bs in ((2, 4), (4, 2)):
        ranks = [train_cli.PositionedLoader(n, bs, rank=r, world=world, seed=2022) for r in range(world)]
        for it in range(1, 41):
            ids, keys = _ids_keys(ranks, it)
            assert all(len(ld.batch(it)) == bs for ld in ranks)
            assert sorted(ids) == sorted(walked[it][0]), (world, it)
            assert dict(zip(ids, keys)) == dict(zip(*walked[it])), (world, it)
    # validation keys: visit 0, another purpose base, independent of the iteration
    assert N.validation_noise(2022, [3, 4]).keys.tolist() == N.stream_keys(2022, [3, 4], [0, 0]).tolist()


def test_collate_hands_out_the_example_indices_on_request():
    cs = train_cli.ComplexSet(train_cli.synthetic_complexes(5, 0, 13, n_rec_range=(20, 30), n_lig_range=(3, 6)))
    plain, with_ids = cs.collate([4, 1, 2]), cs.collate([4, 1, 2], example_ids=True)
    assert set(with_ids) - set(plain) == {"example_index", "ligand_ptr"}
    assert all(torch.equal(plain[k], with_ids[k]) if torch.is_tensor(plain[k]) else plain[k] == with_ids[k] for k in plain)
    assert isinstance(with_ids["example_index"], np.ndarray) and with_ids["example_index"].tolist() == [4, 1, 2]
    ptr = with_ids["ligand_ptr"]
    assert ptr.dtype == torch.int32 and ptr.tolist() == [0] + torch.bincount(plain["ligand_element_batch"]).cumsum(0).tolist()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _cpu_batch(num_classes=13):
    rng = np.random.default_rng(3)
    pockets = [synthetic.make_pocket(rng, 30, radius=6.0) for _ in range(2)]
    return synthetic.make_batch(pockets, [3, 4], rng, num_classes)


def test_counter_mode_refusals():
    cn = N.training_noise(1, [0, 1], 1)
    # TargetDiff's 'uniform' time sampler has another distribution: refused, not silently replaced
    cfg = C.default_targetdiff_config(13, num_layers=1, num_diffusion_timesteps=20)
    cfg.generator.time_sampler = "uniform"
    with pytest.raises(ValueError, match="time_sampler"):
        C.get_model(cfg).train()(_cpu_batch(), noise=cn)
    models = {"targetdiff": C.get_model(C.default_targetdiff_config(13, num_layers=1, num_diffusion_timesteps=20)),
              "diffbp": C.get_model(C.default_diffbp_config(13, num_layers=1, num_diffusion_timesteps=20)),
              "diffsbdd": C.get_model(C.default_diffsbdd_config(8, num_layers=1, num_diffusion_timesteps=20))}
    for name, m in models.items():
        for mode in (m.train, m.eval):
            mode()
            b = _cpu_batch(8 if name == "diffsbdd" else 13)
            with pytest.raises(ValueError, match="GPU"):          # a CPU batch: the draws are made by GPU kernels
                m(b, noise=cn)
            with pytest.raises(ValueError, match="stream keys"):  # one key per graph
                m(dict(b, num_graphs=2), noise=N.training_noise(1, [0, 1, 2], 1))
            b["ligand_element_batch"] = b["ligand_element_batch"].flip(0)
            with pytest.raises(ValueError, match="sorted by graph"):
                m(b, noise=cn)
    with pytest.raises(SystemExit):
        train_cli.main(["--config", "x.yml", "--noise", "philox"])
    with pytest.raises(ValueError, match="noise must be"):
        train_cli.run(None, "x", None, None, None, ".", noise="philox")
