"""Counter-based noise (cbgbench_amd/noise.py, cbgbench_amd/csrc/rng.h), the parts that need no GPU: the numpy model of Philox4x32-10
against the published known-answer vectors, the header built by the host compiler against the model bit for bit, uniqueness of the
addresses a run of each model class draws from, and the placement invariance of ``priors.build_sampling_batch(sample_streams=...)``."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from cbgbench_amd import noise as N, priors, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# (counter, key, output): the Random123 known-answer vectors of philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_numpy_model_reproduces_the_published_vectors():
    for ctr, key, out in KAT:
        assert N.philox4x32_10(np.array(ctr), np.array(key)).tolist() == list(out)
    # vectorised over leading axes, keys broadcast
    got = N.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert got.tolist() == [list(k[2]) for k in KAT]
    # the uniforms: torch.rand's 24-bit grid, in [0, 1), exact in fp32
    u = N.uniforms(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


def test_host_build_of_the_header_equals_the_numpy_model(tmp_path):
    """cbgbench_amd/csrc/rng.h compiled by the host compiler into a stand-alone program (tests/counter_noise/rng_host_main.cpp, with
    the address and undefined-behaviour sanitizers): the words and the uniforms of the three vectors, of 1000 seeded addresses and
    the stream keys of 50 seeded (seed, pocket, sample) equal the numpy model bit for bit.  Nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++) to build rng.h with")
    exe = str(tmp_path / "rng_host")
    src = os.path.join(ROOT, "tests", "counter_noise", "rng_host_main.cpp")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "cbgbench_amd", "csrc"), src, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    rng = np.random.default_rng(20241018)
    lines, expect = [], []
    for ctr, key, out in KAT:
        lines.append("P " + " ".join(f"{v:x}" for v in ctr + key))
        expect.append(["P"] + [f"{v:08x}" for v in out] + [f"{v:08x}" for v in N.uniforms(np.array(out, dtype=np.uint32)).view(np.uint32)])
    keys = rng.integers(0, 1 << 64, size=1000, dtype=np.uint64)
    addr = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64)
    addr[:300, 0] %= 64          # realistic addresses too: small atom indices, steps below 1000, the purposes, a few blocks
    addr[:300, 1] %= 1000
    addr[:300, 2] %= 7
    addr[:300, 3] %= 4
    w = N.philox4x32_10(addr, np.stack([keys & np.uint64(0xFFFFFFFF), keys >> np.uint64(32)], -1))
    u = N.uniforms(w).view(np.uint32)
    for i in range(1000):
        lines.append(f"D {int(keys[i]):x} " + " ".join(f"{int(v):x}" for v in addr[i]))
        expect.append(["D"] + [f"{v:08x}" for v in w[i]] + [f"{v:08x}" for v in u[i]])
    seeds = rng.integers(0, 1 << 63, size=50, dtype=np.uint64)
    seeds[:3] = (0, 2024, (1 << 64) - 1)
    ps = rng.integers(0, 1 << 32, size=(50, 2), dtype=np.uint64)
    for i in range(50):
        lines.append(f"S {int(seeds[i]):x} {int(ps[i, 0]):x} {int(ps[i, 1]):x}")
        expect.append(["S", f"{int(N.stream_keys(int(seeds[i]), [int(ps[i, 0])], [int(ps[i, 1])])[0]):016x}"])
    inp = tmp_path / "addresses.txt"
    inp.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(inp)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    got = [ln.split() for ln in p.stdout.splitlines()]
    assert len(got) == len(expect)
    normal_err = 0.0
    for g, e in zip(got, expect):
        assert g[:len(e)] == e, (g, e)
        if g[0] == "D":      # informative: the host libm's normals against float64 Box-Muller on the same words
            ws = np.array([int(v, 16) for v in g[1:5]], dtype=np.uint32)
            nh = np.array([int(v, 16) for v in g[9:13]], dtype=np.uint32).view(np.float32)
            normal_err = max(normal_err, float(np.abs(nh - N.normals(ws)).max()))
    print(f"host normals vs float64 Box-Muller: max abs error {normal_err:.3e}")
    assert normal_err < 1e-5


@pytest.mark.parametrize("model_type,C", [("targetdiff", 13), ("targetdiff", 8), ("diffbp", 13), ("diffbp", 8), ("diffsbdd", 13),
                                          ("diffsbdd", 8)])
def test_no_two_draws_of_a_run_share_an_address(model_type, C):
    """a 3-graph, T = 5 run of each class: every (key, counter) the host and the kernels use, through the Python model of the
    addressing (noise.run_addresses), pairwise distinct -- DiffSBDD's initial and final draws included; C = 13 is three full blocks
    and a tail, C = 8 two full blocks.  The components of one call are distinct by construction (four words of one output).
    ``noise.run_addresses`` is a hand-written MODEL of the addressing: the host code does not call it, so this test shows that the
    scheme as specified has no collision; that the host and the kernels follow the scheme is what tests/test_gpu_counter_noise.py
    checks (fill against ``noise.words``, the fused kernels against fill, the samplers' draws against fill)."""
    T = 5
    keys = N.stream_keys(2024, [7, 7, 3], [0, 1, 0])
    assert len(set(keys.tolist())) == 3
    lig_ptr = np.array([0, 1, 6, 17])
    rows = N.run_addresses(model_type, keys, lig_ptr, T, C)
    nblk = (C + 3) // 4
    per_atom = {"targetdiff": T * (1 + nblk), "diffbp": T * 2, "diffsbdd": T * (1 + nblk) + 2 + nblk}[model_type]
    assert rows.shape == (17 * per_atom, 5)
    assert np.unique(rows, axis=0).shape[0] == rows.shape[0]
    # and what the addresses cover is what a fill of each purpose asks for: every component has a call
    for purpose, cols in {"targetdiff": [(N.POS_NORMAL, 3), (N.TYPE_UNIFORM, C)], "diffbp": [(N.POS_NORMAL, 3), (N.MASK_UNIFORM, 1)],
                          "diffsbdd": [(N.POS_NORMAL, 3), (N.TYPE_NORMAL, C), (N.INIT_POS, 3), (N.INIT_TYPE, C), (N.FINAL_POS, 3)]}[model_type]:
        have = rows[(rows[:, 3] == purpose) & (rows[:, 0] == keys[2]) & (rows[:, 1] == 10) & (rows[:, 2] == 0)]
        assert sorted(have[:, 4].tolist()) == list(range((cols + 3) // 4))
    # the words of two different addresses differ (a smoke check of the model, not a proof)
    w = N.words(keys, lig_ptr, 3, N.TYPE_UNIFORM, C)
    assert w.shape == (17, C) and np.unique(w).size == w.size


def test_counter_noise_object():
    cn = N.CounterNoise(2024, [5, 5, 9], [0, 1, 0])
    assert cn.num_graphs == 3 and cn.keys.dtype == np.uint64
    assert cn.keys.tolist() == N.stream_keys(2024, [5, 5, 9], [0, 1, 0]).tolist()
    assert N.CounterNoise(2025, [5], [0]).keys[0] != cn.keys[0]
    assert cn.device_keys("cpu").view(torch.int64).numpy().view(np.uint64).tolist() == cn.keys.tolist()
    with pytest.raises(ValueError):
        N.CounterNoise(1, [0], [0], purpose_base=3)
    with pytest.raises(ValueError):
        N.stream_keys(1, [0, 1], [0])
    with pytest.raises(TypeError):
        N.resolve((torch.zeros(1), torch.zeros(1)))
    with pytest.raises(ValueError, match="GPU"):
        N.attach({}, cn, torch.tensor([0, 1, 2]), 3)


# ---- priors ------------------------------------------------------------------------------------------------------------------
def _pockets():
    rng0 = np.random.default_rng(5)
    pockets = [synthetic.make_pocket(rng0, n) for n in (60, 75, 48)]
    ctx = [synthetic.make_context(rng0, n, 13) for n in (6, 9, 4)]
    return pockets, ctx


def _graph(batch, g):
    """every per-atom field of graph g of a batch"""
    out = {}
    for side in ("ligand", "protein"):
        m = batch[f"{side}_element_batch"] == g
        for k, v in batch.items():
            if torch.is_tensor(v) and k.startswith(side) and not k.endswith("_element_batch"):
                out[k] = v[m]
    return out


@pytest.mark.parametrize("case", ["denovo_uniform", "denovo_zero_mean_gaussian_types", "context"])
def test_streamed_priors_do_not_depend_on_placement(case):
    """graph (p, s) of build_sampling_batch(sample_streams=(seed, ids)): identical for pocket p alone, for p in a batch of three
    pockets in two orders, and for another num_samples (s below both) -- positions, types, size, and the context-task fields"""
    pockets, ctx = _pockets()
    ids = [11, 4, 30]
    kw = {"denovo_uniform": dict(type_prior="uniform", pos_prior="gaussian"),
          "denovo_zero_mean_gaussian_types": dict(type_prior="gaussian", pos_prior="zero_mean_gaussian"),
          "context": dict(type_prior="uniform", pos_prior="zero_mean_gaussian", center_on_context=True,
                          num_dist=priors.NumDist.uniform(5, 12))}[case]      # sizes 5..12 around the context sizes: the top-up runs

    def build(order, S):
        ps = priors.PocketSet([pockets[i] for i in order], device="cpu", center=False)
        c = dict(kw, context=[ctx[i] for i in order]) if case == "context" else kw
        return priors.build_sampling_batch(ps, S, 13, sample_streams=(99, [ids[i] for i in order]), **c)

    full, other, alone, more = build([0, 1, 2], 3), build([2, 0, 1], 3), build([1], 3), build([1, 0], 5)
    if case == "context":
        n = np.bincount(full["ligand_element_batch"].numpy()).reshape(3, 3)
        assert (n > np.array([6, 9, 4])[:, None]).all() and len(set(n.reshape(-1).tolist())) > 2
    for s in range(3):
        ref = _graph(full, 1 * 3 + s)
        assert ref["ligand_pos"].shape[0] >= 1
        for name, (b, g) in {"other order": (other, 2 * 3 + s), "alone": (alone, s), "more samples": (more, 0 * 5 + s)}.items():
            got = _graph(b, g)
            assert sorted(got) == sorted(ref)
            for k in ref:
                assert ref[k].shape == got[k].shape and torch.equal(ref[k], got[k]), (case, s, name, k)
    # the batch carries the stream keys of its graphs, in batch order
    assert full["noise_keys"].keys.tolist() == N.stream_keys(99, np.repeat(ids, 3), np.tile(np.arange(3), 3)).tolist()
    assert other["noise_keys"].keys[6:9].tolist() == full["noise_keys"].keys[3:6].tolist()
    # samples differ from each other, and another seed gives other priors
    a, b = _graph(full, 3), _graph(full, 4)       # the generated atoms of two samples of one pocket (a context task: after the context atoms)
    n_fixed = 9 if case == "context" else 0
    assert not torch.equal(a["ligand_pos"][n_fixed:n_fixed + 1], b["ligand_pos"][n_fixed:n_fixed + 1])
    ps = priors.PocketSet(pockets, device="cpu", center=False)
    c = dict(kw, context=ctx) if case == "context" else kw
    again = priors.build_sampling_batch(ps, 3, 13, sample_streams=(100, ids), **c)
    assert again["ligand_pos"].shape != full["ligand_pos"].shape or not torch.equal(again["ligand_pos"], full["ligand_pos"])


def test_zero_mean_prior_is_centred_per_graph():
    pockets, _ = _pockets()
    ps = priors.PocketSet(pockets, device="cpu", center=False)
    b = priors.build_sampling_batch(ps, 2, 8, sample_streams=(3, [0, 1, 2]), type_prior="zeros", pos_prior="zero_mean_gaussian")
    for g in range(6):
        assert b["ligand_pos"][b["ligand_element_batch"] == g].mean(0).abs().max() < 1e-6
    assert b["ligand_atom_type"].shape[1] == 8 and not b["ligand_atom_type"].any()
    with pytest.raises(ValueError):
        priors.build_sampling_batch(ps, 2, 8, sample_streams=(3, [0, 1]))


def test_default_priors_are_what_the_parent_commit_gives():
    """the default mode (``rng`` / ``generator``) is untouched: digests of every tensor of four batches, produced by the commit before
    ``sample_streams`` existed (tests/golden/priors_default_digests.json)"""
    gold = json.load(open(os.path.join(GOLDEN, "priors_default_digests.json")))
    pockets, ctx = _pockets()
    ps = priors.PocketSet(pockets, device="cpu", center=False)
    cases = {"uniform_gaussian": dict(type_prior="uniform", pos_prior="gaussian"),
             "absorbing_gaussian": dict(type_prior="absorbing", pos_prior="gaussian"),
             "zeros_zero_mean": dict(type_prior="zeros", pos_prior="zero_mean_gaussian"),
             "context_uniform": dict(type_prior="uniform", pos_prior="gaussian", context=ctx, center_on_context=True,
                                     num_dist=priors.NumDist.uniform(5, 12))}
    assert sorted(cases) == sorted(gold)
    for name, kw in cases.items():
        b = priors.build_sampling_batch(ps, 3, 13, rng=np.random.default_rng(7), generator=torch.Generator().manual_seed(11), **kw)
        assert "noise_keys" not in b
        got = {k: hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).hexdigest() for k, v in b.items() if torch.is_tensor(v)}
        assert got == gold[name], (name, [k for k in got if got[k] != gold[name].get(k)])


def test_sample_cli_knows_the_noise_flag():
    from cbgbench_amd import sample_cli
    with pytest.raises(SystemExit):
        sample_cli.main(["--config", "x.yml", "--noise", "philox"])
    pockets, _ = _pockets()
    b = sample_cli.build_pocket_batch(pockets[:2], 2, None, 13, sample_streams=(1, [8, 3]))
    assert b["noise_keys"].pocket_index.tolist() == [8, 8, 3, 3] and b["noise_keys"].sample_index.tolist() == [0, 1, 0, 1]
