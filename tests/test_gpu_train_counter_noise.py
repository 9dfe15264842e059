"""Counter-based noise of training and validation on the GPU (cbgx_train_noise_draw, cbgx_targetdiff_train_noise_rng, ``noise=CounterNoise``
in ``forward`` of the three model classes in training and in eval mode, ``validate(noise_for=)``, ``train_cli --noise counter``): the draw
kernel against the numpy model of cbgbench_amd/noise.py, the fused TargetDiff noising against draw + tape kernel bit for bit, the
distribution of the drawn times, placement invariance of the noised inputs, counter mode against the replay of its own draws, validation
as a function of the weights, gradients, and the driver.

    python -m tests.test_gpu_train_counter_noise      # the replay check of every class in this process (the CBGX_FUSED_TRAINING_OPS=0 child)
"""
import os
import statistics
import subprocess
import sys

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, noise as N, synthetic, train_cli
from cbgbench_amd.train import FlatGradients, train_step, validate
from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
T20 = 20
CLASSES = ("targetdiff", "diffbp", "diffsbdd")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _keys_dev(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


# ---- kernel level ----------------------------------------------------------------------------------------------------------------
LIG_PTR = np.array([0, 1, 1, 6, 70, 326], dtype=np.int32)      # ligands of 1, 0, 5, 64 and 256 atoms: an empty graph, a full wave, a
N_LIG, B5 = 326, 5                                              # block boundary at atom 256 of the last ligand's range
KEYS5 = N.stream_keys(2024, [3, 4, 4, 8, 9], [3, 3, 4, 3, 3])


def _draw(keys_d, ptr_d, base, n_t, t_in, t_out, a, b, cols_b, purpose_b, uniform_b, n_graphs=B5, n_lig=N_LIG):
    _native.check(_native.lib().cbgx_train_noise_draw(
        _native.ptr(keys_d), _native.ptr(ptr_d), n_graphs, n_lig, base, n_t, _native.ptr(t_in), _native.ptr(t_out), _native.ptr(a),
        _native.ptr(b), cols_b, purpose_b, int(uniform_b), _native.current_stream(DEV)), "cbgx_train_noise_draw")


@pytest.mark.parametrize("cols_b", [13, 8, 1])
def test_train_noise_draw_matches_the_numpy_model(cols_b):
    """drawn and given times, both purpose bases, uniforms and normals in the second buffer.  t_out bit-equal with the empty graph's entry
    written; uniforms bit-equal; normals within NORMAL_BOUND of tests/test_gpu_counter_noise.py (derived there from the documented
    accuracy of logf / sqrtf / sincosf; the generator and its Box-Muller are the same functions).  Buffers pre-filled with NaN (times:
    -7) with a guard row on either side that stays untouched."""
    from tests.test_gpu_counter_noise import NORMAL_BOUND
    keys_d, ptr_d = _keys_dev(KEYS5), torch.from_numpy(LIG_PTR).to(DEV)
    kinds = [(True, N.TRAIN_MASK_UNIFORM)] if cols_b == 1 else [(True, N.TRAIN_TYPE_UNIFORM), (False, N.TRAIN_TYPE_NORMAL)]
    given = np.array([19, 7, 0, 3, 12], dtype=np.int64)
    worst = 0.0
    for base in (0, N.PURPOSE_STRIDE):
        for t_in in (None, given):
            for uniform_b, purpose_b in kinds:
                t_buf = torch.full((B5 + 2,), -7, dtype=torch.int64, device=DEV)
                a_buf, b_buf = _nan(N_LIG + 2, 3), _nan(N_LIG + 2, cols_b)
                t_in_d = None if t_in is None else torch.from_numpy(t_in).to(DEV)
                _draw(keys_d, ptr_d, base, T20, t_in_d, t_buf[1:B5 + 1], a_buf[1:N_LIG + 1], b_buf[1:N_LIG + 1], cols_b, purpose_b, uniform_b)
                t_ref, a_ref, b_ref = N.train_draw_model(KEYS5, LIG_PTR, T20, base, cols_b, purpose_b, uniform_b, t_in=t_in)
                t_got, a_got, b_got = t_buf.cpu().numpy(), a_buf.cpu().numpy(), b_buf.cpu().numpy()
                assert t_got[0] == -7 and t_got[-1] == -7 and t_got[1:-1].tolist() == t_ref.tolist(), (base, t_in, t_got)
                if t_in is None:
                    assert ((t_ref >= 0) & (t_ref < T20)).all()
                for got in (a_got, b_got):
                    assert np.isnan(got[0]).all() and np.isnan(got[-1]).all() and np.isfinite(got[1:-1]).all()
                err = float(np.abs(a_got[1:-1] - a_ref).max())
                if uniform_b:
                    assert np.array_equal(b_got[1:-1].view(np.uint32), b_ref.view(np.uint32)), (base, purpose_b)
                    assert b_got[1:-1].min() >= 0.0 and b_got[1:-1].max() < 1.0
                else:
                    err = max(err, float(np.abs(b_got[1:-1] - b_ref).max()))
                worst = max(worst, err)
                assert err <= NORMAL_BOUND, (base, purpose_b, err, NORMAL_BOUND)
    print(f"normals: max |device - float64 Box-Muller| = {worst:.3e} (bound {NORMAL_BOUND:.3e})")
    # either buffer alone, and the times alone
    t1 = torch.full((B5,), -7, dtype=torch.int64, device=DEV)
    a1 = _nan(N_LIG, 3)
    _draw(keys_d, ptr_d, 0, T20, None, t1, a1, None, 0, 0, 0)
    t2 = torch.full((B5,), -7, dtype=torch.int64, device=DEV)
    _draw(keys_d, ptr_d, 0, T20, None, t2, None, None, 0, 0, 0)
    assert torch.equal(t1, t2) and t1.tolist() == N.train_times(KEYS5, T20, 0).tolist()
    a_ref = N.train_draw_model(KEYS5, LIG_PTR, T20, 0)[1]
    assert float(np.abs(a1.cpu().numpy() - a_ref).max()) <= NORMAL_BOUND
    # argument errors are CBGX_E_INVALID -> ValueError
    b1 = _nan(N_LIG, cols_b)
    for bad in (dict(keys_d=None), dict(n_t=0), dict(base=5), dict(base=-16), dict(cols_b=33), dict(purpose_b=16), dict(n_lig=-1),
                dict(t_out=None)):
        kw = dict(keys_d=keys_d, ptr_d=ptr_d, base=0, n_t=T20, t_in=None, t_out=t1, a=a1, b=b1, cols_b=cols_b,
                  purpose_b=N.TRAIN_TYPE_UNIFORM, uniform_b=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            _draw(**kw)


@pytest.fixture(scope="module")
def sched():
    return {Cn: C.get_model(C.default_targetdiff_config(Cn, num_layers=1, num_diffusion_timesteps=T20)).to(DEV) for Cn in (13, 8)}


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("Cn", [13, 8])
def test_fused_targetdiff_noising_equals_draw_plus_tape_kernel(sched, Cn, given):
    """cbgx_targetdiff_train_noise_rng against cbgx_train_noise_draw -> cbgx_targetdiff_train_noise on the filled buffers: x_t, c_t, v_t
    and t_out bit for bit, drawn and given times, a partial interleaved gen flag, outputs pre-filled with NaN / -1 / -7; context
    atoms keep the bits of their state; the empty graph's time is written"""
    m = sched[Cn]
    ps, ts = m.pos_scheduler, m.type_scheduler
    lib, p, s = _native.lib(), _native.ptr, _native.current_stream(DEV)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(N_LIG, 3, generator=g).to(DEV)
    v0 = torch.randint(0, Cn, (N_LIG,), generator=g).to(DEV)
    gen = (torch.arange(N_LIG) % 3 != 1).to(torch.uint8).to(DEV)
    batch = torch.repeat_interleave(torch.arange(B5), torch.from_numpy(np.diff(LIG_PTR)).long()).to(DEV)
    keys_d, ptr_d = _keys_dev(KEYS5), torch.from_numpy(LIG_PTR).to(DEV)
    t_in = torch.tensor([19, 7, 0, 3, 12], dtype=torch.int64, device=DEV) if given else None
    tabs = (p(ps.alphas_cumprod), p(ts.log_alphas_cumprod_v), p(ts.log_one_minus_alphas_cumprod_v))
    for base in (0, N.PURPOSE_STRIDE):
        # route 1: draw, then the tape kernel
        t1 = torch.full((B5,), -7, dtype=torch.int64, device=DEV)
        eps, u = _nan(N_LIG, 3), _nan(N_LIG, Cn)
        _draw(keys_d, ptr_d, base, T20, t_in, t1, eps, u, Cn, N.TRAIN_TYPE_UNIFORM, True)
        a = [_nan(N_LIG, 3), _nan(N_LIG, Cn), torch.full((N_LIG,), -1, dtype=torch.int64, device=DEV)]
        _native.check(lib.cbgx_targetdiff_train_noise(p(x0), p(v0), p(t1), p(batch), p(gen), N_LIG, Cn, *tabs, p(eps), p(u), p(a[0]),
                                                      p(a[1]), p(a[2]), s), "train_noise")
        # route 2: one launch
        t2 = torch.full((B5,), -7, dtype=torch.int64, device=DEV)
        b = [_nan(N_LIG, 3), _nan(N_LIG, Cn), torch.full((N_LIG,), -1, dtype=torch.int64, device=DEV)]
        _native.check(lib.cbgx_targetdiff_train_noise_rng(p(x0), p(v0), p(batch), p(gen), N_LIG, Cn, *tabs, p(keys_d), p(ptr_d), B5, base,
                                                          T20, p(t_in), p(t2), p(b[0]), p(b[1]), p(b[2]), s), "train_noise_rng")
        assert torch.equal(t1, t2) and int(t2.min()) >= 0 and int(t2.max()) < T20
        if given:
            assert torch.equal(t2, t_in)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and torch.equal(a[2], b[2])
        assert torch.isfinite(b[0]).all() and torch.isfinite(b[1]).all() and int(b[2].min()) >= 0
        ctx = gen == 0
        assert _same_bits(b[0][ctx], x0[ctx]) and torch.equal(b[2][ctx], v0[ctx]) and not _same_bits(b[0][~ctx], x0[~ctx])
        assert torch.equal(b[1].argmax(-1), b[2])
    with pytest.raises(ValueError):
        _native.check(lib.cbgx_targetdiff_train_noise_rng(p(x0), p(v0), p(batch), p(gen), N_LIG, Cn, *tabs, None, p(ptr_d), B5, 0, T20, None,
                                                          p(t2), p(b[0]), p(b[1]), p(b[2]), s), "x")
    with pytest.raises(ValueError):
        _native.check(lib.cbgx_targetdiff_train_noise_rng(p(x0), p(v0), p(batch), p(gen), N_LIG, Cn, *tabs, p(keys_d), p(ptr_d), B5, 3, T20,
                                                          None, p(t2), p(b[0]), p(b[1]), p(b[2]), s), "x")


def test_distribution_of_the_drawn_times():
    """2^16 keys (samples 0 .. 65535 of example 0 at seed 2024), n_t = 1000: every value occurs, and the chi-square statistic of the 1000
    bin counts against the uniform expectation 65.536 is below the 1 - 10^-6 quantile of chi^2 with 999 degrees of freedom, by
    Wilson-Hilferty  k (1 - 2 / (9 k) + z sqrt(2 / (9 k)))^3  with z = 4.7534 (the normal quantile of 1 - 10^-6): 1226.13.  The draw is
    a pure function of the seed; the numpy model gives chi^2 = 1040.90 at seed 2024 (inside), and the kernel must give the model's
    times bit for bit."""
    n, n_t = 1 << 16, 1000
    keys = N.stream_keys(2024, np.zeros(n, dtype=np.int64), np.arange(n))
    t = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    _draw(_keys_dev(keys), torch.zeros(n + 1, dtype=torch.int32, device=DEV), 0, n_t, None, t, None, None, 0, 0, 0, n_graphs=n, n_lig=0)
    got = t.cpu().numpy()
    assert np.array_equal(got, N.train_times(keys, n_t, 0))
    counts = np.bincount(got, minlength=n_t)
    assert counts.shape == (n_t,) and counts.min() >= 1
    chi2 = float(((counts - n / n_t) ** 2 / (n / n_t)).sum())
    k, z = n_t - 1, statistics.NormalDist().inv_cdf(1 - 1e-6)
    bound = k * (1 - 2 / (9 * k) + z * (2 / (9 * k)) ** 0.5) ** 3
    print(f"chi^2 = {chi2:.2f}, 1 - 1e-6 quantile of chi^2_999 (Wilson-Hilferty) = {bound:.2f}, counts {counts.min()} .. {counts.max()}")
    assert abs(bound - 1226.13) < 0.01 and chi2 < bound


# ---- model level -----------------------------------------------------------------------------------------------------------------
SIZES = (1, 5, 12, 20, 33, 65)      # ligand atoms of the six examples; 65 > 48 puts DiffBP's fused losses on the _knn entry
SEED = 2024
# noising-derived results.  Not among them: eps_0 / eps_0_com / score_0* of DiffBP's TENSOR path -- the zero-centred noise, whose per-graph mean
# that path takes with index_add's float atomics (the reference's own order-free sum): reproducible up to summation order only, with or
# without counter noise (the fused path sums in a fixed order; its results carry no such entry).
NOISING = ("t", "xt", "vt", "mask_gen", "mask_gen_pos", "mask_gen_atom", "eps_0_pos", "eps_0_atom", "x0", "v0")
NETWORK = ("x_pred", "c_pred", "eps_pred", "eps_pred_com", "eps_pred_pos", "eps_pred_atom", "score_pred", "score_pred_com")
DRAWN = ("xt", "vt", "eps_0", "eps_0_pos", "eps_0_atom")      # entries that change when the noise changes


def _classes(name):
    return 8 if name == "diffsbdd" else 13


def _model(name):
    Cn = _classes(name)
    if name == "targetdiff":
        m = C.get_model(C.default_targetdiff_config(Cn, num_layers=2, num_diffusion_timesteps=T20))
        m.load_state_dict(W.synthetic_state_dict(Cn, 2, seed=0, num_timesteps=T20), strict=True)
    elif name == "diffbp":
        m = C.get_model(C.default_diffbp_config(Cn, num_layers=2, num_diffusion_timesteps=T20))
        m.load_state_dict(W.synthetic_state_dict_diffbp(Cn, 2, seed=0, num_timesteps=T20), strict=True)
    else:
        m = C.get_model(C.default_diffsbdd_config(Cn, num_layers=2, num_diffusion_timesteps=T20))
        m.load_state_dict(W.synthetic_state_dict_diffsbdd(Cn, 2, seed=0, num_timesteps=T20), strict=True)
    return m.to(DEV)


def _job(name):
    """six examples: pockets of 40 - 60 atoms, ligands of SIZES atoms; the 12-atom ligand has an interleaved partial gen flag"""
    rng = np.random.default_rng(11)
    out = []
    for m in SIZES:
        pos, feat, aa = synthetic.make_pocket(rng, int(rng.integers(40, 61)), radius=6.0)
        out.append({"protein_pos": pos, "protein_atom_feature": feat, "protein_aa_type": aa,
                    "ligand_pos": (rng.standard_normal((m, 3)) * 1.5).astype(np.float32),
                    "ligand_atom_type": rng.integers(0, _classes(name), size=m).astype(np.int64),
                    "ligand_gen_flag": (np.arange(m) % 3 != 1) if m == 12 else np.ones(m, bool)})
    return train_cli.ComplexSet(out)


@pytest.fixture(scope="module")
def setups():
    return {name: (_model(name), _job(name)) for name in CLASSES}


def _per_example(res, batch):
    """{example index: {key: the example's part of every per-graph / per-atom result}}"""
    bl, B, n_lig = batch["ligand_element_batch"], batch["num_graphs"], batch["ligand_element_batch"].shape[0]
    out = {}
    for g, ex in enumerate(batch["example_index"].tolist()):
        d = {}
        for k, v in res.items():
            if not torch.is_tensor(v) or v.dim() == 0 or k == "fused_bad":      # (fused_bad: one flag per call, not per graph)
                continue
            if k == "t":
                d[k] = v[g]
            elif v.shape[0] == n_lig:
                d[k] = v[bl == g]
            elif v.shape[0] == B:
                d[k] = v[g]
        out[ex] = d
    return out


def _close(a, b):
    return bool(((a - b).abs() <= 1e-5 + 1e-4 * b.abs()).all())


@pytest.mark.parametrize("name", CLASSES)
def test_noised_inputs_do_not_depend_on_placement(setups, name):
    """training mode, iteration 3: the six examples as one batch, reversed, each alone, split 2 + 4.  Per example: t, xt and every other
    noising-derived result bit-equal across the four; the network-derived results at the suite's forward tolerance (1e-5 + 1e-4 rel),
    with a printed note whether they are bit-equal too.  Gradients are enabled, so the network call is the taped forward and every class
    is on its fused path (DiffBP's fused results carry no network-derived entry)."""
    m, cs = setups[name]
    m.train()
    runs = {"one batch": [[0, 1, 2, 3, 4, 5]], "reversed": [[5, 4, 3, 2, 1, 0]], "alone": [[i] for i in range(6)], "2 + 4": [[0, 1], [2, 3, 4, 5]]}
    got = {}
    for tag, batches in runs.items():
        got[tag] = {}
        for ids in batches:
            batch = cs.collate(ids, DEV, example_ids=True)
            _, res = m(batch, noise=N.training_noise(SEED, batch["example_index"], 3))      # (gradients enabled: the taped forward)
            res = {k: v.detach() if torch.is_tensor(v) else v for k, v in res.items()}
            assert "t" in res and "xt" in res and res["t"].dtype == torch.int64
            got[tag].update(_per_example(res, batch))
    ref = got["one batch"]
    assert sorted(ref) == list(range(6)) and len({int(ref[e]["t"]) for e in ref}) > 1
    for e in range(6):
        assert ref[e]["xt"].shape == (SIZES[e], 3)
    bit_equal = True
    for tag in ("reversed", "alone", "2 + 4"):
        for e in range(6):
            assert sorted(got[tag][e]) == sorted(ref[e]), (tag, e)
            for k, v in ref[e].items():
                w = got[tag][e][k]
                if k in NOISING:
                    assert v.shape == w.shape and torch.equal(v, w), (name, tag, e, k)
                elif k in NETWORK:
                    assert _close(w, v), (name, tag, e, k, float((w - v).abs().max()))
                    bit_equal = bit_equal and torch.equal(v, w)
    have = sorted(k for k in ref[5] if k in NETWORK)
    print(f"{name}: network-derived results {have} bit-equal across placements: {bit_equal if have else 'none in this path'}")
    # the 12-atom example: context atoms keep their positions
    ctx = torch.arange(12, device=DEV) % 3 == 1
    x0 = cs.collate([2], DEV)["ligand_pos"]
    if name == "targetdiff":
        assert torch.equal(ref[2]["xt"][ctx], x0[ctx]) and not torch.equal(ref[2]["xt"][~ctx], x0[~ctx])
    # another iteration, another seed: other noise
    batch = cs.collate([0, 1, 2, 3, 4, 5], DEV, example_ids=True)
    with torch.no_grad():
        other_it = m(batch, noise=N.training_noise(SEED, batch["example_index"], 4))[1]
        other_seed = m(batch, noise=N.training_noise(SEED + 1, batch["example_index"], 3))[1]
    one = _per_example(other_it, batch), _per_example(other_seed, batch)
    assert not torch.equal(one[0][5]["xt"], ref[5]["xt"]) and not torch.equal(one[1][5]["xt"], ref[5]["xt"])


def _drawn_buffers(m, name, batch, cn, t_in=None):
    """the replay arguments of a counter-mode call: the buffers of cbgx_train_noise_draw in the form the class's ``noise=`` tuple takes"""
    ops = N.train_operands(cn, batch, batch["num_graphs"])
    n_lig, Cn = batch["ligand_pos"].shape[0], _classes(name)
    if name == "targetdiff":
        return N.train_draw(ops, n_lig, T20, t_in, Cn, N.TRAIN_TYPE_UNIFORM, True)
    if name == "diffbp":
        t, eps, u = N.train_draw(ops, n_lig, T20, t_in, 1, N.TRAIN_MASK_UNIFORM, True)
        return t, eps, u.view(-1)
    return N.train_draw(ops, n_lig, T20 + 1, t_in, Cn, N.TRAIN_TYPE_NORMAL, False)


def _loss_close(a, b):
    return abs(a - b) <= 2e-5 * abs(b) + 1e-7      # tests/test_gpu_training.py: the fused path against the tensor path


def _check_replay(m, cs, name):
    """model(batch, noise=cn) against model(batch, t=t_drawn, noise=(drawn buffers)): noising-derived results bit-equal, losses close;
    also with the times given (``t=`` combined with a CounterNoise)"""
    m.train()
    if name == "diffsbdd":      # the replay takes its per-graph means in the order the counter mode takes them (DiffSBDD.ordered_means)
        m.ordered_means = True
    batch = cs.collate([3, 0, 5, 2, 1, 4], DEV, example_ids=True)
    cn = N.training_noise(SEED, batch["example_index"], 3)
    given = torch.tensor([0, 19, 7, 3, 12, 1], dtype=torch.int64, device=DEV)
    for t_in in (None, given):
        with torch.no_grad():
            ld, res = m(batch, noise=cn) if t_in is None else m(batch, t=t_in, noise=cn)
            t, eps, b = _drawn_buffers(m, name, batch, cn, t_in)
            ld_r, res_r = m(batch, t=t, noise=(eps, b))
        assert torch.equal(res["t"], t) and (t_in is None or torch.equal(t, t_in))
        assert set(res) - set(res_r) <= {"t", "xt"}
        for k, v in res_r.items():
            if k in NOISING and torch.is_tensor(v):
                assert torch.equal(res[k], v), (name, k)
        for k in ld_r:
            a, r = float(ld[k]), float(ld_r[k])
            print(f"{name} loss({k}): counter {a:.8g} replay {r:.8g}")
            assert np.isfinite(a) and _loss_close(a, r), (name, k, a, r)
    # eval mode: every evaluation time against the replay of its draws
    m.eval()
    with torch.no_grad():
        vn = N.validation_noise(SEED, batch["example_index"])
        _, results = m(batch, noise=vn)
        times = N.eval_times(name, T20, m.cfg.get("eval_interval", 10))
        assert len(results) == len(times)
        for tv, res in zip(times, results):
            t_in = torch.full((6,), tv, dtype=torch.int64, device=DEV)
            assert torch.equal(res["t"], t_in)
            t, eps, b = _drawn_buffers(m, name, batch, vn, t_in)
            if name == "diffsbdd":
                noise = (eps, b) + _drawn_buffers(m, name, batch, vn, torch.zeros_like(t_in))[1:]
                _, res_r = m.get_loss(batch, t_in, noise, evaluate=True)
            else:
                _, res_r = m.get_loss(batch, t_in, (eps, b))
            for k, v in res_r.items():
                if k in NOISING and torch.is_tensor(v):
                    assert torch.equal(res[k], v), (name, tv, k)
    m.train()
    if name == "diffsbdd":
        m.ordered_means = False


@pytest.mark.parametrize("name", CLASSES)
def test_counter_mode_equals_the_replay_of_its_draws(setups, name):
    m, cs = setups[name]
    assert m.fused_training_ops
    _check_replay(m, cs, name)


def test_counter_mode_equals_the_replay_on_the_tensor_paths():
    """the same check with CBGX_FUSED_TRAINING_OPS=0 (every class on its tensor path), in a child process with its own time limit"""
    env = dict(os.environ, CBGX_FUSED_TRAINING_OPS="0")
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_train_counter_noise"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    assert all(f"replay ok: {name} fused=False" in p.stdout for name in CLASSES), p.stdout[-2000:]


class _Recorder:
    """an ``evaluator`` for ``validate`` that keeps every batch's results"""
    evaluators = {"recorded": None}

    def __init__(self):
        self.results = []

    def __len__(self):
        return 1

    def __call__(self, results):
        self.results.append(results)
        return {"recorded": 0.0}


@pytest.mark.parametrize("name", CLASSES)
def test_validation_is_a_function_of_the_weights(setups, name):
    """validate(..., noise_for=validation_noise) twice: the noising-derived results of every batch and evaluation time bit for bit, the
    loss within the tolerance of the replay test; with noise_for=None (the default, as before) the noised inputs of two calls differ.
    DiffSBDD's four buffers per time come from two draw calls at distinct addresses: its two network calls see different noise."""
    m, cs = setups[name]
    batches = lambda: (cs.collate(ids, DEV, example_ids=True) for ids in ([0, 1, 2], [3, 4, 5]))
    noise_for = lambda b: N.validation_noise(SEED, b["example_index"])
    out = []
    for nf in (noise_for, noise_for, None, None):
        rec = _Recorder()
        avg, _ = validate(m, batches(), None, rec, noise_for=nf)
        assert np.isfinite(avg) and len(rec.results) == 2
        out.append((avg, rec.results))
    assert not m.training
    (a0, r0), (a1, r1), (a2, r2), (a3, r3) = out
    print(f"{name}: validation loss {a0:.8g} / {a1:.8g} (counter), {a2:.8g} / {a3:.8g} (torch generator)")
    assert _loss_close(a1, a0)
    n_cmp = 0
    for b0, b1 in zip(r0, r1):
        assert len(b0) == len(b1) == m.cfg.get("eval_interval", 10)
        for e0, e1 in zip(b0, b1):
            assert "t" in e0 and "xt" in e0
            for k, v in e0.items():
                if k in NOISING and torch.is_tensor(v):
                    assert torch.equal(v, e1[k]), (name, k)
                    n_cmp += 1
    assert n_cmp >= 2 * 10 * 3
    # the times of one call draw at different addresses: different noise at different evaluation times
    drawn = [k for k in DRAWN if k in r0[0][0]]
    assert drawn and all(not torch.equal(r0[0][0][k], r0[0][-1][k]) for k in drawn if r0[0][0][k].dtype.is_floating_point)
    # default mode: fresh noise at every call
    drawn = [k for k in DRAWN if k in r2[0][0]]
    assert drawn and any(not torch.equal(r2[0][-1][k], r3[0][-1][k]) for k in drawn)
    m.train()


@pytest.mark.parametrize("name", CLASSES)
def test_gradients_flow_in_counter_mode(name):
    """loss.backward() in counter mode against the replay call's gradients (the suite's gerr: rtol 2e-4, floor 2e-5 of the largest entry),
    then one train_step in counter mode: finite losses, a finite non-zero gradient norm"""
    from tests.test_gpu_training import gerr
    m, cs = _model(name).train(), _job(name)
    batch = cs.collate([0, 1, 2, 3, 4, 5], DEV, example_ids=True)
    cn = N.training_noise(SEED, batch["example_index"], 3)
    grads = []
    for replay in (False, True):
        m.zero_grad(set_to_none=True)
        if replay:
            t, eps, b = _drawn_buffers(m, name, batch, cn)
            ld, _ = m(batch, t=t, noise=(eps, b))
        else:
            ld, _ = m(batch, noise=cn)
        sum(ld.values()).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 50
    msgs = [msg for msg in (gerr(grads[0][k], grads[1][k], k) for k in grads[1]) if msg]
    assert not msgs, msgs[:5]
    m.zero_grad(set_to_none=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    loss, ld, grad_norm, _ = train_step(m, batch, opt, FlatGradients(m), None, noise=cn)
    assert np.isfinite(float(loss)) and all(np.isfinite(float(v)) for v in ld.values())
    assert np.isfinite(float(grad_norm)) and float(grad_norm) > 0.0


def test_train_cli_counter_noise(tmp_path):
    """python -m cbgbench_amd.train_cli --noise counter: two iterations and a validation on 16 synthetic complexes, finite losses"""
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_train_tiny.yml")
    p = subprocess.run([sys.executable, "-m", "cbgbench_amd.train_cli", "--config", cfg, "--synthetic", "16", "--max_iters", "2",
                        "--noise", "counter", "--logdir", str(tmp_path / "logs")], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    train = [l for l in p.stdout.splitlines() if l.startswith("[train]")]
    val = [l for l in p.stdout.splitlines() if l.startswith("[validate]")]
    assert len(train) == 2 and len(val) == 1, p.stdout[-2000:]
    for l in train:
        assert np.isfinite(float(l.split("| loss ")[1].split("|")[0])), l
    assert np.isfinite(float(val[0].split("| loss ")[1].split("|")[0])), val[0]


if __name__ == "__main__":
    for cls in CLASSES:
        mod = _model(cls)
        _check_replay(mod, _job(cls), cls)
        print(f"replay ok: {cls} fused={mod.fused_training_ops}", flush=True)
