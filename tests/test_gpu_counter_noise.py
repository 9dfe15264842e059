"""Counter-based noise on the GPU (cbgx_noise_fill, cbgx_targetdiff_*_rng, the ``noise=`` argument of the three samplers,
``sample_cli --noise counter``): the kernels against the numpy model of cbgbench_amd/noise.py, the fused kernels against
fill + the tape kernels bit for bit, placement invariance of whole trajectories, statistics, and the driver."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, noise as N, priors, synthetic
from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _keys_dev(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def _fill(keys_d, ptr_d, n_lig, cols, uniform, purpose, step, out=None, step_dev=None):
    out = torch.empty(n_lig, cols, dtype=torch.float32, device=DEV) if out is None else out
    _native.check(_native.lib().cbgx_noise_fill(_native.ptr(keys_d), _native.ptr(ptr_d), keys_d.shape[0], n_lig, cols, int(uniform),
                                                purpose, step, _native.ptr(step_dev), _native.ptr(out),
                                                _native.current_stream(DEV)), "cbgx_noise_fill")
    return out


# ---- cbgx_noise_fill against the numpy model ----------------------------------------------------------------------------------
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))      # the largest radius, at the smallest radius uniform 2^-24: sqrt(-2 ln 2^-24) = 5.77
ULP = 2.0 ** -23                                 # one ulp of an fp32 value, relative to the value, at most
NORMAL_BOUND = R_MAX * (
    (2 * ULP / 2 + 1 * ULP)                      # radius: logf within 2 ulp, halved by the square root; sqrtf within 1 ulp     2.4e-7
    + 2 * (ULP / 2)                              # sincosf within 2 ulp of a value of magnitude <= 1 (ulp <= 2^-24)              1.2e-7
    + ULP / 2                                    # the product r * trig, rounded to half an ulp                                  6.0e-8
    + (2.0 ** -22 + 2 * np.pi * 2.8e-8))         # the angle: fl(2 pi) * u rounded to half an ulp of a value below 8 (2^-22),    4.1e-7
#                                                  fl(2 pi) itself 2.8e-8 (relative) off; d(r trig) / d(angle) <= r
# = 5.77 * 8.3e-7 = 4.8e-6


@pytest.mark.parametrize("cols", [13, 8])
def test_noise_fill_matches_the_numpy_model(cols):
    """ligands of 1, 5 and 64 atoms in one call, C in {13, 8}, steps {0, 1, 999}, both kinds of draw.  Uniforms bit-equal.  Normals
    against Box-Muller in float64 on the same uniforms (exact angle 2 pi u), within NORMAL_BOUND, which is built from
      * the radius: r = sqrt(-2 log u_r) <= sqrt(48 ln 2) = 5.77 (u_r >= 2^-24); logf is documented within 2 ulp and sqrtf within 1
        ulp, i.e. a relative error of r of at most (2 * 2^-23) / 2 + 2^-23;
      * sincosf, documented within 2 ulp of a value of magnitude <= 1: 2 * 2^-24 absolute, times r;
      * the rounding of the product r * trig: 2^-24 relative;
      * the fp32 angle: fl(2 pi) differs from 2 pi by 2.8e-8 relative and the product fl(2 pi) * u is rounded to half an ulp of a value
        below 8 (2^-22); an angle error d moves r * trig by at most r * d
    which comes to 4.8e-6 absolute.  A value above it is a formula error, not rounding.  The buffer is pre-filled with NaN and has a
    guard row on either side: finite inside [n_lig, cols], untouched outside."""
    keys = N.stream_keys(2024, [3, 3, 8], [0, 1, 0])
    lig_ptr = np.array([0, 1, 6, 70], dtype=np.int32)
    n_lig = 70
    keys_d, ptr_d = _keys_dev(keys), torch.from_numpy(lig_ptr).to(DEV)
    worst = 0.0
    for step in (0, 1, 999):
        for uniform, purpose in ((True, N.TYPE_UNIFORM), (False, N.TYPE_NORMAL), (False, N.POS_NORMAL)):
            buf = torch.full((n_lig + 2, cols), float("nan"), dtype=torch.float32, device=DEV)
            _fill(keys_d, ptr_d, n_lig, cols, uniform, purpose, step, out=buf[1:n_lig + 1])
            got = buf.cpu().numpy()
            assert np.isnan(got[0]).all() and np.isnan(got[-1]).all()
            got = got[1:-1]
            assert np.isfinite(got).all()
            w = N.words(keys, lig_ptr, step, purpose, 4 * ((cols + 3) // 4))
            if uniform:
                assert np.array_equal(got.view(np.uint32), N.uniforms(w)[:, :cols].view(np.uint32)), (step, purpose)
                assert got.min() >= 0.0 and got.max() < 1.0
            else:
                ur = ((w[:, 0::2] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
                th = 2.0 * np.pi * N.uniforms(w[:, 1::2]).astype(np.float64)
                ref = np.empty(w.shape, dtype=np.float64)
                ref[:, 0::2], ref[:, 1::2] = np.sqrt(-2.0 * np.log(ur)) * np.cos(th), np.sqrt(-2.0 * np.log(ur)) * np.sin(th)
                err = float(np.abs(got - ref[:, :cols]).max())
                worst = max(worst, err)
                assert err <= NORMAL_BOUND, (step, purpose, err, NORMAL_BOUND)
    print(f"normals: max |device - float64 Box-Muller| = {worst:.3e} (bound {NORMAL_BOUND:.3e})")
    # the step from a device int (trajectory / hipGraph mode) is the same draw
    t_dev = torch.tensor([999], dtype=torch.int32, device=DEV)
    a = _fill(keys_d, ptr_d, n_lig, cols, False, N.POS_NORMAL, 999)
    b = _fill(keys_d, ptr_d, n_lig, cols, False, N.POS_NORMAL, 0, step_dev=t_dev)
    assert _same_bits(a, b)
    # argument errors are CBGX_E_INVALID -> ValueError
    with pytest.raises(ValueError):
        _native.check(_native.lib().cbgx_noise_fill(None, _native.ptr(ptr_d), 3, n_lig, cols, 0, 0, 0, None, _native.ptr(a),
                                                    _native.current_stream(DEV)), "cbgx_noise_fill")
    with pytest.raises(ValueError):
        _native.check(_native.lib().cbgx_noise_fill(_native.ptr(keys_d), _native.ptr(ptr_d), 3, n_lig, cols, 0, 0, -1, None,
                                                    _native.ptr(a), _native.current_stream(DEV)), "cbgx_noise_fill")


# ---- the fused TargetDiff kernels against fill + the tape kernels ------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    """ligands of 1, 5 and 33 atoms, C = 13, a partial interleaved gen_flag, T = 20; denoiser outputs are random numbers"""
    T, Cn = 20, 13
    torch.manual_seed(1)
    m = C.get_model(C.default_targetdiff_config(Cn, num_diffusion_timesteps=T)).eval().to(DEV)
    g = torch.Generator().manual_seed(2)
    lig_ptr = np.array([0, 1, 6, 39], dtype=np.int32)
    n_lig, n = 39, 2 * 39 + 3
    d = dict(T=T, C=Cn, n_lig=n_lig, N=n, m=m)
    d["x_den"] = torch.randn(n, 3, generator=g).to(DEV)
    d["logits"] = (3 * torch.randn(n, Cn, generator=g)).to(DEV)
    d["lig_rows"] = (2 * torch.arange(n_lig, dtype=torch.int32) + 1).to(DEV)
    d["x_lig"] = torch.randn(n_lig, 3, generator=g).to(DEV)
    d["c_lig"] = torch.nn.functional.one_hot(torch.randint(0, Cn, (n_lig,), generator=g), Cn).float().to(DEV)
    d["gen"] = (torch.arange(n_lig) % 3 != 1).to(torch.uint8).to(DEV)          # context atoms interleaved with generated ones
    d["keys"] = _keys_dev(N.stream_keys(7, [0, 0, 5], [0, 1, 2]))
    d["lig_ptr"] = torch.from_numpy(lig_ptr).to(DEV)
    d["lig_graph"] = torch.repeat_interleave(torch.arange(3, dtype=torch.int32), torch.tensor([1, 5, 33])).to(DEV)
    ps, ts = m.pos_scheduler, m.type_scheduler
    d["tabs_t"] = [ps.posterior_mean_c0_coef, ps.posterior_mean_ct_coef, ps.posterior_logvar, ts.log_alphas_v,
                   ts.log_one_minus_alphas_v, ts.log_alphas_cumprod_v, ts.log_one_minus_alphas_cumprod_v]
    d["tabs"] = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in d["tabs_t"]])
    e = m.context_embedder
    d["emb"] = [e.ligand_atom_emb.weight, e.ligand_atom_emb.bias, e.ligand_indicator.weight, e.ligand_indicator.bias]
    return d


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@pytest.mark.parametrize("t", [0, 1, 19])
def test_fused_kernels_equal_fill_plus_tape_kernels(step_case, t):
    """cbgx_targetdiff_step_boundary_rng / epilogue_rng / epilogue_traj_rng against cbgx_noise_fill -> the entry of the same name
    without _rng: x_next, c_next, the composed x / h rows and v_next bit for bit, outputs pre-filled with NaN; at t = 0 sigma = 0;
    context rows (gen_flag 0) keep the bits of their state; rows of x / h that are no ligand rows stay untouched"""
    d = step_case
    lib, p, s = _native.lib(), _native.ptr, _native.current_stream(DEV)
    n_lig, Cn, T, n = d["n_lig"], d["C"], d["T"], d["N"]
    eps = _fill(d["keys"], d["lig_ptr"], n_lig, 3, False, N.POS_NORMAL, t)
    u = _fill(d["keys"], d["lig_ptr"], n_lig, Cn, True, N.TYPE_UNIFORM, t)
    head = (p(d["x_den"]), p(d["logits"]), p(d["lig_rows"]), p(d["x_lig"]), p(d["c_lig"]), p(d["gen"]), n_lig, Cn, t, T, d["tabs"])
    rng = (p(d["keys"]), p(d["lig_graph"]), p(d["lig_ptr"]), 3, 0)
    emb = tuple(p(w) for w in d["emb"])
    # -- step_boundary
    a = [_nan(n_lig, 3), _nan(n_lig, Cn), _nan(n, 3), _nan(n, 128)]
    b = [_nan(n_lig, 3), _nan(n_lig, Cn), _nan(n, 3), _nan(n, 128)]
    _native.check(lib.cbgx_targetdiff_step_boundary(*head, p(eps), p(u), p(a[0]), p(a[1]), *emb, p(a[2]), p(a[3]), s), "boundary")
    _native.check(lib.cbgx_targetdiff_step_boundary_rng(*head, *rng, p(b[0]), p(b[1]), *emb, p(b[2]), p(b[3]), s), "boundary_rng")
    for name, x, y in zip(("x_next", "c_next", "x", "h"), a, b):
        assert _same_bits(x, y), ("step_boundary", name, t)
    rows = d["lig_rows"].long()
    other = torch.ones(n, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert torch.isfinite(b[0]).all() and torch.isfinite(b[1]).all() and torch.isfinite(b[2][rows]).all() and torch.isfinite(b[3][rows]).all()
    assert torch.isnan(b[2][other]).all() and torch.isnan(b[3][other]).all()
    ctx = d["gen"] == 0
    assert _same_bits(b[0][ctx], d["x_lig"][ctx]) and _same_bits(b[1][ctx], d["c_lig"][ctx])
    assert not torch.equal(b[1][~ctx], d["c_lig"][~ctx])
    if t == 0:      # sigma = 0: the noise does not enter the positions
        mean = (d["tabs_t"][0][0] * d["x_den"][rows] + d["tabs_t"][1][0] * d["x_lig"])
        assert torch.allclose(b[0][~ctx], mean[~ctx], rtol=0, atol=1e-6)
    # -- epilogue (with v_next)
    a = [_nan(n_lig, 3), _nan(n_lig, Cn), torch.full((n_lig,), -1, dtype=torch.int32, device=DEV)]
    b = [_nan(n_lig, 3), _nan(n_lig, Cn), torch.full((n_lig,), -1, dtype=torch.int32, device=DEV)]
    _native.check(lib.cbgx_targetdiff_epilogue(*head, p(eps), p(u), p(a[0]), p(a[1]), p(a[2]), s), "epilogue")
    _native.check(lib.cbgx_targetdiff_epilogue_rng(*head, *rng, p(b[0]), p(b[1]), p(b[2]), s), "epilogue_rng")
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.equal(b[2].long(), b[1].argmax(-1)) and int(b[2].min()) >= 0
    # -- epilogue_traj: state in slot t + 1, result in slot t, the step from the device int (which the call then decrements)
    trajs = []
    for fused in (False, True):
        tx, tc = _nan(T + 1, n_lig, 3), _nan(T + 1, n_lig, Cn)
        tx[t + 1], tc[t + 1] = d["x_lig"], d["c_lig"]
        t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
        args = (p(d["x_den"]), p(d["logits"]), p(d["lig_rows"]), p(tx), p(tc), p(d["gen"]), n_lig, Cn, p(t_dev), d["tabs"])
        if fused:
            _native.check(lib.cbgx_targetdiff_epilogue_traj_rng(*args, *rng, s), "epilogue_traj_rng")
        else:
            t_fill = t_dev.clone()
            e2 = _fill(d["keys"], d["lig_ptr"], n_lig, 3, False, N.POS_NORMAL, 0, step_dev=t_fill)
            u2 = _fill(d["keys"], d["lig_ptr"], n_lig, Cn, True, N.TYPE_UNIFORM, 0, step_dev=t_fill)
            _native.check(lib.cbgx_targetdiff_epilogue_traj(*args, p(e2), p(u2), s), "epilogue_traj")
        assert int(t_dev) == t - 1
        trajs.append((tx, tc))
    assert _same_bits(trajs[0][0], trajs[1][0]) and _same_bits(trajs[0][1], trajs[1][1])
    assert _same_bits(trajs[1][0][t], b[0]) and _same_bits(trajs[1][1][t], b[1])
    keep = [k for k in range(T + 1) if k not in (t, t + 1)]
    assert torch.isnan(trajs[1][0][keep]).all()
    # argument errors
    with pytest.raises(ValueError):
        _native.check(lib.cbgx_targetdiff_epilogue_rng(*head, None, p(d["lig_graph"]), p(d["lig_ptr"]), 3, 0, p(b[0]), p(b[1]), None, s), "x")
    with pytest.raises(ValueError):
        _native.check(lib.cbgx_targetdiff_step_boundary_rng(*head, p(d["keys"]), p(d["lig_graph"]), p(d["lig_ptr"]), 3, 5, p(b[0]), p(b[1]),
                                                            *emb, p(a[0]), p(a[1]), s), "x")


# ---- placement invariance of whole trajectories -------------------------------------------------------------------------------
T5 = 5


def _model(name):
    if name == "targetdiff":
        m = C.get_model(C.default_targetdiff_config(13, num_diffusion_timesteps=T5)).eval()
        m.load_state_dict(W.synthetic_state_dict(13, 9, seed=0, num_timesteps=T5), strict=True)
    elif name == "diffbp":
        m = C.get_model(C.default_diffbp_config(13, num_diffusion_timesteps=T5)).eval()
        m.load_state_dict(W.synthetic_state_dict_diffbp(13, 9, seed=0, num_timesteps=T5), strict=True)
    else:
        m = C.get_model(C.default_diffsbdd_config(8, num_diffusion_timesteps=T5)).eval()
        m.load_state_dict(W.synthetic_state_dict_diffsbdd(8, 9, seed=0, num_timesteps=T5), strict=True)
    return m.to(DEV)


def _placements(name):
    """four pockets of 40 - 80 atoms x two samples, ligands of 6 - 12 atoms: the full batch, (p3, p1), p1 alone; with the index of
    graph (p1, s1) in each"""
    rng0 = np.random.default_rng(17)
    pockets = [synthetic.make_pocket(rng0, int(rng0.integers(40, 81))) for _ in range(4)]
    ids = [10, 11, 12, 13]
    plan = priors.SamplingPlan.for_model(name)
    Cn = 8 if name == "diffsbdd" else 13

    def build(order):
        ps = priors.PocketSet([pockets[i] for i in order], device=DEV, center=False)
        return priors.build_sampling_batch(ps, 2, Cn, num_dist=priors.NumDist.uniform(6, 12), type_prior=plan.type_prior,
                                           pos_prior=plan.pos_prior, sample_streams=(2024, [ids[i] for i in order]))

    return {"full": (build([0, 1, 2, 3]), 3), "pair": (build([3, 1]), 3), "alone": (build([1]), 1)}


def _graph_traj(traj, g):
    m = traj[-1][2] == g
    return {t: (traj[t][0][m], traj[t][1][m]) for t in traj}


def _assert_same_traj(a, b, what):
    assert sorted(a) == sorted(b) == list(range(-1, T5))
    for t in sorted(a, reverse=True):
        for k, nm in enumerate(("x", "c")):
            assert a[t][k].shape == b[t][k].shape and torch.equal(a[t][k], b[t][k]), (what, "first difference at t", t, nm)


def test_targetdiff_trajectories_do_not_depend_on_placement():
    """graph (p1, s1): the full trajectory is torch.equal across the full batch, the batch (p3, p1), p1 alone -- and across
    use_graph=True, fuse_step_boundary=False, sample_many(streams=2) and two values of NOISE_CHUNK"""
    m = _model("targetdiff")
    pl = _placements("targetdiff")
    ref = _graph_traj(m.sample(pl["full"][0]), pl["full"][1])
    assert not torch.equal(ref[-1][0], ref[T5 - 1][0]) and torch.isfinite(ref[-1][0]).all()
    for name in ("pair", "alone"):
        _assert_same_traj(ref, _graph_traj(m.sample(pl[name][0]), pl[name][1]), name)
    _assert_same_traj(ref, _graph_traj(m.sample(pl["pair"][0], use_graph=True), 3), "use_graph")
    many = m.sample_many([pl["alone"][0], pl["pair"][0], pl["full"][0]], streams=2)
    for k, name in enumerate(("alone", "pair", "full")):
        _assert_same_traj(ref, _graph_traj(many[k], pl[name][1]), f"sample_many[{name}]")
    many = m.sample_many([pl["alone"][0], pl["pair"][0]], streams=2, use_graph=True)
    _assert_same_traj(ref, _graph_traj(many[0], 1), "sample_many graphs[alone]")
    _assert_same_traj(ref, _graph_traj(many[1], 3), "sample_many graphs[pair]")
    try:
        m.fuse_step_boundary = False
        _assert_same_traj(ref, _graph_traj(m.sample(pl["alone"][0]), 1), "fuse_step_boundary=False")
    finally:
        del m.fuse_step_boundary
    for chunk in (1, 3):
        try:
            m.NOISE_CHUNK = chunk
            _assert_same_traj(ref, _graph_traj(m.sample(pl["pair"][0]), 3), f"NOISE_CHUNK={chunk}")
        finally:
            del m.NOISE_CHUNK
    # the explicit argument is the batch's own; another seed is another trajectory; the torch generator is not consumed
    b = {k: v for k, v in pl["alone"][0].items() if k != "noise_keys"}
    _assert_same_traj(ref, _graph_traj(m.sample(b, noise=pl["alone"][0]["noise_keys"]), 1), "noise=")
    other = _graph_traj(m.sample(b, noise=N.CounterNoise(2025, [11, 11], [0, 1])), 1)
    assert not torch.equal(other[-1][0], ref[-1][0])
    torch.manual_seed(0)
    before = torch.cuda.get_rng_state(DEV).clone()
    m.sample(pl["alone"][0])
    assert torch.equal(before, torch.cuda.get_rng_state(DEV))
    # the default mode is still the torch generator: seeded, reproducible, and different from the counter mode
    torch.manual_seed(4)
    t1 = m.sample(b)
    torch.manual_seed(4)
    t2 = m.sample(b)
    assert torch.equal(t1[-1][0], t2[-1][0]) and not torch.equal(_graph_traj(t1, 1)[-1][0], ref[-1][0])
    # replay keeps precedence and excludes noise=
    with pytest.raises(ValueError):
        m.sample(b, noise_tape={}, noise=pl["alone"][0]["noise_keys"])
    with pytest.raises(ValueError):
        m.sample_many([b], noise_tapes=[{}], noise=[pl["alone"][0]["noise_keys"]])
    with pytest.raises(ValueError):
        m.sample(b, noise=N.CounterNoise(1, [0, 1, 2], [0, 0, 0]))     # three keys for two graphs


@pytest.mark.parametrize("name", ["diffbp", "diffsbdd"])
def test_other_classes_trajectories_do_not_depend_on_placement(name):
    """DiffBP and DiffSBDD through ``sample`` and ``sample_many``: graph (p1, s1) across the full batch, (p3, p1) and p1 alone.  The
    draws are compared first (cbgx_noise_fill at the same addresses, bit-equal), then the whole trajectories.  The per-purpose list
    below restates by hand what the host code of each class draws (diffbp.py / diffsbdd.py call ``noise.fill`` with these purposes);
    it is not read from that code."""
    m = _model(name)
    pl = _placements(name)
    Cn = 8 if name == "diffsbdd" else 13
    # the draws of graph (p1, s1) at every step, from each placement's own state
    draws = {}
    for pname, (b, g) in pl.items():
        st = m.begin_sampling(b)
        sel = st["bl"] == g
        per_step = [(N.POS_NORMAL, 3, False), (N.MASK_UNIFORM, 1, True)] if name == "diffbp" else \
                   [(N.POS_NORMAL, 3, False), (N.TYPE_NORMAL, Cn, False), (N.INIT_POS, 3, False), (N.INIT_TYPE, Cn, False), (N.FINAL_POS, 3, False)]
        draws[pname] = [N.fill(st, p, t, cols, uni)[sel] for t in range(T5) for p, cols, uni in per_step]
    for pname in ("pair", "alone"):
        for x, y in zip(draws["full"], draws[pname]):
            assert _same_bits(x, y), (name, pname, "draws")
    ref = _graph_traj(m.sample(pl["full"][0]), pl["full"][1])
    assert torch.isfinite(ref[-1][0]).all()
    for pname in ("pair", "alone"):
        _assert_same_traj(ref, _graph_traj(m.sample(pl[pname][0]), pl[pname][1]), (name, pname))
    many = m.sample_many([pl["alone"][0], pl["pair"][0]], streams=2)
    _assert_same_traj(ref, _graph_traj(many[0], 1), (name, "sample_many[alone]"))
    _assert_same_traj(ref, _graph_traj(many[1], 3), (name, "sample_many[pair]"))
    b = {k: v for k, v in pl["alone"][0].items() if k != "noise_keys"}
    with pytest.raises(ValueError):
        if name == "diffbp":
            m.sample(b, noise_tape={}, noise=pl["alone"][0]["noise_keys"])
        else:
            m.sample(b, noise_draws=[], noise=pl["alone"][0]["noise_keys"])


# ---- statistics (fixed seed: cannot flake) -----------------------------------------------------------------------------------------
def _corr(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))


def test_statistics_of_the_draws():
    """2^18 normals and 2^18 uniforms from cbgx_noise_fill (1024 graphs = samples 0..1023 of one pocket, 64 atoms, 4 components): mean
    and variance within 5 standard errors (5 / sqrt(n), 5 sqrt(2 / n); 5 / sqrt(12 n), 5 / sqrt(180 n)), and absolute sample
    correlation below 5 / sqrt(n) between the streams of adjacent atoms, adjacent steps, adjacent sample indices and of the position
    and type purposes"""
    B, A, K = 1024, 64, 4
    n = B * A * K
    assert n == 1 << 18
    keys_d = _keys_dev(N.stream_keys(2024, np.zeros(B, dtype=np.int64), np.arange(B)))
    ptr_d = (torch.arange(B + 1, dtype=torch.int32) * A).to(DEV)
    z = _fill(keys_d, ptr_d, B * A, K, False, N.POS_NORMAL, 10).double()
    u = _fill(keys_d, ptr_d, B * A, K, True, N.TYPE_UNIFORM, 10).double()
    figures = {"normal mean": (abs(float(z.mean())), 5 / np.sqrt(n)), "normal var": (abs(float(z.var()) - 1), 5 * np.sqrt(2 / n)),
               "uniform mean": (abs(float(u.mean()) - 0.5), 5 / np.sqrt(12 * n)),
               "uniform var": (abs(float(u.var()) - 1 / 12), 5 / np.sqrt(180 * n))}
    z3, u3 = z.view(B, A, K), u.view(B, A, K)
    z_next = _fill(keys_d, ptr_d, B * A, K, False, N.POS_NORMAL, 11).double()
    u_next = _fill(keys_d, ptr_d, B * A, K, True, N.TYPE_UNIFORM, 11).double()
    zt = _fill(keys_d, ptr_d, B * A, K, False, N.TYPE_NORMAL, 10).double()
    for kind, v3, v, nxt in (("normal", z3, z, z_next), ("uniform", u3, u, u_next)):
        figures[f"{kind} adjacent atoms"] = (abs(_corr(v3[:, :-1], v3[:, 1:])), 5 / np.sqrt(B * (A - 1) * K))
        figures[f"{kind} adjacent steps"] = (abs(_corr(v, nxt)), 5 / np.sqrt(n))
        figures[f"{kind} adjacent samples"] = (abs(_corr(v3[:-1], v3[1:])), 5 / np.sqrt((B - 1) * A * K))
    figures["position normal vs type uniform"] = (abs(_corr(z, u)), 5 / np.sqrt(n))
    figures["position normal vs type normal"] = (abs(_corr(z, zt)), 5 / np.sqrt(n))
    figures["components 0 vs 1 (one Box-Muller pair)"] = (abs(_corr(z3[..., 0], z3[..., 1])), 5 / np.sqrt(B * A))
    for k, (got, bound) in figures.items():
        print(f"{k}: {got:.3e} (bound {bound:.3e})")
    for k, (got, bound) in figures.items():
        assert got < bound, (k, got, bound)


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def _records(out_dir):
    files = sorted(os.listdir(out_dir))
    assert files == [f"pocket_{i:05d}.pt" for i in range(3)]
    return [torch.load(os.path.join(out_dir, f), weights_only=False) for f in files]


def _same_records(a, b):
    for ra, rb in zip(a, b):
        if ra["pocket_index"] != rb["pocket_index"] or len(ra["samples"]) != len(rb["samples"]):
            return False
        for sa, sb in zip(ra["samples"], rb["samples"]):
            if sorted(sa) != sorted(sb):
                return False
            for k in sa:
                same = (sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k])) if torch.is_tensor(sa[k]) else sa[k] == sb[k]
                if not same:
                    return False
    return True


def test_sample_cli_counter_noise_does_not_depend_on_the_split(tmp_path):
    """sample_cli --noise counter --random_init on three synthetic pockets x two samples (the T = 20 fixture config): one batch of
    three pockets on one stream, three batches of one pocket on three streams, and the two-rank launch -- every tensor of every
    pocket file equal.  --noise torch differs from them and reproduces itself.  Random initial weights differ from process to process
    (and between the ranks' processes and this one), so one random initialisation is written as a checkpoint in the reference's format
    and every run loads it; the flag stays on the command line."""
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    config, _ = C.load_config(cfg)
    C.set_num_atom_type(config)
    torch.manual_seed(123)
    ckpt = tmp_path / "random_init.pt"
    torch.save({"model": C.get_model(config.model).state_dict()}, ckpt)
    common = ["--config", cfg, "--synthetic", "3", "--num_samples", "2", "--random_init", "--checkpoint", str(ckpt), "--seed", "2024"]

    def run(tag, *extra):
        out = tmp_path / tag
        assert sample_cli.main(common + ["--out_root", str(out)] + list(extra)) == 0
        return _records(out / "targetdiff_T20")

    one = run("one", "--noise", "counter", "--pockets_per_batch", "3", "--streams", "1")
    split = run("split", "--noise", "counter", "--pockets_per_batch", "1", "--streams", "3")
    assert all(len(r["samples"]) == 2 for r in one) and torch.isfinite(one[0]["samples"][0]["pos"]).all()
    assert _same_records(one, split)
    t1 = run("torch1", "--noise", "torch", "--pockets_per_batch", "3", "--streams", "1")
    t2 = run("torch2", "--noise", "torch", "--pockets_per_batch", "3", "--streams", "1")
    assert _same_records(t1, t2) and not _same_records(t1, one)
    # two ranks (gloo, one GPU), as tests/test_gpu_bench.py launches them
    ranks = tmp_path / "ranks"
    e = dict(os.environ, CBGX_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "cbgbench_amd.launch", "--nproc", "2", "-m", "cbgbench_amd.sample_cli"] + common + \
          ["--out_root", str(ranks), "--noise", "counter", "--pockets_per_batch", "2"]
    p = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "on 2 rank(s)" in p.stdout
    assert _same_records(one, _records(ranks / "targetdiff_T20"))
