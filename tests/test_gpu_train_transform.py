"""Per-visit transforms of training batches on the GPU (csrc/train_transform.hip: cbgx_train_transform, cbgx_train_transform_rng;
``train_cli.apply_plan``): the tape entry against a float64 restatement at every size where a stride, the tree or a fallback can go
wrong, the counter entry against cbgx_noise_fill + the tape entry bit for bit, placement invariance, resume through ``train_cli.run``,
and the identity plan."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, noise as N, synthetic, train_cli
from cbgbench_amd.priors import TrainingPlan
from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SEED = 2022
MODES = ("protein", "context", "ligand", "whole")
SIGMA = float(np.float32(0.1))        # the fp32 value the entry receives
GUARD = 2                             # untouched rows in front of and behind every output

# (protein atoms, ligand atoms, context atoms): protein sizes around the 256-thread stride, the three held atoms per thread (768) and
# beyond (1025: the stash in the output buffer); ligands of 1 ... 65; context none / one / all
SEVEN = [(1, 1, 0), (2, 65, 1), (255, 7, 7), (256, 0, 0), (0, 13, 1), (257, 33, 0), (1025, 64, 64)]
BATCHES = {"seven": SEVEN, "b1_1": [(1, 1, 1)], "b1_2": [(2, 2, 0)], "b1_255": [(255, 3, 1)], "b1_256": [(256, 65, 65)],
           "b1_257": [(257, 5, 0)], "b1_513": [(513, 17, 1)], "b1_1025": [(1025, 65, 0)]}


def _graphs(spec, seed=0):
    """host tensors of a batch: coordinates of magnitude up to ~40 (a frame far from the origin), context atoms spread over the ligand"""
    g = torch.Generator().manual_seed(seed)
    rec_n, lig_n = [s[0] for s in spec], [s[1] for s in spec]
    x_rec = torch.randn(sum(rec_n), 3, generator=g) * 8.0 + torch.tensor([20.0, -13.0, 5.0])
    x_lig = torch.randn(sum(lig_n), 3, generator=g) * 2.0 + torch.tensor([21.0, -12.0, 4.0])
    ctx = torch.cat([torch.zeros(0, dtype=torch.bool)] + [torch.randperm(nl, generator=g) < nc for _, nl, nc in spec])
    ptr = lambda n: torch.tensor([0] + list(np.cumsum(n)), dtype=torch.int32)
    eps = torch.randn(sum(rec_n), 3, generator=g)
    return {"x_rec": x_rec, "x_lig": x_lig, "rec_ptr": ptr(rec_n), "lig_ptr": ptr(lig_n), "ctx": ctx, "eps": eps, "B": len(spec)}


def _guarded(n):
    buf = torch.full((n + 2 * GUARD, 3), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _launch(G, mode, sigma, eps=None, keys=None, base=0, ctx=True):
    """one launch on NaN-filled outputs with guard rows; returns (x_rec_out, x_lig_out, center_out) after checking the guards"""
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in G.items()}
    n_rec, n_lig, B = d["x_rec"].shape[0], d["x_lig"].shape[0], d["B"]
    (rb, ro), (lb, lo), (cb, co) = _guarded(n_rec), _guarded(n_lig), _guarded(B)
    cx = d["ctx"].view(torch.uint8) if ctx else None
    eps = eps.to(DEV).contiguous() if eps is not None else None
    assert eps is None or tuple(eps.shape) == (n_rec, 3)
    head = (_native.ptr(d["x_rec"]), _native.ptr(d["x_lig"]), _native.ptr(d["rec_ptr"]), _native.ptr(d["lig_ptr"]), _native.ptr(cx), B,
            n_rec, n_lig, sigma, MODES.index(mode))
    tail = (_native.ptr(ro), _native.ptr(lo), _native.ptr(co), _native.current_stream(DEV))
    if keys is not None:
        _native.check(_native.lib().cbgx_train_transform_rng(*head, _native.ptr(keys), base, *tail), "cbgx_train_transform_rng")
    else:
        _native.check(_native.lib().cbgx_train_transform(*head, _native.ptr(eps), *tail), "cbgx_train_transform")
    torch.cuda.synchronize()
    for buf, n in ((rb, n_rec), (lb, n_lig), (cb, B)):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), "a guard row was written"
        assert torch.isfinite(buf[GUARD:GUARD + n]).all(), "an output element was not written"
    return ro.clone(), lo.clone(), co.clone()


def _float64(G, mode, sigma, ctx=True):
    """the transform in float64, graph by graph: (x_rec_out, x_lig_out, centre, per-graph largest magnitude that enters a sum)"""
    xr, xl = G["x_rec"].double(), G["x_lig"].double()
    if sigma > 0:
        xr = xr + sigma * G["eps"].double()
    ro, lo, cen, mag = [], [], [], []
    for g in range(G["B"]):
        P = xr[int(G["rec_ptr"][g]):int(G["rec_ptr"][g + 1])]
        L = xl[int(G["lig_ptr"][g]):int(G["lig_ptr"][g + 1])]
        m = G["ctx"][int(G["lig_ptr"][g]):int(G["lig_ptr"][g + 1])]
        if mode == "protein":
            S = P
        elif mode == "whole":
            S = torch.cat([P, L])
        elif mode == "context" and ctx and bool(m.any()):
            S = L[m]
        else:
            S = L
        c = S.mean(0) if S.shape[0] else torch.zeros(3, dtype=torch.float64)
        ro.append(P - c); lo.append(L - c); cen.append(c)
        mag.append(float(torch.cat([P, L, torch.zeros(1, 3, dtype=torch.float64)]).abs().max()))
    return torch.cat(ro), torch.cat(lo), torch.stack(cen), mag


@pytest.fixture(scope="module")
def graphs():
    return {name: _graphs(spec, seed=i) for i, (name, spec) in enumerate(sorted(BATCHES.items()))}


@pytest.mark.parametrize("sigma", [0.0, SIGMA])
@pytest.mark.parametrize("mode", MODES)
def test_tape_entry_against_float64(graphs, mode, sigma):
    """every batch of BATCHES: every coordinate and every centre within 16 * 2^-24 * max|x| of the float64 result, max|x| the largest
    magnitude of the graph's (noised) coordinates.  16 roundings: at 1025 protein atoms a thread adds 5 values, the tree has 8 levels,
    one division, one fma (the noise) and one subtraction; each is relative to a partial result of at most (count so far) * max|x|, and
    the division by the count brings it back to max|x|."""
    worst = 0.0
    for name, G in sorted(graphs.items()):
        got = _launch(G, mode, sigma, eps=G["eps"] if sigma > 0 else None)
        ref_r, ref_l, ref_c, mag = _float64(G, mode, sigma)
        for g in range(G["B"]):
            bound = 16 * 2.0 ** -24 * mag[g]
            r = slice(int(G["rec_ptr"][g]), int(G["rec_ptr"][g + 1]))
            l = slice(int(G["lig_ptr"][g]), int(G["lig_ptr"][g + 1]))
            errs = [(got[0][r].cpu().double() - ref_r[r]).abs().max() if r.stop > r.start else 0.0,
                    (got[1][l].cpu().double() - ref_l[l]).abs().max() if l.stop > l.start else 0.0,
                    (got[2][g].cpu().double() - ref_c[g]).abs().max()]
            err = max(float(e) for e in errs)
            if mag[g] > 0:
                worst = max(worst, err / bound)
            assert err <= bound, (name, mode, sigma, g, err, bound)
        if sigma > 0:      # eps given with sigma == 0 is not applied; NULL eps with sigma == 0 is the same launch
            a = _launch(G, mode, 0.0, eps=G["eps"])
            b = _launch(G, mode, 0.0, eps=None)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
    print(f"{mode} sigma={sigma:g}: worst |kernel - float64| / (16 * 2^-24 * max|x|) = {worst:.3f}")
    # ctx == NULL: no graph has a context atom, so 'context' is 'ligand'
    G = graphs["seven"]
    if mode == "context":
        a, b = _launch(G, "context", 0.0, ctx=False), _launch(G, "ligand", 0.0)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        # graph 1 has one context atom: it sits at the origin afterwards; graph 5 has none: its ligand's mean does
        one = _launch(G, "context", 0.0)
        l1 = slice(int(G["lig_ptr"][1]), int(G["lig_ptr"][2]))
        assert float(one[1][l1][G["ctx"][l1].to(DEV)].abs().max()) == 0.0
    # empty centre sets give the zero vector: graph 3 has no ligand atom, graph 4 no protein atom
    c = _launch(G, mode, 0.0)[2]
    if mode in ("context", "ligand"):
        assert torch.equal(c[3], torch.zeros(3, device=DEV))
    if mode == "protein":
        assert torch.equal(c[4], torch.zeros(3, device=DEV))


def _keys_dev(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def _normal_bound():
    from tests.test_gpu_counter_noise import NORMAL_BOUND
    return NORMAL_BOUND


@pytest.mark.parametrize("base", [0, N.PURPOSE_STRIDE])
def test_rng_entry_equals_fill_plus_tape_entry(graphs, base):
    """both purpose bases, all four modes, every batch: x_rec_out, x_lig_out and center_out of cbgx_train_transform_rng are the bits of
    cbgx_noise_fill (protein CSR, 3 normals, purpose base + 12, step 0) followed by cbgx_train_transform.  The normals themselves --
    read back through a launch on zero coordinates with sigma 1 and an empty centre set -- are the fill's bits and lie within
    NORMAL_BOUND (tests/test_gpu_counter_noise.py) of noise.protein_draw_model."""
    worst = 0.0
    for name, G in sorted(graphs.items()):
        B, n_rec = G["B"], G["x_rec"].shape[0]
        cn = N.training_noise(SEED, 100 + np.arange(B), 3) if base == 0 else N.validation_noise(SEED, 100 + np.arange(B))
        assert cn.purpose_base == base
        keys = _keys_dev(cn.keys)
        eps = torch.empty(n_rec, 3, device=DEV)
        _native.check(_native.lib().cbgx_noise_fill(_native.ptr(keys), _native.ptr(G["rec_ptr"].to(DEV)), B, n_rec, 3, 0,
                                                    base + N.TRAIN_PROTEIN_NORMAL, 0, None, _native.ptr(eps),
                                                    _native.current_stream(DEV)), "cbgx_noise_fill")
        for mode in MODES:
            a = _launch(G, mode, SIGMA, keys=keys, base=base)
            b = _launch(G, mode, SIGMA, eps=eps)
            for x, y, what in zip(a, b, ("x_rec_out", "x_lig_out", "center_out")):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, mode, what)
        # the drawn normals: 0 + 1 * eps, centre of an empty set (no ligand atom) = 0
        Z = dict(G, x_rec=torch.zeros_like(G["x_rec"]), x_lig=torch.zeros(0, 3), lig_ptr=torch.zeros(B + 1, dtype=torch.int32),
                 ctx=torch.zeros(0, dtype=torch.bool))
        drawn = _launch(Z, "ligand", 1.0, keys=keys, base=base)[0]
        assert torch.equal(drawn.view(torch.int32), eps.view(torch.int32))
        model = N.protein_draw_model(cn.keys, G["rec_ptr"].numpy(), base)
        err = float(np.abs(drawn.cpu().numpy().astype(np.float64) - model).max())
        worst = max(worst, err)
        assert err <= _normal_bound(), (name, err)
        # sigma == 0 reads no key and is the tape entry without eps
        a, b = _launch(G, "whole", 0.0, keys=keys, base=base), _launch(G, "whole", 0.0)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    print(f"base {base}: max |drawn normal - numpy model| = {worst:.3e} (bound {_normal_bound():.3e})")
    # the other base, another iteration: other normals
    G = graphs["b1_513"]
    k1, k2 = _keys_dev(N.training_noise(SEED, [5], 3).keys), _keys_dev(N.training_noise(SEED, [5], 4).keys)
    a, b, c = _launch(G, "protein", SIGMA, keys=k1, base=0), _launch(G, "protein", SIGMA, keys=k2, base=0), _launch(
        G, "protein", SIGMA, keys=k1, base=N.PURPOSE_STRIDE)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[0], c[0])


# ---- through apply_plan ----------------------------------------------------------------------------------------------------------------
LIG_SIZES = (9, 17, 12, 30, 5, 48)
T20 = 20


def _job(num_classes=13, n=6, rec=(40, 61), seed=11):
    """examples with context atoms (every third ligand atom), pockets of 40 - 60 atoms"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = LIG_SIZES[i % len(LIG_SIZES)]
        pos, feat, aa = synthetic.make_pocket(rng, int(rng.integers(*rec)), radius=6.0)
        out.append({"protein_pos": pos, "protein_atom_feature": feat, "protein_aa_type": aa,
                    "ligand_pos": (rng.standard_normal((m, 3)) * 1.5 + 1.0).astype(np.float32),
                    "ligand_atom_type": rng.integers(0, num_classes, size=m).astype(np.int64),
                    "ligand_gen_flag": np.arange(m) % 3 != 1})
    return out


def _split(out, batch):
    res = {}
    for g, ex in enumerate(batch["example_index"].tolist()):
        res[ex] = {"protein_pos": out["protein_pos"][batch["protein_element_batch"] == g],
                   "ligand_pos": out["ligand_pos"][batch["ligand_element_batch"] == g], "translation": out["translation"][g]}
        if "xt" in out:
            res[ex]["xt"] = out["xt"][batch["ligand_element_batch"] == g]
    return res


RUNS = {"one batch": [[0, 1, 2, 3, 4, 5]], "reversed": [[5, 4, 3, 2, 1, 0]], "alone": [[i] for i in range(6)], "2 + 4": [[0, 1], [2, 3, 4, 5]]}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("noise_mode", ["counter", "torch"])
def test_transformed_examples_do_not_depend_on_placement(noise_mode, mode):
    """six examples as one batch, reversed, each alone and split 2 + 4: protein_pos, ligand_pos and translation of every example are
    torch.equal -- in counter mode by construction of the addresses, in torch mode with each example's eps replayed.  In counter mode
    (context centring) the xt of a TargetDiff training call on the transformed batches is torch.equal too."""
    cs = train_cli.ComplexSet(_job())
    plan = TrainingPlan(0.1, mode)
    model = None
    if noise_mode == "counter" and mode == "context":
        model = C.get_model(C.default_targetdiff_config(13, num_layers=2, num_diffusion_timesteps=T20))
        model.load_state_dict(W.synthetic_state_dict(13, 2, seed=0, num_timesteps=T20), strict=True)
        model = model.to(DEV).train()
    g = torch.Generator().manual_seed(4)
    eps_of = [torch.randn(int(cs.rec_ptr[i + 1] - cs.rec_ptr[i]), 3, generator=g) for i in range(6)]
    got = {}
    for tag, batches in RUNS.items():
        got[tag] = {}
        for ids in batches:
            batch = cs.collate(ids, DEV, example_ids=True, ptrs=True)
            if noise_mode == "counter":
                cn = N.training_noise(SEED, batch["example_index"], 3)
                out = train_cli.apply_plan(batch, plan, noise=cn)
                if model is not None:
                    out = dict(out, xt=model(out, noise=cn)[1]["xt"].detach())
            else:
                out = train_cli.apply_plan(batch, plan, eps=torch.cat([eps_of[i] for i in ids]).to(DEV))
            assert out is not batch and out["translation"].shape == (len(ids), 3)
            got[tag].update(_split(out, batch))
    ref = got["one batch"]
    for tag in ("reversed", "alone", "2 + 4"):
        for e in range(6):
            for k, v in ref[e].items():
                assert v.shape == got[tag][e][k].shape and torch.equal(v, got[tag][e][k]), (noise_mode, mode, tag, e, k)
    # against the tensor restatement on the CPU (torch mode: the same eps), at the kernel test's bound
    if noise_mode == "torch":
        batch = cs.collate([0, 1, 2, 3, 4, 5], example_ids=True, ptrs=True)
        cpu = _split(train_cli.apply_plan(batch, plan, eps=torch.cat(eps_of)), batch)
        for e in range(6):
            # both sides are within 16 roundings of the exact result, relative to the largest (noised) input coordinate of the example
            one = cs.collate([e])
            M = float(max(one["protein_pos"].abs().max(), one["ligand_pos"].abs().max()) + 0.1 * eps_of[e].abs().max())
            bound = 2 * 16 * 2.0 ** -24 * M
            for k in ("protein_pos", "ligand_pos", "translation"):
                assert float((ref[e][k].cpu() - cpu[e][k]).abs().max()) <= bound, (mode, e, k)
    else:
        # iteration 4: other protein noise, same ligand frame only where the centre does not see the protein
        batch = cs.collate([0, 1, 2, 3, 4, 5], DEV, example_ids=True, ptrs=True)
        other = _split(train_cli.apply_plan(batch, plan, noise=N.training_noise(SEED, batch["example_index"], 4)), batch)
        assert all(not torch.equal(other[e]["protein_pos"], ref[e]["protein_pos"]) for e in range(6))
        if mode in ("context", "ligand"):
            assert all(torch.equal(other[e]["ligand_pos"], ref[e]["ligand_pos"]) for e in range(6))
    # without the CSRs in the batch apply_plan rebuilds them: same result
    batch = cs.collate([0, 1, 2, 3, 4, 5], DEV, example_ids=True)
    batch.pop("ligand_ptr")
    if noise_mode == "counter":
        again = train_cli.apply_plan(batch, plan, noise=N.training_noise(SEED, batch["example_index"], 3))
    else:
        again = train_cli.apply_plan(batch, plan, eps=torch.cat(eps_of).to(DEV))
    again = _split(again, batch)
    assert all(torch.equal(again[e][k], ref[e][k]) for e in range(6) for k in ("protein_pos", "ligand_pos", "translation"))


def test_apply_plan_draws_from_the_torch_generator_only_with_noise():
    cs = train_cli.ComplexSet(_job())
    batch = cs.collate([0, 1, 2], DEV, ptrs=True)
    torch.manual_seed(5)
    state = torch.cuda.get_rng_state(DEV)
    train_cli.apply_plan(batch, TrainingPlan(0.0, "context"))
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    torch.manual_seed(5)
    a = train_cli.apply_plan(batch, TrainingPlan(0.1, "context"))
    torch.manual_seed(5)
    eps = torch.randn(batch["protein_pos"].shape[0], 3, device=DEV)
    b = train_cli.apply_plan(batch, TrainingPlan(0.1, "context"), eps=eps)
    assert torch.equal(a["protein_pos"], b["protein_pos"]) and not torch.equal(a["protein_pos"], batch["protein_pos"])


# ---- the driver: resume ------------------------------------------------------------------------------------------------------------------
def test_run_resume_sees_the_same_transformed_batches(tmp_path):
    """two-layer T = 20 TargetDiff, add_pos_noise + context centring (tests/fixtures/linker_targetdiff_train_tiny.yml), --noise counter:
    two runs of 2 iterations and one run of 1 iteration + resume hand the model bit-equal batches at iteration 2 (training and
    validation), recorded through a forward pre-hook."""
    config, _ = C.load_config(os.path.join(ROOT, "tests", "fixtures", "linker_targetdiff_train_tiny.yml"))
    C.set_num_atom_type(config)
    cx = _job(config.model.num_atomtype, n=10, seed=3)
    tr, va = train_cli.ComplexSet(cx[:8]), train_cli.ComplexSet(cx[8:])
    records = []

    def hook(module, args):
        if type(module).__name__ == "TargetDiff" and args and isinstance(args[0], dict) and "protein_pos" in args[0]:
            b = args[0]
            records.append((module.training, {k: b[k].clone() if torch.is_tensor(b[k]) else np.array(b[k]) for k in
                                              ("protein_pos", "ligand_pos", "translation", "example_index")}))

    handle = torch.nn.modules.module.register_module_forward_pre_hook(hook)
    try:
        def go(tag, max_iters, resume=None):
            del records[:]
            cfg, _ = C.load_config(os.path.join(ROOT, "tests", "fixtures", "linker_targetdiff_train_tiny.yml"))
            C.set_num_atom_type(cfg)
            out = train_cli.run(cfg, tag, tr, va, DEV, str(tmp_path), max_iters=max_iters, resume=resume, noise="counter",
                                log=lambda s: None)
            return list(records), out
        a1, _ = go("a1", 2)
        a2, _ = go("a2", 2)
        _, first = go("b", 1)
        ckpt = os.path.join(first["ckpt_dir"], "1.pt")
        assert os.path.exists(ckpt)
        b, _ = go("b2", 2, resume=ckpt)          # resumes AT iteration 1 (train.py:175): iterations 1 and 2
    finally:
        handle.remove()

    def at_iteration_2(rec):
        train = [r for training, r in rec if training]
        val = [r for training, r in rec if not training]
        assert len(train) == 2 and len(val) == 2           # val_freq 1, one validation batch
        return train[1], val[1]

    ref_t, ref_v = at_iteration_2(a1)
    for other in (a2, b):
        t, v = at_iteration_2(other)
        for x, y in ((ref_t, t), (ref_v, v)):
            assert np.array_equal(x["example_index"], y["example_index"])
            for k in ("protein_pos", "ligand_pos", "translation"):
                assert torch.equal(x[k], y[k]), k
    # and the transforms ran: context centring, training noised afresh per iteration, validation not noised
    t1, t2 = [r for training, r in a1 if training]
    assert float(ref_t["translation"].abs().max()) > 1e-2
    shared = sorted(set(t1["example_index"].tolist()) & set(t2["example_index"].tolist()))
    stored = va.collate([0, 1], DEV)
    assert float((ref_v["protein_pos"] + ref_v["translation"][stored["protein_element_batch"]] - stored["protein_pos"]).abs().max()) < 1e-5
    stored = tr.collate(ref_t["example_index"].tolist(), DEV)
    resid = ref_t["protein_pos"] + ref_t["translation"][stored["protein_element_batch"]] - stored["protein_pos"]
    assert 0.08 < float(resid.std()) < 0.12, (float(resid.std()), shared)


# ---- identity ------------------------------------------------------------------------------------------------------------------------
def _profiled(fn):
    lib = _native.lib()
    n = len(_native.PROFILE_CLASSES)
    ms, cnt = (ctypes.c_double * n)(), (ctypes.c_int * n)()
    assert lib.cbgx_profile_begin(4096) == 0
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        assert lib.cbgx_profile_end(ms, cnt, n) == 0
    return out, list(cnt)


def test_identity_plan_launches_nothing():
    """the plan (0, 'protein'): apply_plan hands back the batch object itself -- there is no output a launch could have written -- and a
    model call behind it shows, under cbgx_profile_begin / cbgx_profile_end, the launches of a call on the plain batch, not one more"""
    cs = train_cli.ComplexSet(_job())
    model = C.get_model(C.default_targetdiff_config(13, num_layers=2, num_diffusion_timesteps=T20))
    model.load_state_dict(W.synthetic_state_dict(13, 2, seed=0, num_timesteps=T20), strict=True)
    model = model.to(DEV).train()
    batch = cs.collate([0, 1, 2], DEV, example_ids=True)
    cn = N.training_noise(SEED, batch["example_index"], 1)
    model(batch, noise=cn)          # warm-up: weight packing, workspaces
    (_, plain), plain_cnt = _profiled(lambda: model(batch, noise=cn))
    state = torch.cuda.get_rng_state(DEV)

    def through_plan():
        b = train_cli.apply_plan(batch, TrainingPlan.from_config(C.Config({}), "train"), noise=cn)
        assert b is batch and "translation" not in b
        return model(b, noise=cn)
    (_, planned), plan_cnt = _profiled(through_plan)
    assert plan_cnt == plain_cnt and sum(plain_cnt) > 0, (plain_cnt, plan_cnt)
    assert torch.equal(planned["xt"], plain["xt"]) and torch.equal(torch.cuda.get_rng_state(DEV), state)
    (out, alone_cnt) = _profiled(lambda: train_cli.apply_plan(batch, TrainingPlan(), noise=cn))
    assert out is batch and sum(alone_cnt) == 0


# ---- timing (printed, not asserted) ------------------------------------------------------------------------------------------------------
def _vectorised(batch, plan, eps, ctx):
    """the transform in a handful of batched tensor operations (index_add_ sums: an order that depends on the batch) -- the tensor
    program a GPU user would write, for the timing only"""
    rb, lb, B = batch["protein_element_batch"], batch["ligand_element_batch"], batch["num_graphs"]
    xr = batch["protein_pos"] + eps * plan.noise_std
    xl = batch["ligand_pos"]
    w = ctx.to(xl.dtype)[:, None]
    s = torch.zeros(B, 3, device=xr.device).index_add_(0, lb, xl * w)
    n = torch.zeros(B, 1, device=xr.device).index_add_(0, lb, w)
    c = s / n.clamp(min=1.0)
    return xr - c[rb], xl - c[lb], c


def test_timing_of_the_launch_and_the_tensor_restatement():
    """the 32-graph training shape (pockets of 350 - 650 atoms, ligands of 10 - 45), plan (0.1, 'context'): HIP-event time per call of the
    one launch (tape and counter entry, through apply_plan), of the graph-by-graph tensor restatement and of a batched tensor program"""
    cx = train_cli.synthetic_complexes(32, 2022, 13)
    for c in cx:
        c["ligand_gen_flag"] = np.arange(c["ligand_pos"].shape[0]) % 3 != 1
    cs = train_cli.ComplexSet(cx)
    batch = cs.collate(list(range(32)), DEV, example_ids=True, ptrs=True)
    plan = TrainingPlan(0.1, "context")
    eps = torch.randn(batch["protein_pos"].shape[0], 3, device=DEV)
    cn = N.training_noise(SEED, batch["example_index"], 1)
    ctx = ~batch["ligand_gen_flag"]

    def timed(fn, reps):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / reps
    us = {"apply_plan, tape entry (eps given)": timed(lambda: train_cli.apply_plan(batch, plan, eps=eps), 50),
          "apply_plan, counter entry": timed(lambda: train_cli.apply_plan(batch, plan, noise=cn), 50),
          "batched tensor program": timed(lambda: _vectorised(batch, plan, eps, ctx), 50),
          "tensor restatement (graph by graph)": timed(lambda: train_cli.apply_plan_tensors(batch, plan, eps), 5)}
    for k, v in us.items():
        print(f"train transform, 32 graphs, {batch['protein_pos'].shape[0]} protein atoms: {k}: {v:.1f} us per call")
    out = train_cli.apply_plan(batch, plan, eps=eps)
    vr, vl, vc = _vectorised(batch, plan, eps, ctx)
    assert float((out["protein_pos"] - vr).abs().max()) < 1e-4 and float((out["translation"] - vc).abs().max()) < 1e-4
