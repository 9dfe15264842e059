"""The decomposition choice in the batch-transform launch on the GPU (csrc/train_transform.hip: cbgx_train_transform_choose,
cbgx_train_transform_choose_rng; ``train_cli.apply_plan(choose=...)``): both entries against "flag built on the host, then the entry
without the choice" bit for bit at every size where a stride, a barrier or a fallback can go wrong, the drawn choice against
``noise.choose_model``, an index outside the ligand, placement invariance, the three model classes, the driver with resume, and the cost
of the launch (printed)."""
import os
import re

import numpy as np
import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import _native, noise as N, synthetic, train_cli
from cbgbench_amd.priors import ContextChoice, TrainingPlan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SEED = 2022
MODES = ("protein", "context", "ligand", "whole")
SIGMA = float(np.float32(0.1))
GUARD = 2                             # untouched rows in front of and behind every output
UNWRITTEN = -7777                     # fill of choice_out: 0xFF bytes would read as -1, the value a graph without decompositions gets


def _unsorted(n, seed):
    """indices of an n-atom ligand in no order, some twice"""
    r = np.random.default_rng(seed)
    half = r.permutation(n)[:max(n // 2, 1)]
    return np.concatenate([half, half[::3], half[:1]]).tolist()


# (protein atoms, ligand atoms, decompositions).  Ligands of 0, 1, 2, 255, 256, 257 and 600 atoms (one, two and three strides of the 256
# threads, and the sizes around them), pockets of 1, 768 and 769 atoms (768: the atoms a thread holds in registers), K = 0, 1, 2 and 7;
# decompositions that are empty, full, a prefix, interleaved, unsorted with duplicates
SPEC = [
    (1, 0, [[]]),
    (768, 1, [[0], []]),
    (769, 2, []),
    (1, 255, [[], list(range(255)), list(range(100)), list(range(0, 255, 2)), _unsorted(255, 1), [254], list(range(1, 255, 3))]),
    (768, 256, [list(range(256)), list(range(1, 256, 2))]),
    (769, 257, [_unsorted(257, 2)]),
    (40, 600, [list(range(300)), list(range(0, 600, 2)), [], list(range(600)), _unsorted(600, 3) + [599], [0, 599], list(range(256, 600))]),
]
KS = [len(s[2]) for s in SPEC]
CHOICES = [[t % k if k else 0 for k in KS] for t in range(7)]          # every decomposition of every graph is picked once


def _batch(spec, seed=0):
    g = torch.Generator().manual_seed(seed)
    rec_n, lig_n = [s[0] for s in spec], [s[1] for s in spec]
    ptr = lambda n: torch.tensor([0] + list(np.cumsum(n)), dtype=torch.int32)
    decs = [d for s in spec for d in s[2]]
    return {"x_rec": torch.randn(sum(rec_n), 3, generator=g) * 8.0 + torch.tensor([20.0, -13.0, 5.0]),
            "x_lig": torch.randn(sum(lig_n), 3, generator=g) * 2.0 + torch.tensor([21.0, -12.0, 4.0]),
            "rec_ptr": ptr(rec_n), "lig_ptr": ptr(lig_n), "eps": torch.randn(sum(rec_n), 3, generator=g), "B": len(spec),
            "dec_ptr": ptr([len(s[2]) for s in spec]), "gen_ptr": ptr([len(d) for d in decs]),
            "gen_idx": torch.tensor([a for d in decs for a in d], dtype=torch.int32), "spec": spec}


def _host_flag(G, choice):
    """ChooseCtxGen's gen_flag of every graph for the picks ``choice`` (-1: no decomposition, everything generated), on the host; an
    index outside the ligand is skipped"""
    out = []
    for (nr, nl, decs), k in zip(G["spec"], choice):
        f = np.zeros(nl, dtype=bool) if k >= 0 else np.ones(nl, dtype=bool)
        if k >= 0:
            for a in decs[k]:
                if 0 <= a < nl:
                    f[a] = True
        out.append(f)
    return torch.from_numpy(np.concatenate(out))


def _guarded(n, cols=3):
    buf = torch.full((n + 2 * GUARD, cols), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _dev(G):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in G.items()}


def _launch_choose(G, mode, sigma, choice=None, eps=None, keys=None, base=0):
    """one launch of a choose entry on poisoned outputs with guards; returns (x_rec_out, x_lig_out, center_out, gen_flag_out, choice_out)
    after checking that every guard is intact and every element written"""
    d = _dev(G)
    n_rec, n_lig, B = d["x_rec"].shape[0], d["x_lig"].shape[0], d["B"]
    n_dec, n_idx = d["gen_ptr"].shape[0] - 1, d["gen_idx"].shape[0]
    (rb, ro), (lb, lo), (cb, co) = _guarded(n_rec), _guarded(n_lig), _guarded(B)
    fb = torch.full((n_lig + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    kb = torch.full((B + 2 * GUARD,), UNWRITTEN, dtype=torch.int32, device=DEV)
    fo, ko = fb[GUARD:GUARD + n_lig], kb[GUARD:GUARD + B]
    head = (_native.ptr(d["x_rec"]), _native.ptr(d["x_lig"]), _native.ptr(d["rec_ptr"]), _native.ptr(d["lig_ptr"]), _native.ptr(d["dec_ptr"]),
            _native.ptr(d["gen_ptr"]), _native.ptr(d["gen_idx"]))
    sizes = (B, n_rec, n_lig, n_dec, n_idx, sigma, MODES.index(mode))
    tail = (_native.ptr(ro), _native.ptr(lo), _native.ptr(co), _native.ptr(fo), _native.ptr(ko), _native.current_stream(DEV))
    if keys is not None:
        _native.check(_native.lib().cbgx_train_transform_choose_rng(*head, *sizes, _native.ptr(keys), base, *tail),
                      "cbgx_train_transform_choose_rng")
    else:
        ch = torch.tensor(choice, dtype=torch.int32, device=DEV) if choice is not None else None
        eps = eps.to(DEV).contiguous() if eps is not None else None
        _native.check(_native.lib().cbgx_train_transform_choose(*head, _native.ptr(ch), *sizes, _native.ptr(eps), *tail),
                      "cbgx_train_transform_choose")
    torch.cuda.synchronize()
    for buf, n in ((rb, n_rec), (lb, n_lig), (cb, B)):
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), "a guard row was written"
        assert torch.isfinite(buf[GUARD:GUARD + n]).all(), "an output element was not written"
    assert bool((fb[:GUARD] == 0xFF).all()) and bool((fb[GUARD + n_lig:] == 0xFF).all()), "a guard byte of gen_flag_out was written"
    assert bool((kb[:GUARD] == UNWRITTEN).all()) and bool((kb[GUARD + B:] == UNWRITTEN).all()), "a guard of choice_out was written"
    assert bool((fo <= 1).all()) and bool((ko != UNWRITTEN).all()), "a flag or a choice was not written"
    return ro.clone(), lo.clone(), co.clone(), fo.clone(), ko.clone()


def _launch_plain(G, mode, sigma, ctx, eps=None, keys=None, base=0):
    """cbgx_train_transform / cbgx_train_transform_rng with the context flag ``ctx`` [n_lig] bool"""
    d = _dev(G)
    n_rec, n_lig, B = d["x_rec"].shape[0], d["x_lig"].shape[0], d["B"]
    ro, lo, co = torch.empty(n_rec, 3, device=DEV), torch.empty(n_lig, 3, device=DEV), torch.empty(B, 3, device=DEV)
    cx = ctx.to(DEV).contiguous().view(torch.uint8)
    head = (_native.ptr(d["x_rec"]), _native.ptr(d["x_lig"]), _native.ptr(d["rec_ptr"]), _native.ptr(d["lig_ptr"]), _native.ptr(cx), B,
            n_rec, n_lig, sigma, MODES.index(mode))
    tail = (_native.ptr(ro), _native.ptr(lo), _native.ptr(co), _native.current_stream(DEV))
    if keys is not None:
        _native.check(_native.lib().cbgx_train_transform_rng(*head, _native.ptr(keys), base, *tail), "cbgx_train_transform_rng")
    else:
        eps = eps.to(DEV).contiguous() if eps is not None else None
        _native.check(_native.lib().cbgx_train_transform(*head, _native.ptr(eps), *tail), "cbgx_train_transform")
    torch.cuda.synchronize()
    return ro, lo, co


def _bits(t):
    return t.view(torch.int32)


@pytest.fixture(scope="module")
def G():
    return _batch(SPEC)


@pytest.mark.parametrize("sigma", [0.0, SIGMA])
@pytest.mark.parametrize("mode", MODES)
def test_tape_entry_equals_host_flag_plus_the_plain_entry(G, mode, sigma):
    """seven choice vectors that pick every decomposition of every graph once: x_rec_out, x_lig_out and center_out are the bits of
    cbgx_train_transform given the host-built flag; gen_flag_out is that flag; choice_out is the input, -1 for the graph without
    decompositions"""
    eps = G["eps"] if sigma > 0 else None
    for choice in CHOICES:
        want_k = [k if K else -1 for k, K in zip(choice, KS)]
        flag = _host_flag(G, want_k)
        got = _launch_choose(G, mode, sigma, choice=choice, eps=eps)
        ref = _launch_plain(G, mode, sigma, ~flag, eps=eps)
        for x, y, what in zip(got[:3], ref, ("x_rec_out", "x_lig_out", "center_out")):
            assert torch.equal(_bits(x), _bits(y)), (mode, sigma, choice, what)
        assert torch.equal(got[3].cpu().bool(), flag), (mode, choice)
        assert got[4].tolist() == want_k
    # choice_in NULL is decomposition 0; a choice outside [0, K) is clamped into it
    a, b = _launch_choose(G, mode, sigma, choice=None, eps=eps), _launch_choose(G, mode, sigma, choice=CHOICES[0], eps=eps)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = _launch_choose(G, mode, sigma, choice=[50, -3, 9, 7, -1, 1, 100], eps=eps)
    assert c[4].tolist() == [0, 0, -1, 6, 0, 0, 6]
    if mode == "context":
        # graph 3 with its full decomposition has no context atom: its ligand's mean is the centre, as for 'ligand'
        full = _launch_choose(G, "context", 0.0, choice=CHOICES[1])
        lig = _launch_choose(G, "ligand", 0.0, choice=CHOICES[1])
        assert bool(full[3][int(G["lig_ptr"][3]):int(G["lig_ptr"][4])].all()) and torch.equal(full[2][3], lig[2][3])
        # graph 2 has no decomposition: everything generated, the same fallback
        assert bool(full[3][int(G["lig_ptr"][2]):int(G["lig_ptr"][3])].all()) and torch.equal(full[2][2], lig[2][2])


def _keys_dev(keys):
    return torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).to(DEV)


@pytest.mark.parametrize("base", [0, N.PURPOSE_STRIDE])
def test_counter_entry_draws_the_model_choice_and_the_plain_entry_bits(G, base):
    """three sets of keys per base: choice_out equals noise.choose_model; gen_flag_out is the host flag of that choice; everything else is
    bit-equal to cbgx_train_transform_rng given that flag, in every mode and with and without noise"""
    picked = set()
    for visit in (1, 2, 3):
        ex = 100 * visit + np.arange(G["B"])
        cn = N.training_noise(SEED, ex, visit) if base == 0 else N.validation_noise(SEED, ex)
        assert cn.purpose_base == base
        keys = _keys_dev(cn.keys)
        want_k = N.choose_model(cn.keys, np.array(KS), base).tolist()
        flag = _host_flag(G, want_k)
        for mode in MODES:
            for sigma in (0.0, SIGMA):
                got = _launch_choose(G, mode, sigma, keys=keys, base=base)
                assert got[4].tolist() == want_k, (base, visit, mode)
                assert torch.equal(got[3].cpu().bool(), flag)
                ref = _launch_plain(G, mode, sigma, ~flag, keys=keys, base=base)
                for x, y, what in zip(got[:3], ref, ("x_rec_out", "x_lig_out", "center_out")):
                    assert torch.equal(_bits(x), _bits(y)), (base, visit, mode, sigma, what)
        picked.add(tuple(want_k))
    assert len(picked) > 1 and all(k[2] == -1 and k[0] == 0 for k in picked)
    # the other base draws at another address
    other = N.choose_model(cn.keys, np.array(KS), N.PURPOSE_STRIDE - base).tolist()
    assert _launch_choose(G, "context", 0.0, keys=keys, base=N.PURPOSE_STRIDE - base)[4].tolist() == other


def test_an_index_outside_the_ligand_is_ignored():
    """straight to the entry (``ComplexSet`` refuses such lists): indices beyond the graph's ligand -- inside the next graph's rows, far
    outside the array, negative -- set nothing; the other graphs' rows and the guards stay as they are"""
    spec = [(5, 4, [[0, 2]]), (6, 3, [[1, 3, 4, 7, 2 ** 30, -1, -5, 2], [0]]), (4, 5, [[4, 0]])]
    G = _batch(spec, seed=5)
    clean = _batch([(5, 4, [[0, 2]]), (6, 3, [[1, 2], [0]]), (4, 5, [[4, 0]])], seed=5)
    for mode in MODES:
        a = _launch_choose(G, mode, SIGMA, choice=[0, 0, 0], eps=G["eps"])
        b = _launch_choose(clean, mode, SIGMA, choice=[0, 0, 0], eps=G["eps"])
        assert a[3].tolist() == [1, 0, 1, 0] + [0, 1, 1] + [1, 0, 0, 0, 1]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), mode


# ---- through apply_plan ----------------------------------------------------------------------------------------------------------------
LIG_SIZES = (9, 17, 12, 30, 5, 48)


def _job(num_classes=13, n=6, seed=11, K=3, rec=(40, 61)):
    """examples with K decompositions each (none with K = 0)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = LIG_SIZES[i % len(LIG_SIZES)]
        pos, feat, aa = synthetic.make_pocket(rng, int(rng.integers(*rec)), radius=6.0)
        out.append({"protein_pos": pos, "protein_atom_feature": feat, "protein_aa_type": aa,
                    "ligand_pos": (rng.standard_normal((m, 3)) * 1.5 + 1.0).astype(np.float32),
                    "ligand_atom_type": rng.integers(0, num_classes, size=m).astype(np.int64)})
        if K:
            out[-1]["ligand_gen_index"] = synthetic.decompositions(rng, m, K)
        else:
            out[-1]["ligand_gen_flag"] = np.arange(m) % 3 != 1
    return out


KEYS = ("decomposition", "ligand_gen_flag", "protein_pos", "ligand_pos", "translation")


def _example(out, g):
    return {"decomposition": out["decomposition"][g], "translation": out["translation"][g],
            "ligand_gen_flag": out["ligand_gen_flag"][out["ligand_element_batch"] == g],
            "ligand_pos": out["ligand_pos"][out["ligand_element_batch"] == g],
            "protein_pos": out["protein_pos"][out["protein_element_batch"] == g]}


@pytest.mark.parametrize("mode", ["context", "whole"])
def test_chosen_examples_do_not_depend_on_placement(mode):
    """counter mode, K = 3: an example alone in its batch, first of six and last of six gets the same decomposition, flag, coordinates and
    translation, bit for bit; its decomposition is the model's; another iteration picks afresh"""
    cx = _job()
    cs = train_cli.ComplexSet(cx)
    plan, choose = TrainingPlan(0.1, mode), ContextChoice("uniform")

    def run(ids, it=3):
        batch = cs.collate(ids, DEV, example_ids=True, ptrs=True, decomps=True)
        out = train_cli.apply_plan(batch, plan, noise=N.training_noise(SEED, batch["example_index"], it), choose=choose)
        assert out["decomposition"].dtype == torch.int32 and out["ligand_gen_flag"].dtype == torch.bool
        return out
    for e in range(6):
        others = [i for i in range(6) if i != e]
        alone, first, last = _example(run([e]), 0), _example(run([e] + others), 0), _example(run(others + [e]), 5)
        for k in KEYS:
            assert torch.equal(alone[k], first[k]) and torch.equal(alone[k], last[k]), (mode, e, k)
        k = int(N.choose_model(N.training_noise(SEED, [e], 3).keys, 3)[0])
        assert int(alone["decomposition"]) == k
        assert alone["ligand_gen_flag"].nonzero().flatten().tolist() == cx[e]["ligand_gen_index"][k].tolist()
    picks = {it: run(list(range(6)), it)["decomposition"].tolist() for it in range(1, 9)}
    assert len({tuple(v) for v in picks.values()}) > 1
    for it, v in picks.items():
        assert v == N.choose_model(N.training_noise(SEED, np.arange(6), it).keys, 3).tolist()
    # a replay, fix_zero and the torch generator take the tape entry; in counter mode their protein noise is still the counter's
    batch = cs.collate(list(range(6)), DEV, example_ids=True, ptrs=True, decomps=True)
    cn = N.training_noise(SEED, batch["example_index"], 3)
    drawn = train_cli.apply_plan(batch, plan, noise=cn, choose=choose)
    replay = train_cli.apply_plan(batch, plan, noise=cn, choose=choose, choice=drawn["decomposition"])
    assert all(torch.equal(drawn[k], replay[k]) for k in KEYS)
    zero = train_cli.apply_plan(batch, plan, noise=cn, choose=ContextChoice("fix_zero"))
    assert zero["decomposition"].tolist() == [0] * 6
    plain = train_cli.apply_plan(cs.collate(list(range(6)), DEV, example_ids=True, ptrs=True), plan, noise=cn)      # the stored flag: decomposition 0
    assert all(torch.equal(zero[k], plain[k]) for k in KEYS[1:])
    torch.manual_seed(3)
    state = torch.cuda.get_rng_state(DEV)
    mine = train_cli.apply_plan(batch, TrainingPlan(0.0, mode), choose=choose)
    torch.cuda.set_rng_state(state, DEV)
    u = torch.rand(6, dtype=torch.float64, device=DEV)
    assert mine["decomposition"].tolist() == torch.clamp((u * 3).floor().long(), max=2).tolist()
    # the identity plan: the flag with tensor operations, the kernel's bits of the choice, the coordinates untouched
    ident = train_cli.apply_plan(batch, TrainingPlan(), noise=cn, choose=choose)
    assert torch.equal(ident["decomposition"], drawn["decomposition"]) and torch.equal(ident["ligand_gen_flag"], drawn["ligand_gen_flag"])
    assert ident["protein_pos"] is batch["protein_pos"] and "translation" not in ident


def _one_atom_job(num_classes):
    """the examples of ``_job`` with decompositions of ONE generated atom each (three different atoms per ligand)"""
    cx = _job(num_classes)
    for c in cx:
        m = c["ligand_pos"].shape[0]
        c["ligand_gen_index"] = [np.array([(3 * j + 1) % m]) for j in range(3)]
    return cx


@pytest.mark.parametrize("kind", ["one generated atom", "several generated atoms"])
@pytest.mark.parametrize("name", ["targetdiff", "diffbp", "diffsbdd"])
def test_models_read_the_chosen_flag_like_a_stored_one(name, kind):
    """one counter-noise training call on a chosen batch, at three iterations with different picks, against the call on a batch whose
    complexes were stored with that flag as a plain ``ligand_gen_flag``: the transformed inputs and the noising-derived results
    (t, xt, vt, masks, x0, v0 ...) are bit-equal, and so are the losses -- with one exception.  TargetDiff's fused loss
    (csrc/train_loss.hip) adds the per-atom terms of a graph with float atomics in LDS, in an order that differs from call to call: two
    identical calls on a batch with several generated atoms per graph do not always return the same bits (measured on one MI355X, 40
    identical calls: 'atom' took 2 bit patterns, every loss of DiffBP and DiffSBDD and every loss on the one-atom batch took 1).  A
    sum of one term has no order, so with ONE generated atom per graph the losses of all three classes must be bit-equal; with
    several, TargetDiff's are compared at the suite's tolerance for that loss (tests/test_gpu_train_counter_noise.py ``_loss_close``) and
    the other two classes' bit for bit."""
    from tests.test_gpu_train_counter_noise import NOISING, _classes, _loss_close, _model
    m = _model(name).train()
    cx = _one_atom_job(_classes(name)) if kind == "one generated atom" else _job(_classes(name))
    cs = train_cli.ComplexSet(cx)
    plan, choose = TrainingPlan(0.1, "context"), ContextChoice("uniform")
    exact = kind == "one generated atom" or name != "targetdiff"
    seen = []
    for it in (3, 4, 5):
        batch = cs.collate([0, 1, 2, 3, 4, 5], DEV, example_ids=True, ptrs=True, decomps=True)
        cn = N.training_noise(SEED, batch["example_index"], it)
        chosen = train_cli.apply_plan(batch, plan, noise=cn, choose=choose)
        ld, res = m(chosen, noise=cn)
        flag = chosen["ligand_gen_flag"].cpu()
        seen.append(tuple(chosen["decomposition"].tolist()))
        stored = []
        for g, c in enumerate(cx):
            c = {k: v for k, v in c.items() if k != "ligand_gen_index"}
            c["ligand_gen_flag"] = flag[batch["ligand_element_batch"].cpu() == g].numpy()
            stored.append(c)
        pb = train_cli.ComplexSet(stored).collate([0, 1, 2, 3, 4, 5], DEV, example_ids=True, ptrs=True)
        plain = train_cli.apply_plan(pb, plan, noise=cn)
        assert "decomposition" not in plain and all(torch.equal(plain[k], chosen[k]) for k in KEYS[1:])
        ld_p, res_p = m(plain, noise=cn)
        noising = [k for k in NOISING if k in res and torch.is_tensor(res[k])]
        assert noising and sorted(k for k in NOISING if k in res_p and torch.is_tensor(res_p[k])) == sorted(noising)
        for k in noising:
            assert torch.equal(res[k].detach(), res_p[k].detach()), (name, kind, it, k)
        assert sorted(ld) == sorted(ld_p)
        for k in ld:
            a, b = ld[k].detach(), ld_p[k].detach()
            same = torch.equal(a, b)
            print(f"{name}, {kind}, iteration {it}, loss({k}): {float(a):.9g} / {float(b):.9g} bit-equal {same}")
            assert same if exact else _loss_close(float(a), float(b)), (name, kind, it, k, float(a), float(b))
    assert len(set(seen)) > 1


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def test_run_logs_the_model_choices_and_resumes_them(tmp_path):
    """two-layer T = 20 TargetDiff on tests/fixtures/linker_targetdiff_train_tiny.yml (choose_ctx_gen, add_pos_noise, context centring),
    ten tiny complexes with K = 3, --noise counter: the logged decompositions of iterations 1..3 are noise.choose_model's; a run resumed at
    iteration 2 hands the model the batches of the uninterrupted run from there on (training and validation); a set without
    decompositions gets, under the same config, the batches of the entries without the choice."""
    fixture = os.path.join(ROOT, "tests", "fixtures", "linker_targetdiff_train_tiny.yml")
    config, _ = C.load_config(fixture)
    C.set_num_atom_type(config)
    cx = _job(config.model.num_atomtype, n=10, seed=3, rec=(20, 31))
    tr, va = train_cli.ComplexSet(cx[:8]), train_cli.ComplexSet(cx[8:])
    records, lines = [], []
    kept = ("protein_pos", "ligand_pos", "translation", "example_index", "ligand_gen_flag", "decomposition")

    def hook(module, args):
        if type(module).__name__ == "TargetDiff" and args and isinstance(args[0], dict) and "protein_pos" in args[0]:
            b = args[0]
            records.append((module.training, {k: b[k].clone() if torch.is_tensor(b[k]) else np.array(b[k]) for k in kept if k in b}))

    def go(tag, sets, max_iters, resume=None):
        del records[:], lines[:]
        cfg, _ = C.load_config(fixture)
        C.set_num_atom_type(cfg)
        out = train_cli.run(cfg, tag, sets[0], sets[1], DEV, str(tmp_path), max_iters=max_iters, resume=resume, noise="counter",
                            log=lines.append)
        return list(records), list(lines), out

    handle = torch.nn.modules.module.register_module_forward_pre_hook(hook)
    try:
        full, log_full, _ = go("a", (tr, va), 3)
        _, _, first = go("b", (tr, va), 2)
        ckpt = os.path.join(first["ckpt_dir"], "2.pt")
        if not os.path.exists(ckpt):          # (a checkpoint is written when validation improves; iteration 1's always is)
            ckpt = os.path.join(first["ckpt_dir"], "1.pt")
        start = int(os.path.basename(ckpt)[:-3])
        resumed, _, _ = go("b2", (tr, va), 3, resume=ckpt)
        plain_cx = [dict({k: v for k, v in c.items() if k != "ligand_gen_index"}, ligand_gen_flag=np.arange(c["ligand_pos"].shape[0]) % 3 != 1)
                    for c in cx]
        ptr, pva = train_cli.ComplexSet(plain_cx[:8]), train_cli.ComplexSet(plain_cx[8:])
        plain, log_plain, _ = go("c", (ptr, pva), 2)
    finally:
        handle.remove()
    assert any(s.startswith("[data]") and "ContextChoice(sampling='uniform')" in s for s in log_full)
    chosen = [s for s in log_full if s.startswith("[choose]")]
    assert len(chosen) == 3
    for it, line in enumerate(chosen, start=1):
        ex = [int(v) for v in re.search(r"examples \[([^\]]*)\]", line).group(1).split(",")]
        got = [int(v) for v in re.search(r"decomposition \[([^\]]*)\]", line).group(1).split(",")]
        assert f"iter {it:05d}" in line and got == N.choose_model(N.training_noise(SEED, ex, it).keys, 3).tolist()
    train_full = [r for training, r in full if training]
    assert len(train_full) == 3 and len({tuple(r["decomposition"].tolist()) for r in train_full}) > 1
    for r in train_full:
        for g, e in enumerate(r["example_index"].tolist()):
            sizes = [tr.lig_ptr[i + 1] - tr.lig_ptr[i] for i in r["example_index"].tolist()]
            l0 = int(sum(sizes[:g]))
            flag = r["ligand_gen_flag"][l0:l0 + int(sizes[g])]
            assert flag.nonzero().flatten().tolist() == cx[e]["ligand_gen_index"][int(r["decomposition"][g])].tolist()
    # validation: a function of (seed, example) -- the same picks at every iteration
    val_full = [r for training, r in full if not training]
    assert len(val_full) == 3              # val_freq 1, one validation batch
    want = N.choose_model(N.validation_noise(SEED, [0, 1]).keys, 3, N.PURPOSE_STRIDE).tolist()
    assert all(r["decomposition"].tolist() == want for r in val_full)
    # resume: from its first iteration on, the batches of the uninterrupted run
    def from_iteration(rec, first_it, it0):
        train = [r for training, r in rec if training]
        val = [r for training, r in rec if not training]
        return train[it0 - first_it:], val[it0 - first_it:]
    a_t, a_v = from_iteration(full, 1, start)
    b_t, b_v = from_iteration(resumed, start, start)
    assert len(a_t) == len(b_t) == 3 - start + 1 and len(a_v) == len(b_v)
    for x, y in list(zip(a_t, b_t)) + list(zip(a_v, b_v)):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(x[k], y[k]) if k == "example_index" else torch.equal(x[k], y[k]), k
    # a set without decompositions: no pick, and the batches of cbgx_train_transform_rng on the stored flag
    assert not any(s.startswith("[choose]") for s in log_plain) and not any("ContextChoice" in s for s in log_plain)
    plan_tr, plan_va = TrainingPlan(0.1, "context"), TrainingPlan(0.0, "context")
    seen_t = [r for training, r in plain if training]
    assert len(seen_t) == 2
    for it, r in enumerate(seen_t, start=1):
        assert "decomposition" not in r
        b = ptr.collate(r["example_index"].tolist(), DEV, example_ids=True, ptrs=True)
        want = train_cli.apply_plan(b, plan_tr, noise=N.training_noise(SEED, b["example_index"], it))
        assert all(torch.equal(r[k], want[k]) for k in ("protein_pos", "ligand_pos", "translation", "ligand_gen_flag"))
    for training, r in plain:
        if not training:
            want = train_cli.apply_plan(pva.collate([0, 1], DEV, example_ids=True, ptrs=True), plan_va)
            assert all(torch.equal(r[k], want[k]) for k in ("protein_pos", "ligand_pos", "translation", "ligand_gen_flag"))


# ---- cost (printed, not asserted) --------------------------------------------------------------------------------------------------------
def test_timing_of_the_launch_with_and_without_the_choice():
    """the 32-graph training shape (pockets of 350 - 650 atoms, ligands of 10 - 45, K = 3), plan (0.1, 'context'): HIP-event time per
    launch, 100 launches each, of cbgx_train_transform (given a flag) and cbgx_train_transform_choose (given the decompositions) on the
    same batch, and of the two counter entries"""
    cx = train_cli.synthetic_complexes(32, 2022, 13, decompositions=3)
    cs = train_cli.ComplexSet(cx)
    b = cs.collate(list(range(32)), DEV, example_ids=True, ptrs=True, decomps=True)
    n_rec, n_lig, B = b["protein_pos"].shape[0], b["ligand_pos"].shape[0], 32
    eps = torch.randn(n_rec, 3, device=DEV)
    keys = N.training_noise(SEED, b["example_index"], 1).device_keys(DEV)
    ctx = (~b["ligand_gen_flag"]).contiguous().view(torch.uint8)
    choice = torch.zeros(B, dtype=torch.int32, device=DEV)
    ro, lo, co = torch.empty(n_rec, 3, device=DEV), torch.empty(n_lig, 3, device=DEV), torch.empty(B, 3, device=DEV)
    fo, ko = torch.empty(n_lig, dtype=torch.uint8, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    lib, p, s = _native.lib(), _native.ptr, _native.current_stream(DEV)
    x = (p(b["protein_pos"]), p(b["ligand_pos"]), p(b["protein_ptr"]), p(b["ligand_ptr"]))
    dec = (p(b["ligand_dec_ptr"]), p(b["ligand_gen_ptr"]), p(b["ligand_gen_idx"]))
    n_dec, n_idx = b["ligand_gen_ptr"].shape[0] - 1, b["ligand_gen_idx"].shape[0]
    mode = MODES.index("context")
    calls = {
        "cbgx_train_transform": lambda: lib.cbgx_train_transform(*x, p(ctx), B, n_rec, n_lig, SIGMA, mode, p(eps), p(ro), p(lo), p(co), s),
        "cbgx_train_transform_choose": lambda: lib.cbgx_train_transform_choose(*x, *dec, p(choice), B, n_rec, n_lig, n_dec, n_idx, SIGMA,
                                                                               mode, p(eps), p(ro), p(lo), p(co), p(fo), p(ko), s),
        "cbgx_train_transform_rng": lambda: lib.cbgx_train_transform_rng(*x, p(ctx), B, n_rec, n_lig, SIGMA, mode, p(keys), 0, p(ro),
                                                                         p(lo), p(co), s),
        "cbgx_train_transform_choose_rng": lambda: lib.cbgx_train_transform_choose_rng(*x, *dec, B, n_rec, n_lig, n_dec, n_idx, SIGMA, mode,
                                                                                       p(keys), 0, p(ro), p(lo), p(co), p(fo), p(ko), s),
    }

    def timed(fn, reps=100):
        for _ in range(5):
            assert fn() == 0
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(e) / reps
    for rnd in range(2):          # twice, alternating: the second round is the one to read
        for name, fn in calls.items():
            print(f"round {rnd}: 32 graphs, {n_rec} protein atoms, {n_lig} ligand atoms, {n_dec} decompositions: {name}: {timed(fn):.2f} us per launch")
    assert calls["cbgx_train_transform_choose"]() == 0
    torch.cuda.synchronize()
    assert torch.equal(fo.bool(), b["ligand_gen_flag"])          # decomposition 0 is the collated flag
