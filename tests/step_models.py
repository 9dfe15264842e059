"""TEST INFRASTRUCTURE ONLY -- cases and references for the step kernels of csrc/step.hip in isolation (no denoiser in the loop).

Case builders: seeded, CPU tensors only, shared by tests/test_step_models.py (CPU) and tests/test_gpu_step_kernels.py (GPU), so
both sides see the same numbers.  References: thin wrappers that evaluate the oracle's own functions (oracle/targetdiff.py,
oracle/diffbp.py, oracle/diffsbdd.py, pinned bit-exactly to the reference by tests/test_oracle_golden.py) in a given dtype on a
case.  What is restated here, and pinned against the oracle by the CPU tests: the body of ``type_backward`` (it has to return the
perturbed scores besides the decision) and DiffBP's three-line pre-amble of ``com_head``.

Layout of every case: the composed rows of a graph are contiguous (DiffSBDD's graph_ptr), inside a graph the ligand atoms sit on a
random subset of the rows in random order -- ``lig_rows`` is injective, not monotone, and ligand rows interleave with pocket rows;
``gen`` marks two atoms of three, context atoms in between; ligand arrays are sorted by graph.  Denoiser outputs are NaN on every
row a kernel has no business reading."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import diffbp as OB
from oracle import diffsbdd as OS
from oracle import targetdiff as OT

H = 128                       # feature width of the composed h rows
CONTEST_FACTOR = 16           # a decision is contested below this multiple of the fp32 model's largest score error on the case
CONTEST_CAP = 0.01            # contested rows: at most this share of the generated rows of a case
U_MAX = 1.0 - 2.0 ** -24      # the largest uniform the generators produce
NAN = float("nan")


# ---- layout ---------------------------------------------------------------------------------------------------------------------
def composed_layout(lig_sizes, pocket_sizes, g):
    graph_ptr, lig_rows, flags = [0], [], []
    for nl, npk in zip(lig_sizes, pocket_sizes):
        n = nl + npk
        perm = torch.randperm(n, generator=g)
        flag = torch.zeros(n, dtype=torch.bool)
        flag[perm[:nl]] = True
        lig_rows.append(perm[:nl] + graph_ptr[-1])
        flags.append(flag)
        graph_ptr.append(graph_ptr[-1] + n)
    B = len(lig_sizes)
    lig_flag = torch.cat(flags)
    batch_idx = torch.repeat_interleave(torch.arange(B), torch.tensor([a + b for a, b in zip(lig_sizes, pocket_sizes)]))
    lig_rows = torch.cat(lig_rows)
    n_lig = int(lig_rows.shape[0])
    return dict(B=B, N=graph_ptr[-1], n_lig=n_lig, lig_sizes=list(lig_sizes), pocket_sizes=list(pocket_sizes),
                graph_ptr=torch.tensor(graph_ptr, dtype=torch.int32), lig_rows=lig_rows.to(torch.int32),
                lig_ptr=torch.tensor(np.concatenate([[0], np.cumsum(lig_sizes)]), dtype=torch.int32),
                lig_flag=lig_flag.to(torch.uint8), rec_rows=torch.nonzero(~lig_flag).flatten(),
                bl=torch.repeat_interleave(torch.arange(B), torch.tensor(list(lig_sizes))), br=batch_idx[~lig_flag],
                gen=(torch.arange(n_lig) % 3 != 1).to(torch.uint8))


def _on_rows(n, cols, rows, values):
    out = torch.full((n, cols), NAN, dtype=torch.float32)
    out[rows] = values
    return out


def _embedder(C, g):
    """ligand_atom_emb / ligand_indicator parameters, in the order the entry points take them"""
    return [torch.randn(H, C, generator=g), torch.randn(H, generator=g), torch.randn(H, 1, generator=g), torch.randn(H, generator=g)]


def ligand_features(emb, c, dtype):
    """h of the ligand rows through the oracle's context_embed (an empty pocket stands in for the protein side)"""
    sd = {"e.ligand_atom_emb.weight": emb[0], "e.ligand_atom_emb.bias": emb[1], "e.ligand_indicator.weight": emb[2],
          "e.ligand_indicator.bias": emb[3], "e.protein_atom_emb.weight": torch.zeros(H, 1), "e.protein_atom_emb.bias": torch.zeros(H),
          "e.residue_emb.weight": torch.zeros(H, 20), "e.residue_emb.bias": torch.zeros(H)}
    sd = {k: v.to(dtype) for k, v in sd.items()}
    return OT.context_embed(sd, c.to(dtype), torch.zeros(0, 1, dtype=dtype), torch.zeros(0, 20, dtype=dtype), prefix="e")[0]


def onehot_features(emb, v):
    """h of a ligand row whose type vector is an exact one-hot: the kernels' fmaf chain adds exact zeros around one weight, so
    the row is ((w[:, v] + emb_b) + (ind_w[:, 0] + ind_b)) in fp32, bit for bit"""
    return (emb[0][:, v.long()].t() + emb[1]) + (emb[2][:, 0] + emb[3])


# ---- TargetDiff -----------------------------------------------------------------------------------------------------------------
TD_T = 1000
TD_C = (1, 3, 4, 5, 8, 13, 32)
TD_STEPS = (0, 1, 500, 999)
TD_SCALES = (3.0, 150.0)
TD_NLIG = (1, 255, 256, 257)
TD_HAND = (13, 500)           # (C, t) of the case that carries the hand-built rows


@functools.lru_cache(maxsize=None)
def targetdiff_tables(T=TD_T):
    """the shipped config's schedules (positions: sigmoid 1e-7 .. 2e-3, types: cosine s = 0.01)"""
    pos = OT.vp_tables(OT.vp_betas(T, 1.0e-7, 2.0e-3, "sigmoid"))
    typ = OT.type_tables(OT.vp_betas(T, 0.0, 0.0, "cosine", cosine_s=0.01))
    return pos, typ


def targetdiff_kernel_tables(T=TD_T):
    """the seven tables of include/cbgx.h, in its order"""
    pos, typ = targetdiff_tables(T)
    return [pos["posterior_mean_c0_coef"], pos["posterior_mean_ct_coef"], pos["posterior_logvar"], typ["log_alphas_v"],
            typ["log_one_minus_alphas_v"], typ["log_alphas_cumprod_v"], typ["log_one_minus_alphas_cumprod_v"]]


def targetdiff_grid():
    """28 of the 224 grid points: every (C, t), (C, n_lig), (C, scale), (t, n_lig), (t, scale) and (n_lig, scale) pair occurs
    (tests/test_step_models.py checks that)"""
    out = []
    for ci, C in enumerate(TD_C):
        for ti, t in enumerate(TD_STEPS):
            out.append((C, t, TD_SCALES[(ci // 2 + ti + (ci + ti) // 4) % 2], TD_NLIG[(ci + ti) % 4]))
    return out


def targetdiff_case(C, t, scale, n_lig, hand=None):
    """random rows; with ``hand`` the last eight rows are hand-built, in pairs (gen = 1, gen = 0):
      u = 0 in every class | u = 1 - 2^-24 in every class | classes 2 and 5 tied at the top (bit-equal logits, both c entries 0,
      equal u = 1 - 2^-24 against u = 0 elsewhere, which outweighs the pull of the current type 0: 2 must win) | flat logits and
      equal u, so the current type, the only class whose log(c + 1e-8) is not -18.4, wins"""
    hand = (C, t) == TD_HAND if hand is None else hand
    g = torch.Generator().manual_seed(1000 * C + t + int(scale) + 7 * n_lig)
    half = n_lig // 2
    lay = composed_layout([half, 0, n_lig - half], [5, 3, 40], g)
    rows = lay["lig_rows"].long()
    d = dict(lay, kind="targetdiff", C=C, t=t, T=TD_T, scale=scale, name=f"targetdiff C={C} t={t} scale={scale:g} n_lig={n_lig}")
    logits = scale * torch.randn(n_lig, C, generator=g)
    v = torch.randint(0, C, (n_lig,), generator=g)
    u = torch.rand(n_lig, C, generator=g)
    gen = lay["gen"].clone()
    d["tie_rows"], d["current_rows"] = {}, []
    if hand:
        assert C >= 6 and n_lig >= 8
        r = n_lig - 8
        gen[r:] = torch.tensor([1, 0] * 4, dtype=torch.uint8)
        u[r:r + 2] = 0.0
        u[r + 2:r + 4] = U_MAX
        for k in (r + 4, r + 5):
            logits[k, 2] = logits[k, 5] = logits[k].abs().max() + 9.0
            v[k] = 0
            u[k] = 0.0
            u[k, 2] = u[k, 5] = U_MAX
            d["tie_rows"][k] = 2
        for k in (r + 6, r + 7):
            logits[k] = 0.0
            u[k] = 0.5
            v[k] = 4
            d["current_rows"].append(k)
    d["gen"] = gen
    d["x_den"] = _on_rows(lay["N"], 3, rows, 2.0 * torch.randn(n_lig, 3, generator=g))
    d["logits"] = _on_rows(lay["N"], C, rows, logits)
    d["x_lig"] = 2.0 * torch.randn(n_lig, 3, generator=g)
    d["c_lig"] = F.one_hot(v, C).float()
    d["eps"] = torch.randn(n_lig, 3, generator=g)
    d["u"] = u
    d["emb"] = _embedder(C, g)
    return d


def targetdiff_cases():
    return [targetdiff_case(*p) for p in targetdiff_grid()]


def targetdiff_type_scores(tb, num_classes, c_pred_logits, ct, t, batch_idx, gen_flag, u):
    """oracle.targetdiff.type_backward, line for line, returning the perturbed scores gumbel + logp as well (the contested-row
    rule needs them).  tests/test_step_models.py asserts that its v_next is type_backward's on every case and both dtypes."""
    log_c_pred = F.log_softmax(c_pred_logits, dim=-1)
    log_ct = torch.log(ct + 1e-8)
    tm1 = torch.where(t - 1 < 0, torch.zeros_like(t), t - 1)
    lc = math.log(num_classes)
    a = tb["log_alphas_cumprod_v"][tm1][batch_idx].unsqueeze(-1)
    b = tb["log_one_minus_alphas_cumprod_v"][tm1][batch_idx].unsqueeze(-1)
    log_qvt1_v0 = OT.log_add_exp(log_c_pred + a, b - lc)
    a1 = tb["log_alphas_v"][t][batch_idx].unsqueeze(-1)
    b1 = tb["log_one_minus_alphas_v"][t][batch_idx].unsqueeze(-1)
    log_qvs1_vt = OT.log_add_exp(log_ct + a1, b1 - lc)
    un = log_qvt1_v0 + log_qvs1_vt
    logp = un - torch.logsumexp(un, dim=-1, keepdim=True)
    gumbel = -torch.log(-torch.log(u + 1e-30) + 1e-30)
    score = gumbel + logp
    v_next = torch.where(gen_flag, score.argmax(dim=-1), ct.argmax(-1))
    return F.one_hot(v_next, num_classes).to(ct.dtype), v_next, score


def _cast(tb, dtype):
    return {k: v.to(dtype) for k, v in tb.items()}


def targetdiff_reference(d, dtype):
    pos, typ = (_cast(tb, dtype) for tb in targetdiff_tables(d["T"]))
    rows, bl, gen = d["lig_rows"].long(), d["bl"], d["gen"].bool()
    t = torch.full((d["B"],), d["t"], dtype=torch.long)
    x_next = OT.pos_backward_denoise(pos, d["x_den"][rows].to(dtype), d["x_lig"].to(dtype), t, bl, gen, d["eps"].to(dtype))
    c_next, v_next, score = targetdiff_type_scores(typ, d["C"], d["logits"][rows].to(dtype), d["c_lig"].to(dtype), t, bl, gen,
                                                   d["u"].to(dtype))
    return dict(x_next=x_next, c_next=c_next, v_next=v_next, score=score)


# ---- the contested-row rule -----------------------------------------------------------------------------------------------------
def contested_rows(score32, score64, decided, skip=()):
    """``decided``: the rows whose outcome is the argmax of the scores.  A row is contested when the fp64 gap between its best and
    second-best score is below CONTEST_FACTOR x the fp32 model's largest score error against fp64 on those rows.  ``skip``: rows
    with an exact tie built in, decided by the first-index rule instead.  -> (bool mask over all rows, the score error)"""
    mask = decided.clone()
    for k in skip:
        mask[k] = False
    if not bool(mask.any()) or score64.shape[1] < 2:
        return torch.zeros_like(mask), 0.0
    err = float((score32.double() - score64)[mask].abs().max())
    top = score64.topk(2, dim=-1).values
    return ((top[:, 0] - top[:, 1]) < CONTEST_FACTOR * err) & mask, err


def contested_share(contested, decided):
    return float(contested.sum()) / max(int(decided.sum()), 1)


# ---- DiffBP ---------------------------------------------------------------------------------------------------------------------
SIZES_A = (0, 1, 63, 64, 65, 128, 129, 200, 0, 7)      # empty first graph, one in the middle; 63 / 64 / 65 and 128 / 129: the wave trips
SIZES_B = (5, 70, 0)                                   # the LAST graph is empty
BP_C = (2, 13, 14, 32)
BP_STEPS = ((1000, 0), (1000, 1), (1000, 999), (4, 0), (4, 1), (4, 2), (4, 3))     # (T, t); (4, 2): prob = 0.5 in every precision
U_MARGIN = 1e-6
U_BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0.0)))


def _pockets(sizes, g, empty=None):
    p = torch.randint(3, 41, (len(sizes),), generator=g).tolist()
    if empty is not None:
        p[empty] = 0
    return p


@functools.lru_cache(maxsize=None)
def diffbp_tables(T):
    return OT.vp_tables(OT.vp_betas(T, 1.0e-7, 2.0e-3, "sigmoid"))


def diffbp_case(C, absorbing, T, t, sizes=SIZES_A):
    """current types: the absorbing state on about half of the rows, generated and context; every 11th row is in the absorbing
    state and has its two largest logits bit-equal (the lower class must win); some generated rows carry a type vector with two
    entries of 1, the absorbing state and another class (the reference's argmax takes the first).  u: uniform, then
      * T = 4, t = 2 (prob = 0.5 exactly): rows 0 mod 4 get u = 0.5 (must NOT change), rows 1 mod 4 u = nextafter(0.5, 0) (must);
      * otherwise u is kept at least U_MARGIN = 1e-6 away from prob = (T - t) / T, so the outcome of `u < prob` does not hang on how
        a precision rounds the quotient (the dyadic case is the one that sits on the boundary, exactly)."""
    g = torch.Generator().manual_seed(100000 + 1000 * C + 100 * absorbing + 10 * T + t + len(sizes))
    lay = composed_layout(sizes, _pockets(sizes, g), g)
    n, N, rows = lay["n_lig"], lay["N"], lay["lig_rows"].long()
    d = dict(lay, kind="diffbp", C=C, T=T, t=t, absorbing=absorbing,
             name=f"diffbp C={C} absorbing={absorbing} T={T} t={t} graphs={len(sizes)}")
    x_in = 5.0 * torch.randn(n, 3, generator=g)
    d["x_in"] = _on_rows(N, 3, rows, x_in)
    d["x_den"] = _on_rows(N, 3, rows, x_in + torch.randn(n, 3, generator=g))
    d["x_com"] = _on_rows(N, 3, rows, x_in + 0.3 * torch.randn(n, 3, generator=g))
    logits = 3.0 * torch.randn(n, C, generator=g)
    d["tie_rows"] = {}
    for k in range(0, n, 11):
        j = torch.randperm(C, generator=g)[:2].tolist()
        logits[k, j[0]] = logits[k, j[1]] = logits[k].max() + 1.0
        d["tie_rows"][k] = min(j)
    d["logits"] = _on_rows(N, C, rows, logits)
    v = torch.where(torch.rand(n, generator=g) < 0.5, torch.full((n,), absorbing), torch.randint(0, C, (n,), generator=g))
    v[list(d["tie_rows"])] = absorbing
    d["x_lig"] = 3.0 * torch.randn(n, 3, generator=g)
    d["c_lig"] = F.one_hot(v, C).float()
    d["double_rows"] = [k for k in range(5, n, 13) if k % 3 != 1]      # generated rows only: a context row keeps its bits
    for k in d["double_rows"]:                                         # the absorbing state and another class, both 1
        d["c_lig"][k] = 0.0
        d["c_lig"][k, absorbing] = d["c_lig"][k, (absorbing + 1 + k % (C - 1)) % C] = 1.0
    d["eps"] = torch.randn(n, 3, generator=g)
    u = torch.rand(n, generator=g)
    prob = float(np.float32(T - t) / np.float32(T))
    u[2::8] = prob / 2                                  # both outcomes occur at every step, also where prob is 0.001 or 0.999
    u[3::8] = min((1.0 + prob) / 2, U_MAX)
    if (T, t) == (4, 2):
        assert prob == 0.5
        u[0::4] = 0.5
        u[1::4] = U_BELOW_HALF
    else:
        u = torch.where((u - prob).abs() < U_MARGIN, torch.full_like(u, prob - 2 * U_MARGIN), u)
    u[list(d["tie_rows"])[0::2]] = prob / 2             # every other tie row takes the argmax (where it is generated)
    d["u"], d["prob"] = u, prob
    return d


def diffbp_cases(C, absorbing):
    """every step on the ten-graph batch, the dyadic step and the last step on the batch whose last graph is empty"""
    return [diffbp_case(C, absorbing, T, t) for T, t in BP_STEPS] + \
           [diffbp_case(C, absorbing, 4, 2, SIZES_B), diffbp_case(C, absorbing, 1000, 999, SIZES_B)]


def diffbp_reference(d, dtype):
    """pre-amble of oracle.diffbp.com_head (noise = (x_den - x_in)[lig] minus its per-graph mean, shift = per-graph mean of
    (x_com - x_in)[lig]), then the oracle's score step and mask step"""
    rows, bl, B, gen = d["lig_rows"].long(), d["bl"], d["B"], d["gen"].bool()
    x_in = d["x_in"][rows].to(dtype)
    noise = d["x_den"][rows].to(dtype) - x_in
    noise = noise - OB.scatter_mean(noise, bl, B)[bl]
    shift = OB.scatter_mean(d["x_com"][rows].to(dtype) - x_in, bl, B)[bl]
    t = torch.full((B,), d["t"], dtype=torch.long)
    x_next = OB.pos_backward_score(_cast(diffbp_tables(d["T"]), dtype), noise + shift, d["x_lig"].to(dtype), t, bl, gen, d["eps"].to(dtype))
    lg = d["logits"][rows].to(dtype)
    c_next, v_next = OB.type_backward_mask(d["T"], d["C"], lg, d["c_lig"].to(dtype), t, bl, gen, d["u"], absorbing_state=d["absorbing"])
    return dict(x_next=x_next, c_next=c_next, v_next=v_next, score=lg)


def diffbp_decided(d):
    """rows that take the argmax of the logits"""
    return (d["u"] < d["prob"]) & d["gen"].bool() & (d["c_lig"].argmax(-1) == d["absorbing"])


# ---- DiffSBDD -------------------------------------------------------------------------------------------------------------------
SB_T = 1000
SB_STEPS = (0, 1, SB_T - 1)
FRAME0 = (30.0, -20.0, 5.0)


@functools.lru_cache(maxsize=None)
def diffsbdd_step_tables(T):
    """DiffSBDD.step_tables() of a default-config model (one layer: the tables depend on the scheduler alone)"""
    import cbgbench_amd as C
    torch.manual_seed(0)
    return C.get_model(C.default_diffsbdd_config(8, num_layers=1, num_diffusion_timesteps=T)).eval().step_tables()


def diffsbdd_coefficients(T, dtype):
    """the three per-step coefficients through the expressions of oracle.diffsbdd.sample_p_zs_given_zt: one atom per step k,
    mu(z = 1, eps = 0) = 1 / alpha_ts, -mu(z = 0, eps = 1) = sigma2_ts / alpha_ts / sigma_t, and the draw of (z = 0, eps_pred = 0,
    eps = 1) = sigma_ts sigma_s / sigma_t"""
    gam = OS.polynomial_gamma(T).to(dtype)
    k = torch.arange(T)
    s, t = k.to(dtype) / T, (k.to(dtype) + 1) / T
    one, zero = torch.ones(T, 1, dtype=dtype), torch.zeros(T, 1, dtype=dtype)
    f = lambda z, e_pred, e: OS.sample_p_zs_given_zt(gam, T, s, t, z, None, k, k, T, e_pred, e, False)[0].flatten()
    return f(one, zero, zero), -f(zero, one, zero), f(zero, zero, one)


def diffsbdd_case(C, t_idx, sizes, framed, do_x, do_c):
    g = torch.Generator().manual_seed(200000 + 1000 * C + t_idx + 17 * len(sizes) + 4 * framed + 2 * do_x + do_c)
    lay = composed_layout(sizes, _pockets(sizes, g, empty=1), g)        # graph 1 has no pocket atom
    n, N, B, rows, rec = lay["n_lig"], lay["N"], lay["B"], lay["lig_rows"].long(), lay["rec_rows"]
    d = dict(lay, kind="diffsbdd", C=C, T=SB_T, t_idx=t_idx, framed=framed, do_x=do_x, do_c=do_c,
             name=f"diffsbdd C={C} t={t_idx} graphs={len(sizes)} {'framed' if framed else 'unframed'} x={do_x} c={do_c}")
    d["coef"] = tuple(tab[t_idx] for tab in diffsbdd_step_tables(SB_T))
    # frame_shift on entry: the sum of the means removed so far; the composed x and the denoiser's x_den live in that frame
    S0 = (torch.tensor(FRAME0) + torch.randn(B, 3, generator=g)) if framed else torch.zeros(B, 3)
    d["frame0"] = S0 if framed else None
    x = torch.full((N, 3), NAN)
    x[rec] = 8.0 * torch.randn(rec.shape[0], 3, generator=g) + S0[lay["br"]]
    d["x"] = x
    d["x_den"] = _on_rows(N, 3, rows, torch.randn(n, 3, generator=g) + S0[lay["bl"]])
    d["logits"] = _on_rows(N, C, rows, torch.randn(n, C, generator=g))
    d["x_lig"] = 2.0 * torch.randn(n, 3, generator=g)
    d["c_lig"] = torch.randn(n, C, generator=g)
    d["eps_x"] = torch.randn(n, 3, generator=g)
    d["eps_c"] = torch.randn(n, C, generator=g)
    d["emb"] = _embedder(C, g)
    return d


def diffsbdd_cases(framed, t_idx):
    """C = 8: both batches x the four update_positions / update_types combinations; C = 5 once per (mode, step)"""
    out = [diffsbdd_case(8, t_idx, sizes, framed, do_x, do_c) for sizes in (SIZES_A, SIZES_B) for do_x in (1, 0) for do_c in (1, 0)]
    return out + [diffsbdd_case(5, t_idx, SIZES_B, framed, 1, 1)]


def diffsbdd_reference(d, dtype):
    """sample_p_zs_given_zt from the scheduler's gamma table: positions with com=True (and once with com=False for the removed
    mean), types with com=False.  In the framed mode the inputs are taken out of the frame first (true = frame - frame_shift)."""
    T, B, bl, br = d["T"], d["B"], d["bl"], d["br"]
    rows, rec = d["lig_rows"].long(), d["rec_rows"]
    gam = OS.polynomial_gamma(T).to(dtype)
    s = torch.full((B,), d["t_idx"], dtype=dtype) / T
    t = (torch.full((B,), d["t_idx"], dtype=dtype) + 1) / T
    S0 = d["frame0"].to(dtype) if d["framed"] else torch.zeros(B, 3, dtype=dtype)
    x_pred = d["x_den"][rows].to(dtype) - S0[bl]
    x_rec = d["x"][rec].to(dtype) - S0[br]
    x_lig, c_lig = d["x_lig"].to(dtype), d["c_lig"].to(dtype)
    if d["do_x"]:
        args = (gam, T, s, t, x_lig, x_rec, bl, br, B, x_pred, d["eps_x"].to(dtype))
        shift = OS.scatter_mean(OS.sample_p_zs_given_zt(*args, False)[0], bl, B)
        x_next, x_rec_next = OS.sample_p_zs_given_zt(*args, True)
    else:
        shift, x_next, x_rec_next = torch.zeros(B, 3, dtype=dtype), x_lig, x_rec
    if d["do_c"]:
        c_next = OS.sample_p_zs_given_zt(gam, T, s, t, c_lig, None, bl, br, B, d["logits"][rows].to(dtype), d["eps_c"].to(dtype), False)[0]
    else:
        c_next = c_lig
    return dict(x_next=x_next, c_next=c_next, shift=shift, frame=S0 + shift, x_rec=x_rec_next, h=ligand_features(d["emb"], c_next, dtype))
