"""Training driver: the role of the reference's ``train.py`` (config -> model / optimizer / scheduler -> the iteration loop
with periodic validation -- loss and the config's ``eval.metrics`` (the type-prediction AUROC, ``cbgbench_amd/evaluate.py``) -- and
best-so-far checkpoints, ``train.py:99-273``), minus the LMDB datasets and tensorboard (out of scope), made
data-parallel the way SURVEY.md 8e/8f-4 asks:

* one process per GPU (``python -m cbgbench_amd.launch --nproc N -m cbgbench_amd.train_cli ...``: FileStore rendezvous, no port to
  pass; ``torchrun`` works too), every rank holds a full replica;
* a rank-aware loader: one permutation of the training complexes per epoch, seeded identically everywhere, of which rank r
  takes the entries r, r+W, ... -- no sampler object, no collective;
* gradients of all ranks summed by ONE RCCL all-reduce of the flat fp32 gradient buffer per step (``train.FlatGradients``),
  averaged before clipping so that ``clip_grad_norm_`` sees the global gradient;
* validation loss and metrics all-reduced so that ``ReduceLROnPlateau`` takes the same decision on every rank; checkpoints written by
  rank 0 only, in the reference's format ``{'config', 'model', 'optimizer', 'scheduler', 'iteration', 'avg_val_loss'}``
  under ``{logdir}/{tag}/checkpoints/{it}.pt`` (``train.py:266-273``); ``--resume`` restores all of it on every rank
  (``train.py:160-175``; ``--finetune`` keeps only the weights).

    python -m cbgbench_amd.train_cli --config configs/denovo/train/targetdiff.yml --logdir logs
                                     [--data complexes.pt | --synthetic 256] [--resume ckpt.pt] [--max_iters N]
                                     [--noise {torch,counter}] [--ignore_data_transforms] [--synthetic_decompositions K]

Complex input: a ``torch.save``d list of dicts with ``protein_pos [n,3]``, ``protein_atom_feature [n,7]``,
``protein_aa_type [n]``, ``ligand_pos [m,3]``, ``ligand_atom_type [m]`` and optionally ``ligand_gen_flag [m]`` (what the
reference's featurizers produce) and ``ligand_gen_index`` -- a list of K >= 1 integer arrays, the ligand's decompositions into generated
and context atoms (the reference's ``data['ligand']['gen_index']``, molecule_parser.py:442-486); they are stored centred on the protein mean (``center_pos``, translation.py:5-25) and collated into
the ``MergeKeys`` + ``follow_batch`` schema.  Without ``--data``, synthetic complexes stand in.

Every batch then goes through the per-visit transforms of its split's transform list (``config.data.train.transform``,
``config.data.val.transform``; ``priors.TrainingPlan``), as the reference's dataset does at every ``__getitem__``: ``add_pos_noise`` --
fresh protein-coordinate noise at every visit of an example -- followed by the config's centring (``center_pos`` on the noised protein,
on the context atoms ``~ligand_gen_flag`` or on the ligand; ``center_whole_pos``), in ONE libcbgx launch per batch (``apply_plan``,
csrc/train_transform.hip), and the batch records the shift as ``translation``.  A list with neither entry, or a config without a ``data``
section, leaves the batches as collated (no launch, no draw); ``--ignore_data_transforms`` does so for any config.  With
``--noise counter`` the protein noise is a function of (seed, example, iteration, atom) like the rest of the step's noise; validation
without a ``data.val`` section is not noised and takes the train list's centring.

A list that starts with ``choose_ctx_gen`` (every context-task list; ``priors.ContextChoice``) on complexes that carry ``ligand_gen_index``
picks, at every visit of an example, one of its decompositions -- uniformly, or the first under ``sampling: fix_zero`` -- sets
``ligand_gen_flag`` on the atoms it names and centres on the complement, in the same launch (``cbgx_train_transform_choose``); the
batch records the picks as ``decomposition``.  With ``--noise counter`` the pick is a function of (seed, example, iteration), of
(seed, example) in validation.  Complexes without the key train on their one ``ligand_gen_flag``, as before; with the key and without
the transforms (``--ignore_data_transforms``) on decomposition 0.
"""
import argparse
import os
import time

import numpy as np
import torch

from . import get_model, load_config, set_num_atom_type, sharding, synthetic
from . import noise as _noise
from .config import checkpoint_config, load_checkpoint_file
from .evaluate import Evaluator
from .priors import ContextChoice, TrainingPlan
from .train import FlatGradients, broadcast_parameters, get_optimizer, get_scheduler, train_step, validate


# ---- data ------------------------------------------------------------------------------------------------------
class ComplexSet:
    """Protein-ligand complexes packed once (CSR on the host); ``collate(ids)`` builds a batch dict with index arithmetic."""

    def __init__(self, complexes, center=True):
        t = lambda a, dt: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dt)
        self.n = len(complexes)
        rec_n = [int(np.asarray(c["protein_pos"]).shape[0]) for c in complexes]
        lig_n = [int(np.asarray(c["ligand_pos"]).shape[0]) for c in complexes]
        self.rec_ptr = torch.tensor([0] + list(np.cumsum(rec_n)), dtype=torch.long)
        self.lig_ptr = torch.tensor([0] + list(np.cumsum(lig_n)), dtype=torch.long)
        ppos = [t(c["protein_pos"], torch.float32) for c in complexes]
        lpos = [t(c["ligand_pos"], torch.float32) for c in complexes]
        ctr = [p.mean(0) if center else torch.zeros(3) for p in ppos]
        self.protein_pos = torch.cat([p - m for p, m in zip(ppos, ctr)])
        self.ligand_pos = torch.cat([p - m for p, m in zip(lpos, ctr)])
        self.protein_atom_feature = torch.cat([t(c["protein_atom_feature"], torch.float32) for c in complexes])
        self.protein_aa_type = torch.cat([t(c["protein_aa_type"], torch.long) for c in complexes])
        self.ligand_atom_type = torch.cat([t(c["ligand_atom_type"], torch.long) for c in complexes])
        self.has_gen = all("ligand_gen_flag" in c for c in complexes)
        if self.has_gen:
            self.ligand_gen_flag = torch.cat([t(c["ligand_gen_flag"], torch.bool) for c in complexes])
        self._pack_decompositions(complexes, lig_n)

    def _pack_decompositions(self, complexes, lig_n):
        """``ligand_gen_index`` (the reference's ``data['ligand']['gen_index']``: K >= 1 arrays of ligand-local atom indices per complex)
        as three CSR levels: ``dec_ptr`` [n + 1] complex -> its decompositions, ``gen_ptr`` [D + 1] decomposition -> its atoms,
        ``gen_idx`` [total] int32.  An empty decomposition (all atoms context) and a full one (no context) are legal; an index outside
        [0, m), an empty list and a set in which only some complexes carry the key raise ``ValueError``.  A set with the key and without
        ``ligand_gen_flag`` gets the flag of decomposition 0 (what ``choose_ctx_gen, sampling: fix_zero`` would set)."""
        has = ["ligand_gen_index" in c for c in complexes]
        self.has_dec = bool(has) and all(has)
        if not self.has_dec:
            if any(has):
                missing = [i for i, h in enumerate(has) if not h]
                raise ValueError(f"ligand_gen_index: {len(missing)} of {len(has)} complexes do not carry it (first: complex {missing[0]})")
            return
        dec_n, gen_n, idx = [], [], []
        for i, (c, m) in enumerate(zip(complexes, lig_n)):
            decs = list(c["ligand_gen_index"])
            if not decs:
                raise ValueError(f"ligand_gen_index of complex {i} is an empty list: a complex needs at least one decomposition")
            for d, a in enumerate(decs):
                a = (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).reshape(-1)
                if a.size and not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"ligand_gen_index[{d}] of complex {i} must hold integers, not {a.dtype}")
                a = a.astype(np.int64)
                if a.size and (a.min() < 0 or a.max() >= m):
                    raise ValueError(f"ligand_gen_index[{d}] of complex {i} has an index outside [0, {m})")
                gen_n.append(a.size)
                idx.append(a)
            dec_n.append(len(decs))
        self.dec_ptr = torch.tensor([0] + list(np.cumsum(dec_n)), dtype=torch.long)
        self.gen_ptr = torch.tensor([0] + list(np.cumsum(gen_n)), dtype=torch.long)
        self.gen_idx = torch.from_numpy(np.concatenate(idx).astype(np.int32))
        if not self.has_gen:
            flag = torch.zeros(int(self.lig_ptr[-1]), dtype=torch.bool)
            first = self.dec_ptr[:-1]
            rows, seg = self._rows(self.gen_ptr, first)
            flag[self.lig_ptr[:-1][seg] + self.gen_idx[rows].long()] = True
            self.ligand_gen_flag, self.has_gen = flag, True

    def __len__(self):
        return self.n

    @staticmethod
    def _rows(ptr, ids):
        cnt = ptr[ids + 1] - ptr[ids]
        seg = torch.repeat_interleave(torch.arange(ids.numel()), cnt)
        start = torch.cumsum(cnt, 0) - cnt
        return ptr[ids][seg] + (torch.arange(int(cnt.sum())) - start[seg]), seg

    def collate(self, ids, device="cpu", example_ids=False, ptrs=False, decomps=False):
        """``example_ids=True`` (the counter noise mode): the batch also carries ``example_index`` -- ``ids`` as a host array, the
        global identity its noise is keyed by -- and ``ligand_ptr``, the [B + 1] int32 ligand CSR on ``device``.
        ``ptrs=True`` (a batch that ``apply_plan`` will transform): ``protein_ptr`` and ``ligand_ptr``, both CSRs, built on the host.
        ``decomps=True`` (a batch whose ``apply_plan`` gets a ``ContextChoice``), on a set with ``ligand_gen_index``: the decompositions
        of the batch's complexes as ``ligand_dec_ptr`` [B + 1], ``ligand_gen_ptr`` [D_b + 1] and ``ligand_gen_idx`` (ligand-local), all
        int32 on ``device``, the two CSRs rebased to the batch.  A set without the key collates what it collates without the option."""
        ids = torch.as_tensor(ids, dtype=torch.long)
        rr, rseg = self._rows(self.rec_ptr, ids)
        lr, lseg = self._rows(self.lig_ptr, ids)
        b = {
            "protein_pos": self.protein_pos[rr], "protein_atom_feature": self.protein_atom_feature[rr],
            "protein_aa_type": self.protein_aa_type[rr], "protein_lig_flag": torch.zeros(rr.numel(), dtype=torch.bool),
            "protein_element_batch": rseg,
            "ligand_pos": self.ligand_pos[lr], "ligand_atom_type": self.ligand_atom_type[lr],
            "ligand_lig_flag": torch.ones(lr.numel(), dtype=torch.bool), "ligand_element_batch": lseg,
        }
        if self.has_gen:
            b["ligand_gen_flag"] = self.ligand_gen_flag[lr]
        b = {k: v.to(device) for k, v in b.items()}
        b["num_graphs"] = int(ids.numel())       # known on the host: spares the model a device round trip per step
        b["max_ligand_atoms"] = int((self.lig_ptr[ids + 1] - self.lig_ptr[ids]).max())     # DiffBP's interior loss sizes a tile with it
        if example_ids:
            b["example_index"] = ids.numpy().copy()
            cnt = self.lig_ptr[ids + 1] - self.lig_ptr[ids]
            b["ligand_ptr"] = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)]).to(torch.int32).to(device)
        if ptrs:
            for name, ptr in (("protein_ptr", self.rec_ptr), ("ligand_ptr", self.lig_ptr)):
                if name not in b:
                    cnt = ptr[ids + 1] - ptr[ids]
                    b[name] = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)]).to(torch.int32).to(device)
        if decomps and self.has_dec:
            drows, _ = self._rows(self.dec_ptr, ids)              # the batch's decompositions, complex after complex
            irows, _ = self._rows(self.gen_ptr, drows)
            csr = lambda cnt: torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)]).to(torch.int32).to(device)
            b["ligand_dec_ptr"] = csr(self.dec_ptr[ids + 1] - self.dec_ptr[ids])
            b["ligand_gen_ptr"] = csr(self.gen_ptr[drows + 1] - self.gen_ptr[drows])
            b["ligand_gen_idx"] = self.gen_idx[irows].to(device)
        return b


def synthetic_complexes(n, seed, num_classes, n_rec_range=(350, 650), n_lig_range=(10, 45), decompositions=0):
    """stand-in data: synthetic pockets with a ligand blob near the centre (jittered lattice points).
    ``decompositions`` K > 0: every complex also gets K seeded decompositions (``ligand_gen_index``, ``synthetic.decompositions``), drawn
    from a generator of their own -- the complexes themselves are those of K = 0."""
    rng = np.random.default_rng(seed)
    rng_dec = np.random.default_rng([int(seed), 0x6465636F])
    out = []
    for _ in range(n):
        pos, feat, aa = synthetic.make_pocket(rng, int(rng.integers(n_rec_range[0], n_rec_range[1] + 1)))
        m = int(rng.integers(n_lig_range[0], n_lig_range[1] + 1))
        lig = (rng.standard_normal((m, 3)) * 2.0).astype(np.float32)
        out.append({"protein_pos": pos, "protein_atom_feature": feat, "protein_aa_type": aa, "ligand_pos": lig,
                    "ligand_atom_type": rng.integers(0, num_classes, size=m).astype(np.int64)})
        if decompositions > 0:
            out[-1]["ligand_gen_index"] = synthetic.decompositions(rng_dec, m, int(decompositions))
    return out


class ShardedLoader:
    """Rank-aware batches of item indices.  Every rank draws the same permutation of ``range(n_items)`` per epoch
    (``seed + epoch``) and keeps the entries ``rank, rank + world, ...``; the tail is padded by wrapping around so that all
    ranks make the same number of steps (a collective per step must not be left waiting)."""

    def __init__(self, n_items, batch_size, rank=0, world=1, seed=0, shuffle=True):
        if n_items < 1:
            raise ValueError("ShardedLoader: empty dataset")
        self.n, self.bs, self.rank, self.world, self.seed, self.shuffle = n_items, batch_size, rank, world, seed, shuffle
        self.per_rank = (n_items + world - 1) // world

    def epoch(self, e):
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + e)
            perm = torch.randperm(self.n, generator=g)
        else:
            perm = torch.arange(self.n)
        total = self.per_rank * self.world
        if total > self.n:                                   # wrap around (more than once when n_items < world / 2)
            perm = perm.repeat((total + self.n - 1) // self.n)[:total]
        mine = perm[self.rank::self.world]
        return [mine[i:i + self.bs].tolist() for i in range(0, mine.numel(), self.bs)]

    def __iter__(self):           # the reference's inf_iterator (repo/utils/train.py)
        e = 0
        while True:
            for ids in self.epoch(e):
                yield ids
            e += 1


class PositionedLoader:
    """The loader of the counter noise mode: the batch of iteration ``it`` (1-based) is a function of ``it`` -- not of how many times
    ``next()`` was called since the process started -- and the GLOBAL batch of an iteration is the same for every world size that
    divides it.  One permutation of ``range(n_items)`` per epoch (``seed + epoch``, as ShardedLoader), wrapped around to a whole number
    of global batches of ``batch_size * world`` items; iteration ``it`` is global batch ``(it - 1) % steps`` of epoch ``(it - 1) // steps``,
    of which rank r takes the entries r, r + W, ...  So a resumed run sees, from its first iteration on, the batches the uninterrupted
    run saw there, and world sizes 1, 2, 4 with batch sizes 8, 4, 2 train on the same examples at every iteration."""

    def __init__(self, n_items, batch_size, rank=0, world=1, seed=0, shuffle=True):
        if n_items < 1:
            raise ValueError("PositionedLoader: empty dataset")
        self.n, self.bs, self.rank, self.world, self.seed, self.shuffle = n_items, batch_size, rank, world, seed, shuffle
        self.global_bs = batch_size * world
        self.steps = (n_items + self.global_bs - 1) // self.global_bs
        self._epoch = (None, None)

    def _perm(self, e):
        if self._epoch[0] != e:
            perm = torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed + e)) if self.shuffle else torch.arange(self.n)
            total = self.steps * self.global_bs
            if total > self.n:
                perm = perm.repeat((total + self.n - 1) // self.n)[:total]
            self._epoch = (e, perm)
        return self._epoch[1]

    def position(self, it):
        """(epoch, step in the epoch) of iteration ``it`` >= 1"""
        return (it - 1) // self.steps, (it - 1) % self.steps

    def batch(self, it):
        """this rank's example indices at iteration ``it``"""
        e, k = self.position(it)
        return self._perm(e)[k * self.global_bs:(k + 1) * self.global_bs][self.rank::self.world].tolist()


# ---- the config's per-visit transforms ---------------------------------------------------------------------------------------------
CENTER_MODES = {"protein": 0, "context": 1, "ligand": 2, "whole": 3}      # include/cbgx.h CBGX_CENTER_*


def _csr(batch, ptr_key, batch_key, B, counts=False):
    """the [B + 1] int32 CSR of one side of the batch on its device: the batch's own (``collate(ptrs=True)``), else from the sorted
    ``*_element_batch`` ids.  ``counts=True``: the per-graph sizes as a host list instead."""
    ptr = batch.get(ptr_key, None)
    idx = batch[batch_key]
    if ptr is None:
        if idx.numel() and not bool((idx[1:] >= idx[:-1]).all()):
            raise ValueError(f"apply_plan needs {batch_key} sorted by graph")
        ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=idx.device), torch.bincount(idx, minlength=B).cumsum(0)]).to(torch.int32)
    if ptr.dtype != torch.int32 or ptr.shape[0] != B + 1 or ptr.device != idx.device:
        raise ValueError(f"{ptr_key} must be the [B + 1] int32 CSR on the batch's device (B = {B})")
    return (ptr[1:] - ptr[:-1]).tolist() if counts else ptr.contiguous()


def _context_flag(batch):
    """context atoms = ~ligand_gen_flag; a batch without the flag has none"""
    gen = batch.get("ligand_gen_flag", None)
    return None if gen is None else ~gen.to(torch.bool)


CHOOSE_LOGGED = 16        # graphs per reported iteration whose pick ``run`` logs
DECOMP_KEYS = ("ligand_dec_ptr", "ligand_gen_ptr", "ligand_gen_idx")      # ``collate(decomps=True)``


def _has_decompositions(batch, choose, choice=None):
    """does ``choose`` (a ``priors.ContextChoice`` or None) have something to choose from in this batch?"""
    has = choose is not None and batch.get("ligand_dec_ptr", None) is not None
    if has and any(batch.get(k, None) is None for k in DECOMP_KEYS):
        raise ValueError(f"a batch with decompositions carries {', '.join(DECOMP_KEYS)} (collate(decomps=True))")
    if choice is not None and not has:
        raise ValueError("choice= replays a decomposition choice: it needs choose= and a batch with decompositions")
    return has


def _pick_decompositions(batch, choose, choice, B):
    """k [B] int64 on the batch's device: the decomposition every graph trains on at this visit -- ``choice`` (a replay, clamped into
    [0, K)), zeros for 'fix_zero', else ``min(floor(u * K), K - 1)`` with ``u = torch.rand(B, dtype=float64)`` from the torch generator
    of the batch's device; -1 for a graph without decompositions.  The draw is made for every batch that carries decompositions, also
    when no graph of it has more than one: the counts live on the device, and asking would cost a synchronisation per batch."""
    dec_ptr = batch["ligand_dec_ptr"]
    dev = dec_ptr.device
    if dec_ptr.dtype != torch.int32 or dec_ptr.shape[0] != B + 1:
        raise ValueError(f"ligand_dec_ptr must be the [B + 1] int32 CSR of the batch's decompositions (B = {B})")
    K = (dec_ptr[1:] - dec_ptr[:-1]).long()
    if choice is not None:
        choice = torch.as_tensor(choice)
        if tuple(choice.shape) != (B,) or choice.dtype.is_floating_point:
            raise ValueError(f"choice must hold {B} integers")
        k = choice.to(device=dev, dtype=torch.long)
    elif choose.sampling == "fix_zero":
        k = torch.zeros(B, dtype=torch.long, device=dev)
    else:
        k = (torch.rand(B, dtype=torch.float64, device=dev) * K).floor().long()
    return torch.where(K > 0, torch.minimum(k.clamp(min=0), K - 1), torch.full_like(K, -1))


def _flag_of_decompositions(batch, k, B):
    """``ligand_gen_flag`` [n_lig] bool of the picks ``k`` (``_pick_decompositions``), with tensor operations: ChooseCtxGen's
    ``gen_flag[gen_index] = True`` for the whole batch; a graph without decompositions (k = -1) is generated entirely"""
    dec_ptr, gen_ptr, gen_idx = (batch[key].long() for key in DECOMP_KEYS)
    lig_ptr = _csr(batch, "ligand_ptr", "ligand_element_batch", B).long()
    lb = batch["ligand_element_batch"]
    flag = (k < 0)[lb]
    top = gen_ptr.numel() - 1                    # (a graph without decompositions may point at the end of gen_ptr)
    d0, d1 = (dec_ptr[:-1] + k.clamp(min=0)).clamp(max=top), (dec_ptr[:-1] + k.clamp(min=0) + 1).clamp(max=top)
    cnt = torch.where(k >= 0, gen_ptr[d1] - gen_ptr[d0], torch.zeros_like(k))
    seg = torch.repeat_interleave(torch.arange(B, device=k.device), cnt)
    start = torch.cumsum(cnt, 0) - cnt
    local = gen_idx[gen_ptr[d0][seg] + (torch.arange(int(cnt.sum()), device=k.device) - start[seg])]
    if local.numel() and bool(((local < 0) | (local >= (lig_ptr[1:] - lig_ptr[:-1])[seg])).any()):
        raise ValueError("ligand_gen_idx has an index outside its graph's ligand")
    flag[lig_ptr[:-1][seg] + local] = True
    return flag


def apply_plan_tensors(batch, plan, eps=None, choose=None, choice=None):
    """``apply_plan`` restated with tensor operations, graph by graph in the reference's own expressions (``AddPosNoise`` then
    ``CenterPos`` / ``CenterWholePos``, translation.py): ``pos + eps * noise_std``, then ``mean(dim=0)`` of the centre set --
    ``(ligand.sum(0) + protein.sum(0)) / n`` for 'whole'.  On one graph it gives the bits of the reference's classes.  It is what a CPU
    batch gets (stub models, gloo tests) and what the GPU tests compare the kernel with; an empty centre set gives the zero vector.
    ``choose`` / ``choice`` as in ``apply_plan``: on a batch with decompositions ``ligand_gen_flag`` is first replaced by the flag of the
    picked decompositions (``ChooseCtxGen``, select.py:21-58) and ``decomposition`` [B] int32 records the picks."""
    x_rec, x_lig = batch["protein_pos"], batch["ligand_pos"]
    B = int(batch["num_graphs"])
    if _has_decompositions(batch, choose, choice):
        k = _pick_decompositions(batch, choose, choice, B)
        batch = dict(batch, ligand_gen_flag=_flag_of_decompositions(batch, k, B), decomposition=k.to(torch.int32))
    rec_n = _csr(batch, "protein_ptr", "protein_element_batch", B, counts=True)
    lig_n = _csr(batch, "ligand_ptr", "ligand_element_batch", B, counts=True)
    ctx = _context_flag(batch)
    if plan.noise_std > 0:
        if eps is None:
            raise ValueError("apply_plan_tensors: a plan with noise needs eps")
        x_rec = x_rec + eps * plan.noise_std
    rec_out, lig_out, centers, r0, l0 = [], [], [], 0, 0
    for nr, nl in zip(rec_n, lig_n):
        P, L = x_rec[r0:r0 + nr], x_lig[l0:l0 + nl]
        zero = x_rec.new_zeros(3)
        if plan.center == "protein":
            c = P.mean(dim=0) if nr else zero
        elif plan.center == "whole":
            c = (L.sum(0) + P.sum(0)) / (nl + nr) if nl + nr else zero
        else:
            m = ctx[l0:l0 + nl] if plan.center == "context" and ctx is not None else None
            if m is not None and int(m.sum()) > 0:
                c = L[m].mean(dim=0)
            else:
                c = L.mean(dim=0) if nl else zero
        rec_out.append(P - c)
        lig_out.append(L - c)
        centers.append(c)
        r0, l0 = r0 + nr, l0 + nl
    out = dict(batch)
    out["protein_pos"] = torch.cat(rec_out) if rec_out else x_rec
    out["ligand_pos"] = torch.cat(lig_out) if lig_out else x_lig
    out["translation"] = torch.stack(centers) if centers else x_rec.new_zeros(0, 3)
    return out


def apply_plan(batch, plan, noise=None, eps=None, choose=None, choice=None):
    """The per-visit transforms of the config (``priors.TrainingPlan``) on a collated batch: protein noise, then the centring.  Returns the
    batch with ``protein_pos`` / ``ligand_pos`` replaced and ``translation`` [B, 3] added -- the shift relative to the stored frame
    (``ComplexSet``: the protein mean of the stored coordinates).  The identity plan ``(0, 'protein')`` returns ``batch`` itself: no
    launch, no draw.
    On a CUDA device: ONE libcbgx launch (csrc/train_transform.hip).  ``noise`` a ``CounterNoise`` (``noise.training_noise`` /
    ``validation_noise`` of the batch's examples) selects ``cbgx_train_transform_rng``: the normals are drawn in the kernel at the
    protein atoms' addresses (noise.py), so an example's transformed coordinates do not depend on its batch; the batch should carry
    ``protein_ptr`` / ``ligand_ptr`` (``collate(ptrs=True)``), else they are rebuilt from the batch ids.  Otherwise ``eps`` [n_rec, 3]
    -- the caller's (a replay), or ``torch.randn`` from the torch generator, drawn only when ``noise_std > 0`` -- goes to
    ``cbgx_train_transform``.  On a CPU device ``apply_plan_tensors`` runs instead; a ``CounterNoise`` there raises: its draws are made
    by GPU kernels.
    ``choose`` (a ``priors.ContextChoice``: the list's ``choose_ctx_gen``) on a batch with decompositions (``collate(decomps=True)``):
    every graph first picks one of its decompositions, ``ligand_gen_flag`` is replaced by the flag of the picked ones -- the context of
    the centring is its complement -- and ``decomposition`` [B] int32 records the picks, all in the same launch
    (``cbgx_train_transform_choose`` / ``_choose_rng``).  The pick: ``choice`` [B] (a replay, like ``eps``); with a ``CounterNoise`` and
    'uniform', drawn in the kernel at the graph's TRAIN_CHOOSE_CTX address (``noise.choose_model``); otherwise
    ``min(floor(u * K), K - 1)`` with ``u = torch.rand(B, dtype=float64)`` from the torch generator, drawn before ``eps`` and only for
    'uniform'; 'fix_zero' draws nothing and picks decomposition 0.  On a batch without decompositions ``choose`` changes nothing: no
    draw, the entries and the bits of a call without it.  An identity plan with something to choose builds the flag with tensor
    operations and leaves the coordinates alone."""
    choosing = _has_decompositions(batch, choose, choice)
    if (plan is None or plan.identity) and not choosing:
        return batch
    noise = _noise.resolve(noise)
    x_rec, x_lig = batch["protein_pos"], batch["ligand_pos"]
    dev, n_rec, n_lig = x_rec.device, int(x_rec.shape[0]), int(x_lig.shape[0])
    B = batch.get("num_graphs", None)
    if B is None:
        B = batch["num_graphs"] = int(max(batch["protein_element_batch"].max(), batch["ligand_element_batch"].max())) + 1
    B = int(B)
    if noise is not None and noise.num_graphs != B:
        raise ValueError(f"noise has {noise.num_graphs} stream keys for a batch of {B} graphs")
    if noise is not None and eps is not None:
        raise ValueError("apply_plan: pass either noise= (counter mode) or eps= (a replay), not both")
    if eps is not None and (tuple(eps.shape) != (n_rec, 3) or eps.device != dev or eps.dtype != torch.float32):
        raise ValueError(f"eps must be a float32 [{n_rec}, 3] tensor on the batch's device")
    if dev.type != "cuda" and noise is not None:
        raise ValueError("counter noise is generated by the GPU kernels: the batch must live on the GPU")
    drawn_in_kernel = choosing and noise is not None and choice is None and choose.sampling == "uniform"
    if plan is None or plan.identity:
        # no shipped diffusion list is one; the counter mode's pick is its host model (integers: the kernel's bits)
        if drawn_in_kernel:
            K = np.diff(batch["ligand_dec_ptr"].cpu().numpy())
            choice = torch.from_numpy(_noise.choose_model(noise.keys, K, noise.purpose_base))
        k = _pick_decompositions(batch, choose, choice, B)
        return dict(batch, ligand_gen_flag=_flag_of_decompositions(batch, k, B), decomposition=k.to(torch.int32))
    if dev.type != "cuda":
        k = _pick_decompositions(batch, choose, choice, B) if choosing else None
        if eps is None and plan.noise_std > 0:
            eps = torch.randn(n_rec, 3, device=dev)
        return apply_plan_tensors(batch, plan, eps if plan.noise_std > 0 else None, choose if choosing else None, k)
    from . import _native
    rec_ptr = _csr(batch, "protein_ptr", "protein_element_batch", B)
    lig_ptr = _csr(batch, "ligand_ptr", "ligand_element_batch", B)
    ctx = _context_flag(batch) if plan.center == "context" and not choosing else None      # (a choice brings its own context)
    if ctx is not None:
        ctx = ctx.contiguous().view(torch.uint8)
    x_rec, x_lig = x_rec.to(torch.float32).contiguous(), x_lig.to(torch.float32).contiguous()
    rec_out, lig_out = torch.empty_like(x_rec), torch.empty_like(x_lig)
    center = torch.empty(B, 3, dtype=torch.float32, device=dev)
    if choosing:
        return _apply_plan_choosing(batch, plan, noise, eps, choose, choice, drawn_in_kernel, B, x_rec, x_lig, rec_ptr, lig_ptr, rec_out,
                                    lig_out, center)
    head = (_native.ptr(x_rec), _native.ptr(x_lig), _native.ptr(rec_ptr), _native.ptr(lig_ptr), _native.ptr(ctx), B, n_rec, n_lig,
            float(plan.noise_std), CENTER_MODES[plan.center])
    tail = (_native.ptr(rec_out), _native.ptr(lig_out), _native.ptr(center), _native.current_stream(dev))
    if noise is not None:
        _native.check(_native.lib().cbgx_train_transform_rng(*head, _native.ptr(noise.device_keys(dev)), noise.purpose_base, *tail),
                      "cbgx_train_transform_rng")
    else:
        if eps is None and plan.noise_std > 0:
            eps = torch.randn(n_rec, 3, device=dev)
        eps = eps.contiguous() if eps is not None and plan.noise_std > 0 else None
        _native.check(_native.lib().cbgx_train_transform(*head, _native.ptr(eps), *tail), "cbgx_train_transform")
    out = dict(batch)
    out["protein_pos"], out["ligand_pos"], out["translation"] = rec_out, lig_out, center
    return out


def _apply_plan_choosing(batch, plan, noise, eps, choose, choice, drawn_in_kernel, B, x_rec, x_lig, rec_ptr, lig_ptr, rec_out, lig_out,
                         center):
    """the launch of ``apply_plan`` on a batch with decompositions: ``cbgx_train_transform_choose`` / ``_choose_rng``"""
    from . import _native
    dev, n_rec, n_lig = x_rec.device, int(x_rec.shape[0]), int(x_lig.shape[0])
    dec_ptr, gen_ptr, gen_idx = (batch[key] for key in DECOMP_KEYS)
    for key, v in zip(DECOMP_KEYS, (dec_ptr, gen_ptr, gen_idx)):
        if v.dtype != torch.int32 or v.device != dev or v.dim() != 1:
            raise ValueError(f"{key} must be a one-dimensional int32 tensor on the batch's device")
    if dec_ptr.shape[0] != B + 1 or gen_ptr.shape[0] < 1:
        raise ValueError(f"ligand_dec_ptr must have B + 1 = {B + 1} entries and ligand_gen_ptr at least one")
    dec_ptr, gen_ptr, gen_idx = dec_ptr.contiguous(), gen_ptr.contiguous(), gen_idx.contiguous()
    n_dec, n_idx = int(gen_ptr.shape[0]) - 1, int(gen_idx.shape[0])
    flag = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    picked = torch.empty(B, dtype=torch.int32, device=dev)
    head = (_native.ptr(x_rec), _native.ptr(x_lig), _native.ptr(rec_ptr), _native.ptr(lig_ptr), _native.ptr(dec_ptr), _native.ptr(gen_ptr),
            _native.ptr(gen_idx))
    sizes = (B, n_rec, n_lig, n_dec, n_idx, float(plan.noise_std), CENTER_MODES[plan.center])
    tail = (_native.ptr(rec_out), _native.ptr(lig_out), _native.ptr(center), _native.ptr(flag), _native.ptr(picked),
            _native.current_stream(dev))
    if drawn_in_kernel:
        _native.check(_native.lib().cbgx_train_transform_choose_rng(*head, *sizes, _native.ptr(noise.device_keys(dev)), noise.purpose_base,
                                                                    *tail), "cbgx_train_transform_choose_rng")
    else:
        # the pick comes from the host side (a replay, fix_zero: NULL = decomposition 0, the torch generator); the protein normals of the
        # counter mode are then filled at their own addresses first -- the bits the _rng entries draw in place
        k = None
        if choice is not None or choose.sampling != "fix_zero":
            k = _pick_decompositions(batch, choose, choice, B).to(torch.int32).contiguous()
        if plan.noise_std > 0:
            if noise is not None:
                eps = torch.empty(n_rec, 3, dtype=torch.float32, device=dev)
                _native.check(_native.lib().cbgx_noise_fill(
                    _native.ptr(noise.device_keys(dev)), _native.ptr(rec_ptr), B, n_rec, 3, 0,
                    noise.purpose_base + _noise.TRAIN_PROTEIN_NORMAL, 0, None, _native.ptr(eps), _native.current_stream(dev)),
                    "cbgx_noise_fill")
            elif eps is None:
                eps = torch.randn(n_rec, 3, device=dev)
            eps = eps.contiguous()
        else:
            eps = None
        _native.check(_native.lib().cbgx_train_transform_choose(*head, _native.ptr(k), *sizes, _native.ptr(eps), *tail),
                      "cbgx_train_transform_choose")
    out = dict(batch)
    out["protein_pos"], out["ligand_pos"], out["translation"] = rec_out, lig_out, center
    out["ligand_gen_flag"], out["decomposition"] = flag.view(torch.bool), picked
    return out


# ---- checkpoints -----------------------------------------------------------------------------------------------
def save_checkpoint(path, config, model, optimizer, scheduler, iteration, avg_val_loss):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".tmp"
    # same keys as train.py:266-273; `config` in a form the reference's scripts can unpickle without this package
    torch.save({"config": checkpoint_config(config), "model": model.state_dict(), "optimizer": optimizer.state_dict(),
                "scheduler": scheduler.state_dict() if scheduler is not None else {},
                "iteration": iteration, "avg_val_loss": avg_val_loss}, tmp)
    os.replace(tmp, path)         # never leave a truncated checkpoint behind


def load_checkpoint(path, model, optimizer=None, scheduler=None, finetune=False, device="cpu"):
    """``train.py:160-175``: weights with strict=False; optimizer / scheduler / iteration unless fine-tuning.
    Returns (first iteration, missing keys, unexpected keys)."""
    ckpt = load_checkpoint_file(path, map_location=device)
    res = model.load_state_dict(ckpt["model"], strict=False)
    it_first = 1
    if not finetune:
        if optimizer is not None:
            optimizer.load_state_dict(ckpt["optimizer"])
        if scheduler is not None and ckpt.get("scheduler"):
            scheduler.load_state_dict(ckpt["scheduler"])
        it_first = int(ckpt["iteration"])          # the reference resumes AT the saved iteration (no + 1)
    return it_first, list(res.missing_keys), list(res.unexpected_keys)


# ---- the loop --------------------------------------------------------------------------------------------------
def run(config, config_name, train_set, val_set, dev, logdir, tag="", resume=None, finetune=False, max_iters=None,
        log=print, noise="torch", data_transforms=True):
    """``data_transforms`` (default on): every training batch goes through the per-visit transforms of ``config.data.train.transform``,
    every validation batch through those of ``config.data.val.transform`` (``priors.TrainingPlan``, ``apply_plan``) before the model
    call; a config without them is not touched.  A list with ``choose_ctx_gen`` (``priors.ContextChoice``) on a set whose complexes
    carry ``ligand_gen_index`` picks one decomposition per example and visit in the same launch; the picks of a reported iteration (of
    its first ``CHOOSE_LOGGED`` graphs) are logged (``[choose]``).  Off (``--ignore_data_transforms``): protein-centred, unnoised batches for any config.
    ``noise="counter"``: every training call gets ``noise.training_noise(seed, example indices, it)``, every validation call
    ``noise.validation_noise(seed, example indices)``, and the loader is positioned from the iteration (``PositionedLoader``): the noised
    inputs of an iteration do not depend on the world size, validation is a function of the weights, and a resumed run sees the
    batches and the noise the uninterrupted run saw.  ``"torch"`` (default): the torch generator and ShardedLoader, as before."""
    if noise not in ("torch", "counter"):
        raise ValueError(f"noise must be 'torch' or 'counter', not {noise!r}")
    counter = noise == "counter"
    plan_tr = TrainingPlan.from_config(config, "train") if data_transforms else TrainingPlan()
    plan_va = TrainingPlan.from_config(config, "val") if data_transforms else TrainingPlan()
    # the list's choose_ctx_gen: it acts only on sets that carry decompositions (ligand_gen_index)
    choose_tr = ContextChoice.from_config(config, "train") if data_transforms and getattr(train_set, "has_dec", False) else None
    choose_va = ContextChoice.from_config(config, "val") if data_transforms and getattr(val_set, "has_dec", False) else None
    rank, world, _ = sharding.env_rank_world()
    if rank == 0 and not (plan_tr.identity and plan_va.identity and choose_tr is None and choose_va is None):
        chosen = f" | choice train {choose_tr} | val {choose_va}" if choose_tr is not None or choose_va is not None else ""
        log(f"[data] train {plan_tr} | val {plan_va}{chosen}")
    tc, ec = config.train, config.get("eval", {})
    max_iters = int(max_iters if max_iters is not None else tc.max_iters)
    val_freq = int(ec.get("val_freq", 1000))
    report_freq = int(tc.get("report_freq", 100))
    weights = tc.get("loss_weights", None)
    torch.manual_seed(int(tc.get("seed", 2022)) + rank)          # per-rank noise / time draws
    model = get_model(config.model).to(dev)
    optimizer = get_optimizer(tc.optimizer, model)
    scheduler = get_scheduler(tc.get("scheduler", None), optimizer)
    evaluator = Evaluator(ec.get("metrics", []))                  # train.py:141
    it_first = 1
    if resume:
        it_first, missing, unexpected = load_checkpoint(resume, model, optimizer, scheduler, finetune, device=dev)
        if rank == 0:
            log(f"[resume] {resume}: iteration {it_first}, missing keys {len(missing)}, unexpected {len(unexpected)}")
    else:
        broadcast_parameters(model)                              # every replica starts from rank 0's initialisation
    flat = FlatGradients(model)
    seed = int(tc.get("seed", 2022))
    if counter:
        positioned = PositionedLoader(len(train_set), int(tc.batch_size), rank, world, seed=seed)
    else:
        train_it = iter(ShardedLoader(len(train_set), int(tc.batch_size), rank, world, seed=seed))
    val_batches = ShardedLoader(len(val_set), int(tc.batch_size), rank, world, shuffle=False).epoch(0)
    ckpt_dir = os.path.join(logdir, tag or config_name, "checkpoints")
    best_loss, best_iter, history, metric_history = None, None, [], []
    t_last = time.perf_counter()
    for it in range(it_first, max_iters + 1):
        if counter:
            batch = train_set.collate(positioned.batch(it), dev, example_ids=True, ptrs=not plan_tr.identity,
                                      decomps=choose_tr is not None)
            step_noise = {"noise": _noise.training_noise(seed, batch["example_index"], it)}
        else:
            batch, step_noise = train_set.collate(next(train_it), dev, ptrs=not plan_tr.identity, decomps=choose_tr is not None), {}
        batch = apply_plan(batch, plan_tr, choose=choose_tr, **step_noise)
        loss, loss_dict, grad_norm, t_ar = train_step(model, batch, optimizer, flat, weights,
                                                      max_grad_norm=float(tc.get("max_grad_norm", 8.0)), **step_noise)
        if it % report_freq == 0 and rank == 0:
            now = time.perf_counter()
            parts = " | ".join(f"loss({k}) {float(v):.4f}" for k, v in loss_dict.items())
            log(f"[train] iter {it:05d} | loss {float(loss):.4f} | {parts} | grad {float(grad_norm):.4f} | "
                f"lr {optimizer.param_groups[0]['lr']:.3e} | {1e3 * (now - t_last) / report_freq:.1f} ms/iter "
                f"(all-reduce {1e3 * t_ar:.2f} ms)")
            t_last = now
            if "decomposition" in batch:
                # (the report has synchronised already; a large batch shows its first CHOOSE_LOGGED graphs)
                more = f" (+ {batch['num_graphs'] - CHOOSE_LOGGED} more)" if batch["num_graphs"] > CHOOSE_LOGGED else ""
                ex = f" | examples {batch['example_index'][:CHOOSE_LOGGED].tolist()}" if "example_index" in batch else ""
                log(f"[choose] iter {it:05d}{ex} | decomposition {batch['decomposition'][:CHOOSE_LOGGED].tolist()}{more}")
        if it % val_freq == 0:
            if counter:
                # the validation draws (protein noise, a uniform choice) are functions of (seed, example): the loss one of the weights
                val_noise = lambda b: _noise.validation_noise(seed, b["example_index"])
                val_draws = plan_va.noise_std > 0 or (choose_va is not None and choose_va.sampling == "uniform")
                avg, metrics = validate(model, (apply_plan(b, plan_va, noise=val_noise(b) if val_draws else None, choose=choose_va)
                                                for b in (val_set.collate(ids, dev, example_ids=True, ptrs=not plan_va.identity,
                                                                          decomps=choose_va is not None)
                                                          for ids in val_batches)), weights, evaluator, noise_for=val_noise)
            else:
                avg, metrics = validate(model, (apply_plan(val_set.collate(ids, dev, ptrs=not plan_va.identity,
                                                                           decomps=choose_va is not None), plan_va, choose=choose_va)
                                                for ids in val_batches), weights, evaluator)
            history.append((it, avg))
            metric_history.append((it, metrics))
            if scheduler is not None and it != it_first:         # train.py:247-251
                scheduler.step(avg) if tc.scheduler.type == "plateau" else scheduler.step()
            improved = best_loss is None or avg < best_loss or it % int(ec.get("force_save_freq", 1000000)) == 0
            if improved:
                best_loss, best_iter = avg, it
                if rank == 0:
                    save_checkpoint(os.path.join(ckpt_dir, "%d.pt" % it), config, model, optimizer, scheduler, it, avg)
            if rank == 0:
                log(f"[validate] iter {it:05d} | loss {avg:.6f} | " + "".join(f"{k} {v:.4f} | " for k, v in metrics.items()) +
                    ("saved" if improved else
                    f"not improved (best {best_loss:.6f} at iter {best_iter})"))
            sharding.barrier()
    return {"model": model, "optimizer": optimizer, "scheduler": scheduler, "history": history, "metrics": metric_history,
            "best_iter": best_iter,
            "ckpt_dir": ckpt_dir}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--logdir", default="./logs")
    ap.add_argument("--tag", default="")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--data", default=None, help="torch file with a list of complex dicts (see module docstring)")
    ap.add_argument("--val_data", default=None, help="validation complexes; default: the last 10 %% of --data")
    ap.add_argument("--synthetic", type=int, default=256, help="number of synthetic complexes when --data is not given")
    ap.add_argument("--synthetic_decompositions", type=int, default=0,
                    help="K > 0: every synthetic complex carries K seeded decompositions (ligand_gen_index) for the config's "
                         "choose_ctx_gen to pick from; 0: the complexes of a run without the option")
    ap.add_argument("--resume", default=None)
    ap.add_argument("--finetune", action="store_true")
    ap.add_argument("--max_iters", type=int, default=None)
    ap.add_argument("--noise", choices=("torch", "counter"), default="torch",
                    help="counter: time and noise of every training and validation call are functions of (seed, example, iteration) "
                         "-- independent of world size, batch size and batch position; resume continues data order and noise")
    ap.add_argument("--ignore_data_transforms", action="store_true",
                    help="do not apply the config's per-visit transforms (add_pos_noise, center_pos / center_whole_pos of "
                         "data.train.transform / data.val.transform): protein-centred, unnoised batches for any config")
    args = ap.parse_args(argv)

    rank, world, local = sharding.init_process_group()
    config, config_name = load_config(args.config)
    set_num_atom_type(config)
    if not (args.device.startswith("cuda") and torch.cuda.is_available()):
        raise SystemExit("training needs an MI355X: the message-passing path has no CPU fallback")
    local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.data:
        raw = torch.load(args.data, map_location="cpu", weights_only=False)
        if args.val_data:
            tr, va = raw, torch.load(args.val_data, map_location="cpu", weights_only=False)
        else:
            k = max(1, len(raw) // 10)
            tr, va = raw[:-k], raw[-k:]
    else:
        raw = synthetic_complexes(max(args.synthetic, 2), int(config.train.get("seed", 2022)), config.model.num_atomtype,
                                  decompositions=max(args.synthetic_decompositions, 0))
        k = max(1, len(raw) // 10)
        tr, va = raw[:-k], raw[-k:]
    resume = args.resume or config.get("resume", None)
    out = run(config, config_name, ComplexSet(tr), ComplexSet(va), dev, args.logdir, args.tag, resume, args.finetune,
              args.max_iters, noise=args.noise, data_transforms=not args.ignore_data_transforms)
    if rank == 0:
        print(f"done: best validation loss at iteration {out['best_iter']}, checkpoints in {out['ckpt_dir']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
