"""Sampling driver: the role of the reference's ``sample.py`` (config -> model -> per-pocket batches ->
``model.sample`` -> one result file per pocket), minus dataset parsing and RDKit reconstruction (out of scope,
SURVEY.md section 2), plus rank sharding of the pocket loop (``sample.py:159`` is embarrassingly parallel).

    python -m cbgbench_amd.sample_cli --config cfg.yml --out_root results [--checkpoint ckpt.pt]
                                      [--pockets pockets.pt | --synthetic 16] [--num_samples 10] [--pockets_per_batch 10]
    python -m cbgbench_amd.launch --nproc 8 -m cbgbench_amd.sample_cli ...      # rank r takes pockets r, r+W, ...; no port to pass

Pocket input: a ``torch.save``d list of dicts with ``protein_pos [n,3]``, ``protein_atom_feature [n,7]``,
``protein_aa_type [n]`` (what ``featurize_protein_fa`` + ``center_pos`` produce, protein_featurizer.py:21-30),
or synthetic pockets.

The task comes from the config's transform list (``priors.SamplingPlan.from_config``): de-novo configs (``assign_molsize``)
sample whole ligands; linker / frag / scaffold / sidechain configs (``assign_gensize`` + ``assign_genatomtype`` + ``center_pos``
on the context atoms + ``assign_genpos``; configs/linker/test/targetdiff.yml:12-28) keep per-pocket CONTEXT atoms fixed and
generate the rest.  Context atoms -- what ``choose_ctx_gen`` + ``remove_ligand_gen`` leave of the native ligand
(select.py:21-88, molecule_featurizer.py:175-205) -- come with the pockets (``ligand_ctx_pos [c,3]``, ``ligand_ctx_atom_type [c]``
in each pocket dict, same frame as ``protein_pos``) or from ``--context`` (a ``torch.save``d list, one ``{'pos', 'atom_type'}``
per pocket); synthetic pockets get synthetic fragments.  Every sample's frame is then centred on its context atoms' mean and
``protein_translation`` records the shift (sample.py:198-201 adds it back: ``sampling.translate``, on in the shipped configs).
Output: ``{out_root}/{tag}/pocket_{i:05d}.pt`` with the final ligand positions, atom types and
(optionally) the trajectory for each sample -- the tensors ``sample.py:198-206`` hands to reconstruction.
``--geometry`` adds a stability and steric-clash report per sample, computed on the device in one launch per batch
(cbgbench_amd/geometry.py), and ``{out_dir}/geometry_summary.json`` for the job.
``--bonds`` adds the table-bond graph of every sample -- bond list, fragment labels, connectivity -- computed on the device in two
launches per batch (``geometry.batch_bonds``), and ``{out_dir}/bonds_summary.json`` for the job.
``--rings`` adds the ring sizes of that graph -- rings of every size 3 ... 9 in a minimum cycle basis, rings above 9, the shortest ring
through every atom -- computed on the device in one more launch per batch (``geometry.batch_rings``), and
``{out_dir}/rings_summary.json`` for the job.
``--distributions`` adds the bond angles of that graph to every sample and, per pocket and for the job, the three histograms the
reference's geometry report compares with a dataset's by Jensen-Shannon distance -- pair distances (All_12A, CC_2A), bond lengths per
bond type, bond angles per angle type -- computed on the device in two more launches per batch (``geometry.batch_distributions``), and
``{out_dir}/distributions_summary.json`` for the job; ``--distributions_reference`` adds the distances to the caller's own vectors.
``--aromatic`` adds the aromatic atoms and bonds of that graph -- the closure of the model's aromatic flags under the reference's
reconstruction rules over the chordless 5- and 6-cycles, bond type 4 for the edges of aromatic cycles -- computed on the device in one more
launch per batch (``geometry.batch_aromatic``), and ``{out_dir}/aromatic_summary.json`` for the job; with ``--distributions`` the bond-length
and bond-angle profiles are then keyed by four bond types (``6:6``, ``6:6:6``).
``--valence`` asks whether the sample is a molecule at all: Kekule orders for the aromatic bonds, implicit hydrogens and a valence check per
atom on that graph, computed on the device in one more launch per batch (``geometry.batch_valence``), with the formula, the molecular
weight and ``mol_valid`` per sample and ``{out_dir}/valence_summary.json`` for the job.
``--interactions`` asks how the sample sits in its pocket: donor / acceptor / hydrophobic types of both sides, rotatable bonds and the five
pair terms of Vina's functional form, computed on the device in two more launches per batch (``geometry.batch_interactions``), with
``score`` per sample and ``{out_dir}/interactions_summary.json`` for the job.  This library's own typing: not the Vina program.
``--groups`` asks which functional groups the sample holds: members by marking rules, groups as connected components under the group
bonds, each group's class out of the reference's 25 names by an exact isomorphism test, computed on the device in one more launch per batch
(``geometry.batch_groups``), with the group names per sample and ``{out_dir}/groups_summary.json`` for the job; ``--groups_reference`` adds
the MAE and the Jensen-Shannon distance to the caller's own ratios and distribution.  Marking rules of this library's own: not the EFGs program.
``--diversity`` asks whether the samples of a pocket are different molecules: a fingerprint and a hash per sample by colour refinement of
that graph, then per pocket the duplicates, every pair's Tanimoto similarity and each sample's nearest neighbour, computed on the device
in two more launches per batch (``geometry.batch_diversity``), with ``{out_dir}/diversity_summary.json`` for the job.  A fingerprint of
this library's own, not RDKit's; equal hashes are equivalence under the refinement, not isomorphism.
``--native`` (with ``--pockets`` whose dicts carry ``ligand_pos`` / ``ligand_atom_type``) compares every sample with the ligand its
pocket was crystallised with: that ligand goes through the same reports as one more graph per pocket, two more kernels say which pocket
atoms a ligand touches and compare fingerprints, contact sets and centroids (``geometry.batch_native``), and the reference's MPBG / IMP /
LBE formulas (``calculate_vina_metrics``) are taken on the scores of ``--interactions``, with ``{out_dir}/native_summary.json`` for the job.
It inherits the deviations of ``--interactions`` and ``--diversity``: a score in Vina's functional form, not Vina; a fingerprint of this
library's own, not RDKit's.  The contact Jaccard index and the centroid distance are descriptors of this library's own.
``--sdf`` writes ``pocket_{i:05d}.sdf`` beside every result file: one V2000 record per sample, bond types the Kekule orders of ``--valence``
when given, else from ``--aromatic`` when given, table-bond orders otherwise (``geometry.sdf_record``; host side, no RDKit).
A checkpoint is the reference's format: ``{'config': ..., 'model': state_dict}`` (``sample.py:153-156``)."""
import argparse
import os
import time

import numpy as np
import torch

from . import get_model, load_config, priors, set_num_atom_type, sharding, synthetic
from .config import NUM_ATOM_TYPES, get_atomic_number_from_index, is_aromatic_from_index, load_checkpoint_file
from .sample_reports import SampleReports


def build_pocket_batch(pockets, num_samples, rng, num_classes, prior_types="uniform", device="cpu", num_dist=None,
                       generator=None, plan=None, context=None, sample_streams=None):
    """num_samples replicas of every pocket with fresh priors (sample.py:177-183; init_lig.py:232-258, 376-432), built
    for the whole batch at once on ``device`` (cbgbench_amd/priors.py).  ``plan`` (priors.SamplingPlan) selects the priors and the
    centring; ``context``: per pocket (pos, atom_type) of the fixed atoms of a linker / frag / scaffold / sidechain job;
    ``sample_streams`` = (seed, pocket ids): ``--noise counter``, every graph draws from its own stream (``rng`` is then unused)."""
    ps = priors.PocketSet(pockets, device=device, center=False)   # pocket files are already centred (center_pos)
    if plan is None:
        return priors.build_sampling_batch(ps, num_samples, num_classes, num_dist=num_dist, rng=rng, generator=generator,
                                           type_prior=prior_types, sample_streams=sample_streams)
    if plan.task == "context" and context is None:
        raise ValueError("the config asks for a context task (assign_gensize) but no context atoms were given")
    return priors.build_sampling_batch(ps, num_samples, num_classes, num_dist=num_dist, rng=rng, generator=generator,
                                       type_prior=plan.type_prior, pos_prior=plan.pos_prior,
                                       context=context if plan.task == "context" else None,
                                       center_on_context=plan.task == "context" and plan.center == "context",
                                       sample_streams=sample_streams)


def load_context(raw_pockets, path, choose=None, rng=None, counter=False):
    """per-pocket context atoms [(pos [c,3] float32, atom_type [c] int64)] from the pocket dicts' ``ligand_ctx_*`` keys or from a
    ``--context`` file (a list with one {'pos', 'atom_type'} dict or (pos, atom_type) pair per pocket); None when neither exists.
    Pockets that carry the native ligand and its decompositions instead (``ligand_pos``, ``ligand_atom_type``, ``ligand_gen_index``: a
    list of K >= 1 index arrays, the reference's ``gen_index``) and no ``ligand_ctx_*``: the context is the complement of the
    decomposition that ``choose`` (``priors.ContextChoice``: the config's ``choose_ctx_gen``) names -- decomposition 0 without the entry
    (what ``remove_ligand_gen`` would leave) and under ``fix_zero``; under ``uniform`` one ``rng.integers(K)`` per pocket, in pocket
    order, which ``counter=True`` (``--noise counter``: no shared stream) refuses."""
    def one(pos, typ):
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        typ = np.asarray(typ, np.int64).reshape(-1)
        if pos.shape[0] != typ.shape[0]:
            raise ValueError(f"context: {pos.shape[0]} positions but {typ.shape[0]} atom types")
        return pos, typ
    if path:
        raw = torch.load(path, map_location="cpu", weights_only=False)
        out = [one(c["pos"], c["atom_type"]) if isinstance(c, dict) else one(c[0], c[1]) for c in raw]
        if raw_pockets is not None and len(out) != len(raw_pockets):
            raise ValueError(f"--context has {len(out)} entries for {len(raw_pockets)} pockets")
        return out
    if raw_pockets is not None and all("ligand_ctx_pos" in p for p in raw_pockets):
        return [one(p["ligand_ctx_pos"], p["ligand_ctx_atom_type"]) for p in raw_pockets]
    if raw_pockets is not None and len(raw_pockets) and all("ligand_gen_index" in p and "ligand_pos" in p and "ligand_atom_type" in p
                                                            for p in raw_pockets):
        uniform = choose is not None and choose.sampling == "uniform"
        if uniform and counter:
            raise ValueError("choose_ctx_gen with sampling 'uniform' draws from a shared stream: not available with --noise counter "
                             "(the shipped test lists use fix_zero)")
        if uniform and rng is None:
            raise ValueError("choose_ctx_gen with sampling 'uniform' needs a generator (rng=)")
        out = []
        for k, p in enumerate(raw_pockets):
            pos, typ = one(p["ligand_pos"], p["ligand_atom_type"])
            decs = list(p["ligand_gen_index"])
            if not decs:
                raise ValueError(f"ligand_gen_index of pocket {k} is an empty list: a pocket needs at least one decomposition")
            gen = np.asarray(decs[int(rng.integers(len(decs))) if uniform else 0]).reshape(-1).astype(np.int64)
            if gen.size and (gen.min() < 0 or gen.max() >= typ.shape[0]):
                raise ValueError(f"ligand_gen_index of pocket {k} has an index outside [0, {typ.shape[0]})")
            ctx = np.ones(typ.shape[0], dtype=bool)
            ctx[gen] = False
            out.append((pos[ctx], typ[ctx]))
        return out
    return None


def load_native(raw_pockets, num_classes):
    """``--native``: per pocket (pos [n, 3] float32, atom_type [n] int64) of the ligand the pocket file carries (``ligand_pos``,
    ``ligand_atom_type``: indices of the ``num_classes`` types the samples are decoded with), n >= 1; whatever else a context task reads
    of the dict (``ligand_gen_index``) changes nothing.  A pocket without them, a length mismatch or a type out of range is a SystemExit
    naming the pocket"""
    out = []
    for k, p in enumerate(raw_pockets):
        if "ligand_pos" not in p or "ligand_atom_type" not in p:
            raise SystemExit(f"sample_cli: --native: pocket {k} carries no ligand_pos / ligand_atom_type")
        pos, typ = np.asarray(p["ligand_pos"], np.float32), np.asarray(p["ligand_atom_type"], np.int64).reshape(-1)
        if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] != typ.shape[0] or typ.shape[0] < 1:
            raise SystemExit(f"sample_cli: --native: pocket {k}: ligand_pos {tuple(pos.shape)} and ligand_atom_type {tuple(typ.shape)} "
                             f"are not [n, 3] and [n] with n >= 1")
        if typ.min() < 0 or typ.max() >= num_classes:
            raise SystemExit(f"sample_cli: --native: pocket {k}: ligand_atom_type out of range [0, {num_classes})")
        out.append((np.ascontiguousarray(pos), typ))
    return out


def split_samples(x, c, batch_idx, n_graphs, mode="add_aromatic"):
    """per-graph records like ``split_batch_into_samples`` (sample.py:16-32): ``pos``, ``type`` (index), ``atom`` (atomic
    numbers) and ``aromatic`` (flags, None in 'basic' mode) -- the arguments of ``reconstruct_mol`` (sample.py:211-214) -- plus
    the raw ``type_vector``."""
    out = []
    for g in range(n_graphs):
        m = batch_idx == g
        typ = c[m].argmax(-1) if c.dim() == 2 else c[m]
        out.append({"pos": x[m].clone(), "type": typ.clone(), "atom_type": typ.clone(),
                    "atom": get_atomic_number_from_index(typ.tolist(), mode),
                    "aromatic": is_aromatic_from_index(typ.tolist(), mode), "type_vector": c[m].clone()})
    return out


def decode_mode(plan_mode, config_mode, num_classes):
    """the atom-type vocabulary the samples are decoded with (sample.py:211-214 passes the transform's ``mode`` on to
    ``reconstruct_mol``): the ``mode`` of the config's assign_atomtype / assign_genatomtype transform (``SamplingPlan.mode``), else the
    top-level ``config.mode`` -- and it must be the vocabulary the model's ``num_atomtype`` was built with"""
    for mode in (plan_mode, config_mode):
        if mode in NUM_ATOM_TYPES and NUM_ATOM_TYPES[mode] == num_classes:
            return mode
    raise ValueError(f"no atom-type vocabulary of {num_classes} classes among the config's modes "
                     f"(transform mode {plan_mode!r}, config.mode {config_mode!r}; known: {dict(NUM_ATOM_TYPES)})")


def main(argv=None, stats=None):
    """``stats`` (optional dict): filled with the wall seconds of the phases (setup = config + model + weights, batch = prior
    construction, sample = model.sample incl. the trajectory download, write = per-pocket records and files) and, for every requested report
    (geometry, bonds, rings, aromatic, distributions, valence, interactions, groups, diversity, native: evaluated in that order), its own launches and downloads, a part of write: the bond
    list and the ring report are made once per batch, and where they were not asked for their time goes to the first requested report
    in that order that needs them (cbgbench_amd/sample_reports.py)."""
    t_phase = time.perf_counter()
    phases = {"setup": 0.0, "batch": 0.0, "sample": 0.0, "write": 0.0}

    def lap(name, dev=None):
        nonlocal t_phase
        if dev is not None and dev.type == "cuda":
            torch.cuda.synchronize(dev)
        now = time.perf_counter()
        phases[name] += now - t_phase
        t_phase = now

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--out_root", default="./results")
    ap.add_argument("--tag", default="")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--pockets", default=None, help="torch file with a list of pocket dicts")
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic pockets when --pockets is not given")
    ap.add_argument("--num_samples", type=int, default=None)
    ap.add_argument("--pockets_per_batch", type=int, default=10)
    ap.add_argument("--streams", type=int, default=3,
                    help="batches kept in flight together on this many HIP streams (model.sample_many; 1 = one batch after the other)")
    ap.add_argument("--random_init", action="store_true",
                    help="sample from randomly initialised weights when no checkpoint is given / found (smoke runs only)")
    ap.add_argument("--save_traj", action="store_true")
    ap.add_argument("--final_state", action="store_true",
                    help="write traj[-1] (the state after the last step) instead of traj[0], which sample.py:198 uses")
    ap.add_argument("--context", default=None,
                    help="linker / frag / scaffold / sidechain configs: torch file with one {'pos' [c,3], 'atom_type' [c]} per pocket "
                         "(the fixed atoms, same frame as protein_pos); default: the pockets' ligand_ctx_pos / ligand_ctx_atom_type")
    ap.add_argument("--no_translate", action="store_true",
                    help="keep results in the sampling frame (default: add protein_translation back when the config's "
                         "sampling.translate is set, sample.py:198-201)")
    ap.add_argument("--noise", choices=("torch", "counter"), default="torch",
                    help="torch: priors and step noise from the seeded torch / numpy generators (seed + rank; the samples depend on the "
                         "number of ranks, --pockets_per_batch, --streams and the pocket order).  counter: every random number is a "
                         "function of (seed, pocket index, sample index, atom, step), generated in the step kernels: a pocket's file "
                         "is the same however the job is split (cbgbench_amd/noise.py).  GPU only (the generator lives in the step "
                         "kernels: --device cpu raises).  Nothing seeds torch in this mode, so --random_init weights differ from process "
                         "to process: compare runs through a --checkpoint")
    ap.add_argument("--geometry", action="store_true",
                    help="add a geometry report to every sample (nr_bonds, atom_stable, inter_clash, intra_clash_table_bonds, mol_stable), "
                         "a `geometry` dict of counts to every pocket record and {out_dir}/geometry_summary.json: atom / molecule "
                         "stability and protein-ligand steric clash of the state the record holds, evaluated on the GPU in the "
                         "sampling frame against the batch's own protein_pos, one launch per batch (cbgbench_amd/geometry.py).  "
                         "Intra-ligand clashes exclude pairs with a TABLE bond (the reference uses RDKit's bonds)")
    ap.add_argument("--bonds", action="store_true",
                    help="add the table-bond graph to every sample (bond_index [2, nb] ligand-local with i < j, bond_order, bond_length, "
                         "fragment = smallest index of the atom's connected component, n_fragments, connected), a `bonds` dict of counts "
                         "to every pocket record and {out_dir}/bonds_summary.json: which atoms are bonded and whether the sample is one "
                         "molecule, of the state the record holds, evaluated on the GPU in two launches per batch "
                         "(cbgbench_amd/geometry.py).  TABLE bonds from the stability metric's bond lengths, not RDKit's: no "
                         "aromaticity, no valence repair.  Independent of --geometry")
    ap.add_argument("--rings", action="store_true",
                    help="add the ring sizes of the table-bond graph to every sample (ring_sizes [7] = rings of size 3 ... 9 in a "
                         "minimum cycle basis, n_rings_larger, atom_ring_min = the shortest ring through every atom, ring_status), a "
                         "`rings` dict of counts to every pocket record and {out_dir}/rings_summary.json: the ring ratios of the "
                         "reference's quality path, of the state the record holds, evaluated on the GPU in one launch per batch on the "
                         "bond list (cbgbench_amd/geometry.py).  A sample above 256 atoms or 128 independent cycles is reported "
                         "(ring_status != 0, sizes -1) and left out of the ratios.  Rings of TABLE bonds, not RDKit's SSSR.  Independent "
                         "of --geometry and --bonds: without --bonds the bonds are computed and not written")
    ap.add_argument("--distributions", action="store_true",
                    help="add the bond angles of the table-bond graph to every sample (angle_index [3, n] ligand-local rows a, c, b; "
                         "angle_cos; angle_deg, for convenience only: never binned; angle_type; distribution_status), a `distributions` "
                         "dict of integer histograms to every pocket record (pair distances [2, 101], bond lengths and bond angles by "
                         "type) and {out_dir}/distributions_summary.json: the normalised pair-distance (All_12A, CC_2A), bond-length and "
                         "bond-angle profiles of the reference's geometry report, of the state the record holds, evaluated on the GPU in "
                         "two launches per batch on the bond list (cbgbench_amd/geometry.py).  Angles are binned in cosine space.  A sample "
                         "above 16384 angles is reported (distribution_status != 0) and contributes no angles.  TABLE bonds, not RDKit's: "
                         "no aromatic type.  Independent of --geometry, --bonds and --rings: without --bonds the bonds are computed and "
                         "not written")
    ap.add_argument("--distributions_reference", default=None,
                    help="with --distributions: a .npz or torch.save'd dict {key: vector} of the caller's own reference distributions "
                         "(keys 'All_12A', 'CC_2A', bond types like '6-6', angle types like '6-6=8' in either orientation; none ship "
                         "with this package); distributions_summary.json then carries their Jensen-Shannon distances as JSD_<key>")
    ap.add_argument("--aromatic", action="store_true",
                    help="add the aromatic report to every sample (aromatic_atom = on an aromatic cycle, aromatic_bond [nb] aligned with "
                         "the bond_index of --bonds, bond_type = 4 for an aromatic bond else the order, n_aromatic_rings, "
                         "aromatic_status), an `aromatic` dict of counts to every pocket record and {out_dir}/aromatic_summary.json: the "
                         "closure of the model's aromatic flags (the sample's `aromatic` field, which stays as it is) under the rules of "
                         "the reference's reconstruct_mol over the chordless 5- and 6-cycles of the table-bond graph, evaluated on the "
                         "GPU in one launch per batch on the bond list and the ring report (cbgbench_amd/geometry.py).  add_aromatic "
                         "atom types only.  A bond is aromatic as an edge of an aromatic cycle (the link of biphenyl is not).  "
                         "Independent of --bonds and --rings: without them bonds and rings are computed and not written.  With "
                         "--distributions the bond-length and bond-angle blocks are keyed by four bond types (6:6, 6:6:6)")
    ap.add_argument("--valence", action="store_true",
                    help="add the valence report to every sample (implicit_h and valence_flags per atom: 1 valence exceeded, 2 on an "
                         "aromatic system without a Kekule structure, 4 unknown element, 8 on an aromatic system; bond_kekule [nb] aligned "
                         "with the bond_index of --bonds: the aromatic bonds as 1 / 2, 4 where no Kekule structure exists; formula, "
                         "mol_weight, n_nhoh, n_no, valence_ok, mol_valid = valence_ok and one fragment, valence_status), a `valence` "
                         "dict of counts to every pocket record and {out_dir}/valence_summary.json, evaluated on the GPU in one launch "
                         "per batch on the bond list and, with add_aromatic atom types, the aromatic report (cbgbench_amd/geometry.py); "
                         "with basic atom types no bond is aromatic.  Valences from this library's table (H 1, C 4, N 3, O 2, F 1, P 3/5, "
                         "S 2/4/6, Cl 1), no charges: a nitro group drawn N(=O)=O counts as exceeded.  TABLE bonds, not RDKit's.  A sample "
                         "over a limit is reported (valence_status != 0) and left out of every ratio.  Independent of --bonds, --rings "
                         "and --aromatic: without them they are computed and not written.  With --sdf the records carry bond_kekule")
    ap.add_argument("--interactions", action="store_true",
                    help="add typed pocket contacts and a score in Vina's functional form to every sample (lig_xs_type [n] type bytes: "
                         "element code 1 ... 7 = C N O F P S Cl, 8 hydrophobic, 16 donor, 32 acceptor; atom_terms [n, 5] and "
                         "interaction_terms [5] float64: gauss1, gauss2, repulsion, hydrophobic, hbond; bond_rotatable [nb] aligned with "
                         "the bond_index of --bonds, n_rotatable; score_inter = the terms under Vina's published weights, score = "
                         "score_inter / (1 + 0.05846 n_rotatable); n_hbond_pairs, n_hydrophobic_pairs, n_close_pairs, n_contact_atoms, "
                         "interactions_status), an `interactions` dict of counts to every pocket record and "
                         "{out_dir}/interactions_summary.json, evaluated on the GPU in two launches per batch on the bond list, the "
                         "valence report and the pocket's residue types (cbgbench_amd/geometry.py).  This library's own atom typing on "
                         "TABLE bonds, no hydrogens or protonation states in the pocket, no intramolecular term: NOT the Vina program "
                         "and not validated against it.  A sample over a limit is reported (interactions_status != 0) and left out of "
                         "every ratio.  Independent of every other flag: what it needs is computed and not written")
    ap.add_argument("--groups", action="store_true",
                    help="add the functional groups to every sample (atom_group [n]: the smallest atom of the atom's group, -1 in no "
                         "group; atom_class [n]: 0 ... 24 the reference's 25 named groups, 25 other, 254 in no group; groups: the names of "
                         "the sample's groups in the order of their smallest atoms, 'other' included; n_groups, fg_counts [26], "
                         "groups_status), a `groups` dict of counts to every pocket record and {out_dir}/groups_summary.json (fg_ratio, "
                         "fg_distribution as the reference's eval_fg_type_ratio / _distribution), evaluated on the GPU in one launch per "
                         "batch on the bond list and, with add_aromatic atom types, the aromatic report (cbgbench_amd/geometry.py); with "
                         "basic atom types no bond is aromatic.  Members: aromatic atoms, hetero atoms, unsaturated, acetal and "
                         "hetero-triangle carbons; a group's class is isomorphism with a template graph.  TABLE bonds, marking rules of "
                         "this library's own: NOT the EFGs program, no agreement with it is claimed; no charges; a single-atom group is "
                         "'other'.  A sample over a limit is reported (groups_status != 0) and left out of every ratio.  Independent of "
                         "every other flag: what it needs is computed and not written")
    ap.add_argument("--diversity", action="store_true",
                    help="add what the samples of a pocket share: to every sample fingerprint [32] (int32 words of a 1024-bit "
                         "fingerprint), mol_hash (a Python int below 2**64), duplicate_of (the index, among the pocket's samples, of the "
                         "first one with the same hash: its own if it is the first), nearest_sample and nearest_similarity (the most "
                         "similar other sample; -1 and nan if none) and diversity_status; to every pocket record similarity_micro [n, n] "
                         "(Tanimoto similarities in millionths, -1 for a sample that was not evaluated) and a `diversity` dict of counts "
                         "(n_unique, n_pairs, sim_micro_sum, diversity_micro = 1000000 - the rounded mean pair similarity); and "
                         "{out_dir}/diversity_summary.json (unique_mol_ratio, mean_pocket_diversity = the per-pocket average of 1 - mean "
                         "pairwise similarity, collapsed_pocket_ratio), evaluated on the GPU in two launches per batch on the bond list, "
                         "the ring report and, with add_aromatic atom types, the aromatic report (cbgbench_amd/geometry.py).  Integer "
                         "work only: colour refinement from (element, degree, aromatic, smallest ring) over the typed bonds.  Equal "
                         "hashes mean equivalence under that refinement, up to 64-bit collisions: NOT a proof of isomorphism.  A "
                         "fingerprint of this library's own in the manner of ECFP4 on TABLE bonds: neither RDKit's Morgan fingerprint nor "
                         "RDKFingerprint, no agreement with them is claimed.  Uniqueness is per pocket.  A sample over a limit is reported "
                         "(diversity_status != 0) and left out of every number.  Independent of every other flag: what it needs is "
                         "computed and not written")
    ap.add_argument("--native", action="store_true",
                    help="with --pockets whose dicts carry the pocket's own ligand (ligand_pos [n, 3], ligand_atom_type [n]: indices of "
                         "the vocabulary the samples are decoded with; the whole ligand in a context task too): compare every sample "
                         "with it.  Adds to every sample native_similarity (Tanimoto similarity of the two fingerprints), "
                         "native_same_hash, native_contact_jaccard / native_contact_common / native_contact_union (the heavy pocket atoms "
                         "within 4 A of a heavy ligand atom that both touch), native_centroid_distance, score_minus_native, "
                         "better_than_native (None where either score is missing), ligand_efficiency (score / heavy atoms) and "
                         "native_status; to every pocket record `native` (the ligand's own record with the fields of every requested "
                         "report, plus score, score_micro, n_contact_atoms and n_pocket_contact_atoms: the pocket atoms it touches) and `native_comparison` (integer counts); and "
                         "{out_dir}/native_summary.json (improved_mol_ratio, mean_binding_gap, mean_score, mean_native_score, "
                         "mean_ligand_efficiency as per-pocket averages: the reference's IMP, MPBG, Evina and LBE of "
                         "calculate_vina_metrics; mean_native_similarity, rediscovered_mol_ratio, mean_contact_jaccard, "
                         "pockets_with_rediscovery_ratio; pockets with a positive native score are left out as there), evaluated on the "
                         "GPU (cbgbench_amd/geometry.py batch_native).  The native ligand is moved into the sampling frame by its "
                         "pocket's translation and goes through the same kernels as a sample.  Inherits the deviations of --interactions "
                         "and --diversity: a score in Vina's functional form, NOT the Vina program; a fingerprint of this library's own, "
                         "NOT RDKit's.  The contact Jaccard index and the centroid distance are descriptors of this library's own.  "
                         "Independent of every other flag: what it needs is computed and not written")
    ap.add_argument("--groups_reference", default=None,
                    help="with --groups: a .npz or torch.save'd dict {'ratio': ..., 'distribution': ...}, each the 25 values in the order "
                         "of the vocabulary (a torch.save'd dict may hold {name: value} dicts instead; none ship with this package); "
                         "groups_summary.json then carries MAE_fg and JSD_fg")
    ap.add_argument("--sdf", action="store_true",
                    help="write pocket_XXXXX.sdf beside every pocket_XXXXX.pt: one V2000 record per sample with the positions the record "
                         "holds, bond types from --aromatic when given (4 = aromatic), else the table-bond orders (bonds are computed "
                         "when --bonds is absent; GPU only).  A sample above 999 atoms or bonds, or with an element outside "
                         "H C N O F P S Cl, is left out of the file and counted in one printed line.  No RDKit: no sanitisation, no "
                         "hydrogens")
    ap.add_argument("--atom_num_dist", default=None,
                    help="the reference's size-conditioned ligand-size histogram (repo/datasets/transforms/_atom_num_dist.npy); "
                         "without it ligand sizes are U{10..45}")
    args = ap.parse_args(argv)

    rank, world, local = sharding.init_process_group()
    config, config_name = load_config(args.config)
    set_num_atom_type(config)
    if args.device.startswith("cuda"):
        if not torch.cuda.is_available():
            raise SystemExit("sampling needs an MI355X: the message-passing path has no CPU fallback")
        local = local % torch.cuda.device_count()
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    else:
        dev = torch.device(args.device)
    reports = SampleReports.from_args(args)
    reports.refuse(dev, lambda: decode_mode(priors.SamplingPlan.from_config(config).mode, config.get("mode", None),
                                            config.model.num_atomtype))
    native_ligands = None
    if args.native:
        if not args.pockets:
            raise SystemExit("sample_cli: --native needs --pockets: the native ligand comes with its pocket (ligand_pos, ligand_atom_type)")
        native_ligands = load_native(torch.load(args.pockets, map_location="cpu", weights_only=False), config.model.num_atomtype)

    ckpt_path = args.checkpoint or config.model.get("checkpoint", None)
    if ckpt_path and os.path.exists(ckpt_path):
        ckpt = load_checkpoint_file(ckpt_path, map_location="cpu")
        model_cfg = ckpt["config"].model if "config" in ckpt else config.model
        model_cfg.num_atomtype = config.model.num_atomtype
        model = get_model(model_cfg)
        model.load_state_dict(ckpt["model"])            # strict, like sample.py:156
    elif args.random_init:
        # no checkpoints ship with the reference: explicit opt-in, and said loudly
        print(f"[sample_cli] WARNING: --random_init: sampling from a RANDOMLY INITIALISED {config.model.type} model"
              + (f" (checkpoint {ckpt_path!r} not found)" if ckpt_path else ""), flush=True)
        model = get_model(config.model)
    else:
        raise SystemExit(f"sample_cli: checkpoint {ckpt_path!r} does not exist (the reference fails here too, sample.py:150-156); "
                         f"pass --random_init to sample from random weights on purpose" if ckpt_path else
                         "sample_cli: no checkpoint given (--checkpoint or model.checkpoint in the config); pass --random_init "
                         "to sample from random weights on purpose")
    model = model.to(dev).eval()

    plan = priors.SamplingPlan.from_config(config)       # priors, centring and task of the config's transform list
    num_classes = config.model.num_atomtype
    mode = decode_mode(plan.mode, config.get("mode", None), num_classes)
    if args.pockets:
        raw = torch.load(args.pockets, map_location="cpu", weights_only=False)
        pockets = [(np.asarray(p["protein_pos"], np.float32), np.asarray(p["protein_atom_feature"], np.float32),
                    np.asarray(p["protein_aa_type"], np.int64)) for p in raw]
        context = load_context(raw, args.context, choose=priors.ContextChoice.from_config(config, "test"),
                               rng=np.random.default_rng([args.seed, 0x63686F6F]), counter=args.noise == "counter")
    else:
        rng0 = np.random.default_rng(args.seed)
        pockets = [synthetic.make_pocket(rng0, int(rng0.integers(350, 651))) for _ in range(max(args.synthetic, 1))]
        context = load_context(None, args.context) if args.context else (
            [synthetic.make_context(rng0, int(rng0.integers(10, 36)), num_classes) for _ in pockets] if plan.task == "context" else None)
    if plan.task == "context":
        if context is None:
            raise SystemExit(f"sample_cli: {args.config} is a context task (assign_gensize) -- give the fixed atoms with --context "
                             f"or as ligand_ctx_pos / ligand_ctx_atom_type in the pocket file")
        for k, (_, typ) in enumerate(context):
            if typ.size and (typ.min() < 0 or typ.max() >= num_classes):
                raise SystemExit(f"sample_cli: context atom type out of range [0, {num_classes}) in pocket {k}")
    num_samples = args.num_samples or config.get("sampling", {}).get("num_samples", 10)
    translate = bool(config.get("sampling", {}).get("translate", False)) and not args.no_translate
    num_dist = priors.NumDist.from_npy(args.atom_num_dist) if args.atom_num_dist else None

    mine = sharding.shard_indices(len(pockets), rank, world)
    out_dir = os.path.join(args.out_root, args.tag or config_name)
    os.makedirs(out_dir, exist_ok=True)
    if args.noise == "counter":
        rng = None                                      # no shared stream: priors and step noise are addressed per (pocket, sample)
    else:
        torch.manual_seed(args.seed + rank)             # independent noise streams per shard
        rng = np.random.default_rng([args.seed, rank])

    def write_results(ids, traj, batch):
        # sample.py:198-201 hands traj[0] to the reconstruction -- for targetdiff / diffbp that is the state entering the
        # last step, not traj[-1]; kept as the default for drop-in outputs, --final_state selects traj[-1]
        x, c, bidx = traj[-1] if (args.final_state and config.model.type != "diffsbdd") else traj[0]
        n_graphs = len(ids) * num_samples
        group_ptr = [k * num_samples for k in range(len(ids) + 1)]
        native = reports.native_state(batch, group_ptr, [native_ligands[i] for i in ids]) if native_ligands is not None else None
        found = reports.evaluate(dev, (x, c, bidx), batch, n_graphs, mode, group_ptr=group_ptr, native=native)
        x, c, bidx = x.cpu(), c.cpu(), bidx.cpu()
        if translate:       # back to the frame the pockets came in (sample.py:198-199; here per graph: a batch holds many pockets)
            x = x + batch["ligand_translation"].cpu()
        samples = split_samples(x, c, bidx, n_graphs, mode)
        if "ligand_gen_flag" in batch:      # context tasks: which atoms of a record were generated
            gen = batch["ligand_gen_flag"].cpu()
            for g, smp in enumerate(samples):
                smp["gen_flag"] = gen[bidx == g].clone()
        reports.annotate(samples, found)
        if native is not None:      # the native ligands' own records, in the frame the samples' are written in
            nat_x = torch.cat([torch.from_numpy(native_ligands[i][0]) for i in ids]) if translate else native["x"].cpu()
            natives = reports.annotate_native(split_samples(nat_x, native["c"].cpu(), native["lig_batch"].cpu(), len(ids), mode), found)
        for k, pid in enumerate(ids):
            g0, g1 = k * num_samples, (k + 1) * num_samples
            rec = {"pocket_index": pid, "samples": samples[g0:g1], **reports.pocket_counts(found, g0, g1)}
            if native is not None:
                rec["native"] = natives[k]
            if args.save_traj:
                rec["traj_keys"] = sorted(traj.keys())
            torch.save(rec, os.path.join(out_dir, f"pocket_{pid:05d}.pt"))
            for name, text in reports.pocket_files(f"pocket_{pid:05d}", samples[g0:g1], found, g0):
                with open(os.path.join(out_dir, name), "w") as f:
                    f.write(text)
        return n_graphs * model.num_diffusion_timesteps

    lap("setup", dev)
    timing = {}
    t0, graph_steps = time.perf_counter(), 0
    # `--streams` batches are in flight together (independent pockets: sample.py:159's loop has no order); models without
    # sample_many take them one after the other
    many = getattr(model, "sample_many", None) if (args.streams > 1 and dev.type == "cuda") else None
    group = args.pockets_per_batch * (args.streams if many is not None else 1)
    for g0 in range(0, len(mine), group):
        chunk = [mine[b0:b0 + args.pockets_per_batch] for b0 in range(g0, min(g0 + group, len(mine)), args.pockets_per_batch)]
        batches = [build_pocket_batch([pockets[i] for i in ids], num_samples, rng, num_classes, device=dev, num_dist=num_dist,
                                      plan=plan, context=[context[i] for i in ids] if context is not None else None,
                                      sample_streams=(args.seed, ids) if args.noise == "counter" else None)
                   for ids in chunk]
        lap("batch", dev)
        # (targetdiff itemises its share of the `sample` phase: static context, the T steps, the trajectory download)
        tk = {"timing": timing} if (stats is not None and config.model.type == "targetdiff") else {}
        trajs = (many(batches, streams=args.streams, **tk) if many is not None and len(batches) > 1
                 else [model.sample(b, **tk) for b in batches])
        lap("sample", dev)
        for ids, traj, b in zip(chunk, trajs, batches):
            graph_steps += write_results(ids, traj, b)
        lap("write")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    sharding.barrier()
    el, gs = sharding.reduce_max_sum(time.perf_counter() - t0, graph_steps, device=dev)
    if stats is not None:
        stats.update(phases)
        stats.update(timing)
        stats.update(reports.seconds)
    reports.finish(out_dir, rank, dev)
    if rank == 0:
        print(f"sampled {len(pockets)} pockets x {num_samples} samples on {world} rank(s): "
              f"{gs / el:.1f} graph-steps/s, results in {out_dir}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
