"""The reports of ``sample_cli`` (--geometry, --bonds, --rings, --aromatic, --distributions, --valence, --interactions, --groups, --diversity, --native, --sdf) in three stages: ``evaluate`` runs the
requested reports of one batch on the GPU and returns plain dicts of CPU tensors; ``annotate`` / ``pocket_counts`` / ``pocket_files``
turn those into the per-sample fields, the per-pocket dicts and the ``.sdf`` text on the host (CPU tensors in, no device); ``finish`` sums
the job's integer totals over the ranks, writes ``*_summary.json`` and prints one line per report.

Reports run in the order of ORDER.  What a report is computed from beside the state (NEEDS: the bond list, the ring report) is made at
most once per batch and shared; a dependency that was not asked for is computed, used and not written, and its wall time goes to the first
requested report in that order that needs it.  The valence report takes the aromatic report (and so the ring report) where the atom types
have aromatic flags ('add_aromatic'); with any other vocabulary no bond is aromatic and it needs the bond list only.

The reports of EXTRA come after those of ORDER, under the same rules, in every stage.  ``interactions`` (typed pocket contacts and a score
in Vina's functional form on this library's own atom typing: not the Vina program, not validated against it) is the first report that
reads the pocket's chemistry (``protein_aa_type``, the backbone column of ``protein_atom_feature``); it takes the bond list and the valence
report, and through the latter whatever ``needs("valence", mode)`` says.  Its job numbers are sums of integers too: every sample's score is
rounded to a whole number of millionths before the ranks add them up.

The reports of LATE come after those of EXTRA, under the same rules again.  ``groups`` (the functional groups of the substructure block:
marking rules of this library's own, not the EFGs program) takes what the valence report takes: the bond list, and the aromatic report
where the atom types have aromatic flags.

The reports of ACROSS come after those of LATE.  ``diversity`` (fingerprints and hashes of this library's own, not RDKit's; uniqueness and
Tanimoto similarity per pocket) is the first report that reads more than one graph at a time: ``evaluate`` takes the pocket -> graphs
grouping for it (``group_ptr``), and a pocket's record carries what its samples share.  It takes the bond list, the ring report and,
where the atom types have aromatic flags, the aromatic report.

The reports of AGAINST come after those of ACROSS.  ``native`` compares every sample with the ligand its pocket was crystallised with:
``evaluate`` takes that ligand of every pocket of the batch as one more state of P graphs (``native=``, built by ``native_state``), runs it
through the same functions as the samples -- the bond list, the ring, aromatic and valence reports, ``interactions`` and the fingerprints,
and whatever else was requested -- and hands both to ``geometry.batch_native``.  All of that is the report's own time.  MPBG / IMP / LBE
are the reference's formulas on this library's score in Vina's functional form, not Vina's; the fingerprint is this library's own, not
RDKit's; the contact Jaccard index and the centroid distance are descriptors of this library's own."""
import json
import os
import time

import numpy as np
import torch

from . import geometry, sharding
from .config import _AROMATIC

ORDER = ("geometry", "bonds", "rings", "aromatic", "distributions", "valence")
EXTRA = ("interactions",)        # evaluated, annotated and finished after ORDER
LATE = ("groups",)               # ... and these after EXTRA
ACROSS = ("diversity",)          # ... and these, which compare the samples of a pocket, after LATE
AGAINST = ("native",)            # ... and these, which compare every sample with its pocket's native ligand, after ACROSS
NEEDS = {"rings": ("bonds",), "aromatic": ("bonds", "rings"), "distributions": ("bonds",), "valence": ("bonds", "aromatic"),
         "interactions": ("bonds", "valence"), "groups": ("bonds", "aromatic"), "diversity": ("bonds", "rings", "aromatic"),
         "native": ("bonds", "rings", "aromatic", "valence", "interactions", "diversity")}


def needs(name, mode):
    """what report ``name`` is computed from under the atom-type vocabulary ``mode``"""
    if name in ("valence", "groups") and mode not in _AROMATIC:
        return ("bonds",)
    if name == "diversity" and mode not in _AROMATIC:
        return ("bonds", "rings")
    if name == "native" and mode not in _AROMATIC:
        return ("bonds", "rings", "valence", "interactions", "diversity")
    return NEEDS.get(name, ())


_COUNT_REPORTS = {rep.name: rep for rep in geometry.COUNT_REPORTS}
# the refusals off the GPU, in the order they are made (the check of --aromatic's atom types comes before its own)
_GPU_ONLY = {"geometry": "--geometry runs on the GPU (cbgx_ligand_geometry has no CPU fallback)",
             "bonds": "--bonds runs on the GPU (cbgx_ligand_bonds_count / _fill have no CPU fallback)",
             "rings": "--rings runs on the GPU (cbgx_ligand_rings has no CPU fallback)",
             "distributions": "--distributions runs on the GPU (cbgx_ligand_pair_hist / cbgx_ligand_angles have no CPU fallback)",
             "aromatic": "--aromatic runs on the GPU (cbgx_ligand_aromatic has no CPU fallback)",
             "valence": "--valence runs on the GPU (cbgx_ligand_valence has no CPU fallback)",
             "interactions": "--interactions runs on the GPU (cbgx_pocket_types / cbgx_ligand_interactions have no CPU fallback)",
             "groups": "--groups runs on the GPU (cbgx_ligand_groups has no CPU fallback)",
             "diversity": "--diversity runs on the GPU (cbgx_ligand_fingerprints / cbgx_group_diversity have no CPU fallback)",
             "native": "--native runs on the GPU (cbgx_pocket_contacts / cbgx_native_compare have no CPU fallback)",
             "sdf": "--sdf takes its bonds from the GPU (cbgx_ligand_bonds_count / _fill have no CPU fallback)"}
# a count report's printed line: the ratios it names, and its own tail
_LINE = {"geometry": (geometry.RATIOS, lambda c: f"{c['n_mol']} molecules, {c['n_atoms']} atoms"),
         "bonds": (geometry.BOND_RATIOS, lambda c: f"{c['n_mol']} molecules, {c['n_bonds']} bonds"),
         "rings": (tuple(f"ring_mol_ratio_{k}" for k in geometry.RING_SIZES) + ("macrocycle_mol_ratio", "ring_atom_ratio"),
                   lambda c: f"{c['n_mol_evaluated']} of {c['n_mol']} molecules evaluated, {c['n_rings']} rings"),
         "aromatic": (geometry.AROMATIC_RATIOS,
                      lambda c: f"{c['n_mol_evaluated']} of {c['n_mol']} molecules evaluated, {c['n_aromatic_cycles']} aromatic rings"),
         "valence": (geometry.VALENCE_RATIOS,
                     lambda c: f"{c['n_mol_evaluated']} of {c['n_mol']} molecules evaluated, {c['n_systems_failed']} of {c['n_systems']} "
                               f"aromatic systems without a Kekule structure")}


def load_reference_distributions(path):
    """``--distributions_reference``: {key: vector} from a ``.npz`` (np.savez(path, **{'6-6': v, ...})) or a ``torch.save``d dict"""
    if path.endswith(".npz"):
        with np.load(path) as f:
            return {k: np.asarray(f[k], np.float64) for k in f.files}
    raw = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(raw, dict):
        raise SystemExit(f"sample_cli: {path} does not hold a dict of reference distributions")
    return {k: np.asarray(v, np.float64) for k, v in raw.items()}


def load_reference_groups(path):
    """``--groups_reference``: {'ratio': ..., 'distribution': ...} from a ``.npz`` (np.savez(path, ratio=v25, distribution=v25)) or a
    ``torch.save``d dict whose two values are 25-vectors or {name: value} dicts"""
    if path.endswith(".npz"):
        with np.load(path) as f:
            raw = {k: np.asarray(f[k], np.float64) for k in f.files}
    else:
        raw = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(raw, dict) or not {"ratio", "distribution"} <= set(raw):
        raise SystemExit(f"sample_cli: {path} does not hold a dict with 'ratio' and 'distribution'")
    return {k: raw[k] for k in ("ratio", "distribution")}


def ranges(counts):
    """a per-graph count column [B] -> [(start, end)] per graph: rows (atoms, bonds, angles) are grouped by graph, in graph order"""
    ends = counts.to(torch.int64).cumsum(0).tolist()
    return list(zip([0] + ends[:-1], ends))


class SampleReports:
    """``requested``: names out of ORDER, EXTRA, LATE, ACROSS, AGAINST and 'sdf'; ``reference``: the path of --distributions_reference;
    ``groups_reference``: that of --groups_reference"""

    def __init__(self, requested, reference=None, groups_reference=None):
        self.requested = frozenset(requested)
        self.reference = reference
        self.groups_reference = groups_reference
        self.n_orders = 4 if "aromatic" in self.requested else 3        # --aromatic --distributions: types with the aromatic type
        self.seconds = {name: 0.0 for name in ORDER + EXTRA + LATE + ACROSS + AGAINST if name in self.requested}  # wall time of every report (``stats``)
        self.counts = {name: [] for name in _COUNT_REPORTS if name in self.requested}  # per-sample counts of this rank
        # the pockets' flat integer totals are added up as they come (one is 3.5 MB)
        self.distribution_totals = np.zeros(geometry.distribution_totals_length(n_orders=self.n_orders), np.int64)
        self.sdf_left_out, self.sdf_written = 0, 0
        self.interactions = []                                          # (graph_counts, graph_terms) of this rank's pockets
        self.groups = []                                                # graph_counts of this rank's pockets
        self.diversity = []                                             # group_counts rows of this rank's pockets
        self.native = []                                                # native_comparison dicts of this rank's pockets

    @classmethod
    def from_args(cls, args):
        return cls([name for name in ORDER + EXTRA + LATE + ACROSS + AGAINST + ("sdf",) if getattr(args, name, False)], args.distributions_reference,
                   getattr(args, "groups_reference", None))

    def refuse(self, dev, atom_mode):
        """what cannot run is refused before any model is built; ``atom_mode()``: the vocabulary the samples are decoded with"""
        for name in ("geometry", "bonds", "rings", "distributions", "aromatic", "valence") + EXTRA + LATE + ACROSS + AGAINST + ("sdf",):
            if name not in self.requested:
                continue
            if name == "aromatic" and atom_mode() != "add_aromatic":
                # on any device: the report starts from the aromatic atom types
                raise SystemExit(f"sample_cli: --aromatic starts from the model's aromatic flags: atom types of mode 'add_aromatic', "
                                 f"not {atom_mode()!r}")
            if dev.type != "cuda":
                raise SystemExit("sample_cli: " + _GPU_ONLY[name])
        if self.reference and "distributions" not in self.requested:
            raise SystemExit("sample_cli: --distributions_reference needs --distributions")
        if self.groups_reference and "groups" not in self.requested:
            raise SystemExit("sample_cli: --groups_reference needs --groups")

    # ---- GPU -----------------------------------------------------------------------------------------------------------------------------
    def evaluate(self, dev, state, batch, n_graphs, mode, group_ptr=None, native=None):
        """the requested reports of the state ``(x, c, bidx)`` the records hold, in the sampling frame (before ligand_translation), against
        the batch's own pocket -> {report: {name: CPU tensor}}; with --sdf or --aromatic and no --bonds also the ``bonds`` the host side
        slices by (not written).  ``group_ptr`` [P + 1]: the graphs group_ptr[p] ... group_ptr[p + 1] are the samples of the batch's pocket
        p; only the reports of ACROSS and AGAINST read it, and they need it.  ``native``: what ``native_state`` made of the pockets' own
        ligands; the native report needs it, and also returns ``native_reports``: the native ligands' rows of every other requested
        report, a dict like this one over P graphs"""
        if not self.requested:
            return {}
        if group_ptr is None and self.requested & set(ACROSS + AGAINST):
            raise ValueError("the diversity and native reports compare the samples of a pocket: evaluate needs group_ptr")
        if native is None and "native" in self.requested:
            raise ValueError("the native report compares with the pockets' own ligands: evaluate needs native")
        out = {}

        def reports_of(state, batch, n_graphs, group_ptr, against=None):
            """``get(name)`` of one state: every report is made once; ``against``: the ``get`` of the native ligands' state"""
            x, c, bidx = (t.to(dev) for t in state)
            info, made = {"num_graphs": n_graphs}, {}
            pocket = lambda: {k: batch[k].to(dev) for k in ("protein_pos", "protein_element", "protein_element_batch", "protein_aa_type",
                                                            "protein_atom_feature")}

            def get(name):
                if name not in made:
                    deps = {dep: get(dep) for dep in needs(name, mode)}
                    if name == "geometry":
                        rec = {k: batch[k].to(dev) for k in ("protein_pos", "protein_element", "protein_element_batch")}
                        made[name] = geometry.batch_geometry({**rec, **info}, x, c, bidx, mode)
                    elif name == "interactions":
                        made[name] = geometry.batch_interactions({**pocket(), **info}, x, c, bidx, mode, **deps)
                    elif name == "diversity":
                        made[name] = geometry.batch_diversity(info, x, c, bidx, mode, group_ptr, **deps)
                    elif name == "native":
                        theirs = {**native, **{dep: against(dep) for dep in needs(name, mode)}}
                        made[name] = geometry.batch_native({**pocket(), **info}, x, c, bidx, mode, group_ptr, theirs, **deps)
                    elif name == "distributions":
                        made[name] = geometry.batch_distributions(info, x, c, bidx, mode, aromatic=made.get("aromatic"), **deps)
                    else:
                        made[name] = getattr(geometry, "batch_" + name)(info, x, c, bidx, mode, **deps)
                return made[name]
            return get

        get_native = None
        if "native" in self.requested:
            n_pockets = len(group_ptr) - 1
            get_native = reports_of((native["x"], native["c"], native["lig_batch"]), native["batch"], n_pockets,
                                    list(range(n_pockets + 1)))
        get = reports_of(state, batch, n_graphs, group_ptr, get_native)
        for name in self.seconds:
            t0 = time.perf_counter()
            out[name] = {k: v.cpu() for k, v in get(name).items()}      # (the download waits for the launches)
            if name == "native":    # the native ligands' rows of every other requested report: what their records carry
                theirs = {other: {k: v.cpu() for k, v in get_native(other).items()} for other in self.seconds if other != "native"}
                if "bonds" not in theirs and "aromatic" in self.requested:
                    theirs["bonds"] = {k: get_native("bonds")[k].cpu() for k in ("bond_index", "bond_order", "graph_counts")}
                out["native_reports"] = theirs
            self.seconds[name] += time.perf_counter() - t0
        if "bonds" not in out and self.requested & {"aromatic", "sdf"}:
            out["bonds"] = {k: get("bonds")[k].cpu() for k in ("bond_index", "bond_order", "graph_counts")}
        return out

    @staticmethod
    def native_state(batch, group_ptr, ligands):
        """what ``evaluate`` takes as ``native``: the native ligands ``ligands`` ([(pos [n, 3], type indices [n])], one per pocket of the
        batch, in the frame the pockets came in) as a state of P graphs in the sampling frame -- float32(pos) minus the translation the
        graphs of the pocket carry in ``batch`` (``ligand_translation``; one fp32 subtraction per component) -- with the pocket copy of
        the pocket's first graph group_ptr[p]"""
        dev = batch["protein_pos"].device
        rec_b, bidx = batch["protein_element_batch"], batch["ligand_element_batch"]
        keys = ("protein_pos", "protein_element", "protein_aa_type", "protein_atom_feature")
        rows, xs, cs, lbs, pocket = [], [], [], [], {k: [] for k in keys}
        for p, (pos, typ) in enumerate(ligands):
            g = int(group_ptr[p])
            mine = (rec_b == g).nonzero().reshape(-1)
            own = (bidx == g).nonzero().reshape(-1)
            if own.numel():
                shift = batch["ligand_translation"][own[0]]
            elif mine.numel():
                shift = batch["protein_translation"][mine[0]]
            else:
                shift = torch.zeros(3, device=dev)
            xs.append(torch.as_tensor(np.asarray(pos, np.float32).reshape(-1, 3)).to(dev) - shift.to(torch.float32))
            cs.append(torch.as_tensor(np.asarray(typ, np.int64).reshape(-1)).to(dev))
            lbs.append(torch.full((cs[-1].shape[0],), p, dtype=torch.long, device=dev))
            rows.append(torch.full((mine.shape[0],), p, dtype=torch.long, device=dev))
            for k in keys:
                pocket[k].append(batch[k][mine])
        return {"x": torch.cat(xs), "c": torch.cat(cs), "lig_batch": torch.cat(lbs),
                "batch": {**{k: torch.cat(v) for k, v in pocket.items()}, "protein_element_batch": torch.cat(rows)}}

    # ---- host ----------------------------------------------------------------------------------------------------------------------------
    def annotate(self, samples, ev):
        """the per-sample fields of the requested reports, added to ``samples`` (one dict per graph of the batch, in graph order).  Atoms
        are sorted by graph, bonds by their first atom and angles by their centre: a graph's rows are ranges, and bond and angle rows
        become ligand-local"""
        if "geometry" in self.requested:
            geo = ev["geometry"]
            for g, (smp, (a0, a1)) in enumerate(zip(samples, ranges(geo["graph_counts"][:, 0]))):
                f = geo["flags"][a0:a1]
                smp["nr_bonds"] = geo["nr_bonds"][a0:a1].clone()
                smp["atom_stable"] = (f & geometry.STABLE) != 0
                smp["inter_clash"] = (f & geometry.INTER_CLASH) != 0
                smp["intra_clash_table_bonds"] = (f & geometry.INTRA_CLASH) != 0
                smp["mol_stable"] = bool(geo["graph_counts"][g, 2])
        if "bonds" in self.requested:
            bonds, gc = ev["bonds"], ev["bonds"]["graph_counts"]
            for g, (smp, (a0, a1), (b0, b1)) in enumerate(zip(samples, ranges(gc[:, 0]), ranges(gc[:, 1]))):
                smp["bond_index"] = bonds["bond_index"][:, b0:b1] - a0
                smp["bond_order"] = bonds["bond_order"][b0:b1].clone()
                smp["bond_length"] = bonds["bond_length"][b0:b1].clone()
                smp["fragment"] = bonds["fragment"][a0:a1].clone()
                smp["n_fragments"] = int(gc[g, 3])
                smp["connected"] = int(gc[g, 3]) == 1
        if "rings" in self.requested:
            gc = ev["rings"]["graph_counts"].to(torch.int64)
            for g, (smp, (a0, a1)) in enumerate(zip(samples, ranges(gc[:, 0]))):
                smp["ring_sizes"] = gc[g, 3:3 + len(geometry.RING_SIZES)].clone()
                smp["n_rings_larger"] = int(gc[g, -3])
                smp["atom_ring_min"] = ev["rings"]["atom_ring_min"][a0:a1].clone()
                smp["ring_status"] = int(gc[g, -1])
        if "aromatic" in self.requested:
            aro, gc, bgc = ev["aromatic"], ev["aromatic"]["graph_counts"], ev["bonds"]["graph_counts"]
            for g, (smp, (a0, a1), (b0, b1)) in enumerate(zip(samples, ranges(bgc[:, 0]), ranges(bgc[:, 1]))):
                smp["aromatic_atom"] = aro["aromatic_atom"][a0:a1].clone()
                smp["aromatic_bond"] = aro["aromatic_bond"][b0:b1].clone()
                smp["bond_type"] = aro["bond_type"][b0:b1].clone()
                smp["n_aromatic_rings"] = int(gc[g, 3])
                smp["aromatic_status"] = int(gc[g, 9])
        if "valence" in self.requested:
            val, gc = ev["valence"], ev["valence"]["graph_counts"].to(torch.int64)
            for g, (smp, (a0, a1), (b0, b1)) in enumerate(zip(samples, ranges(gc[:, 0]), ranges(gc[:, 1]))):
                row = dict(zip(geometry.VALENCE_GRAPH_COLUMNS, gc[g].tolist()))
                evaluated, el = row["status"] == 0, [row[f"el_{k}"] for k in range(8)]
                smp["implicit_h"] = val["implicit_h"][a0:a1].clone()
                smp["valence_flags"] = val["atom_flags"][a0:a1].clone()
                smp["bond_kekule"] = val["bond_kekule"][b0:b1].clone()
                smp["formula"] = geometry.formula(el, row["n_implicit_h"]) if evaluated else ""
                smp["mol_weight"] = geometry.mol_weight(el, row["n_implicit_h"]) if evaluated else float("nan")
                smp["n_nhoh"], smp["n_no"] = row["n_nhoh"], row["n_no"]
                smp["valence_ok"] = evaluated and row["valence_ok"] == 1
                smp["mol_valid"] = smp["valence_ok"] and row["n_fragments"] == 1
                smp["valence_status"] = row["status"]
        if "distributions" in self.requested:
            dists, gc = ev["distributions"], ev["distributions"]["graph_counts"]
            for g, (smp, (a0, a1), (n0, n1)) in enumerate(zip(samples, ranges(gc[:, 0]), ranges(gc[:, 2]))):
                smp["angle_index"] = dists["angle_index"][:, n0:n1] - a0
                smp["angle_cos"] = dists["angle_cos"][n0:n1].clone()
                smp["angle_deg"] = torch.from_numpy(np.degrees(np.arccos(smp["angle_cos"].numpy())))
                smp["angle_type"] = dists["angle_type"][n0:n1].clone()
                smp["distribution_status"] = int(gc[g, 4])
        if "interactions" in self.requested:
            ia, gc = ev["interactions"], ev["interactions"]["graph_counts"].to(torch.int64)
            inter, score = geometry.interaction_scores(gc, ia["graph_terms"])
            for g, (smp, (a0, a1), (b0, b1)) in enumerate(zip(samples, ranges(gc[:, 0]), ranges(gc[:, 1]))):
                row = dict(zip(geometry.INTERACTION_GRAPH_COLUMNS, gc[g].tolist()))
                smp["lig_xs_type"] = ia["lig_type"][a0:a1].clone()
                smp["atom_terms"] = ia["atom_terms"][a0:a1].clone()
                smp["bond_rotatable"] = ia["bond_rotatable"][b0:b1].clone()
                smp["interaction_terms"] = ia["graph_terms"][g].clone()
                smp["score_inter"], smp["score"] = float(inter[g]), float(score[g])
                for k in ("n_rotatable", "n_hbond_pairs", "n_hydrophobic_pairs", "n_close_pairs", "n_contact_atoms"):
                    smp[k] = row[k]
                smp["interactions_status"] = row["status"]
        if "groups" in self.requested:
            grp, gc = ev["groups"], ev["groups"]["graph_counts"].to(torch.int64)
            for g, (smp, (a0, a1)) in enumerate(zip(samples, ranges(gc[:, 0]))):
                smp["atom_group"] = grp["atom_group"][a0:a1].clone()
                smp["atom_class"] = grp["atom_class"][a0:a1].clone()
                smp["groups"] = geometry.group_names(smp["atom_group"], smp["atom_class"])
                smp["n_groups"] = int(gc[g, 2])
                smp["fg_counts"] = gc[g, 6:6 + geometry.GROUP_CLASSES + 1].clone()
                smp["groups_status"] = int(gc[g, -1])
        if "diversity" in self.requested:
            div = ev["diversity"]
            for g0, g1 in zip(div["group_ptr"][:-1].tolist(), div["group_ptr"][1:].tolist()):
                for g in range(g0, g1):             # the cross-sample fields are indices among the pocket's own samples
                    smp, micro = samples[g], int(div["nearest_micro"][g])
                    smp["fingerprint"] = div["fingerprint"][g].clone()
                    smp["mol_hash"] = geometry.mol_hash_int(div["mol_hash"][g])
                    smp["duplicate_of"] = int(div["first_same"][g])
                    smp["nearest_sample"] = int(div["nearest"][g])
                    smp["nearest_similarity"] = micro / geometry.SIMILARITY_ONE if micro >= 0 else float("nan")
                    smp["diversity_status"] = int(div["graph_counts"][g, -1])
        if "native" in self.requested:
            nat = ev["native"]
            micro, heavy = self._score_micro(nat["interaction_counts"], nat["interaction_terms"]), nat["contact_counts"][:, 1].tolist()
            theirs = self._score_micro(nat["native_interaction_counts"], nat["native_interaction_terms"])
            ptr = nat["group_ptr"].tolist()
            for p, (g0, g1) in enumerate(zip(ptr[:-1], ptr[1:])):
                for g in range(g0, g1):
                    smp, row = samples[g], dict(zip(geometry.NATIVE_SAMPLE_COLUMNS, nat["sample_counts"][g].tolist()))
                    both = micro[g] is not None and theirs[p] is not None
                    smp["native_similarity"] = row["sim_micro"] / geometry.SIMILARITY_ONE if row["sim_micro"] >= 0 else float("nan")
                    smp["native_same_hash"] = row["same_hash"] == 1 if row["same_hash"] >= 0 else None
                    smp["native_contact_jaccard"] = (row["contact_micro"] / geometry.SIMILARITY_ONE if row["contact_micro"] >= 0
                                                     else float("nan"))
                    smp["native_contact_common"], smp["native_contact_union"] = row["contact_common"], row["contact_union"]
                    smp["native_centroid_distance"] = float(np.sqrt(float(nat["centroid_d2"][g])))
                    smp["score_minus_native"] = (micro[g] - theirs[p]) / 1e6 if both else float("nan")
                    smp["better_than_native"] = micro[g] < theirs[p] if both else None
                    smp["ligand_efficiency"] = micro[g] / 1e6 / heavy[g] if micro[g] is not None and heavy[g] > 0 else float("nan")
                    smp["native_status"] = row["status"]

    @staticmethod
    def _score_micro(graph_counts, graph_terms):
        """per graph the score as whole millionths (``geometry.score_micro``), None where the interaction report did not evaluate it"""
        _, score = geometry.interaction_scores(graph_counts.to(torch.int64), graph_terms)
        return [None if np.isnan(v) else geometry.score_micro(v) for v in score]

    def annotate_native(self, records, ev):
        """the native ligands' records (``records``: one dict per pocket of the batch, as ``samples`` are per graph) with the fields of
        every other requested report -- the same functions on the same atoms give what the ligand would get as a sample -- plus
        ``score``, ``score_micro`` (None where not evaluated) and ``n_contact_atoms`` as the interaction report defines them, and
        ``n_pocket_contact_atoms``: the heavy pocket atoms it touches, what ``native_contact_union`` of a sample is counted against"""
        SampleReports(self.requested - {"native", "sdf"}).annotate(records, ev["native_reports"])
        nat = ev["native"]
        micro = self._score_micro(nat["native_interaction_counts"], nat["native_interaction_terms"])
        _, score = geometry.interaction_scores(nat["native_interaction_counts"].to(torch.int64), nat["native_interaction_terms"])
        for p, rec in enumerate(records):
            rec["score"] = float(score[p])
            rec["score_micro"] = micro[p]
            rec["n_contact_atoms"] = int(nat["native_interaction_counts"][p, geometry.INTERACTION_GRAPH_COLUMNS.index("n_contact_atoms")])
            rec["n_pocket_contact_atoms"] = int(nat["native_contact_counts"][p, 3])
        return records

    def pocket_counts(self, ev, g0, g1):
        """the dicts of counts a pocket record carries for its graphs g0 ... g1 - 1, which join the job's totals"""
        rec = {}
        if "distributions" in self.requested:
            totals = geometry.distribution_totals(ev["distributions"], graphs=(g0, g1), n_orders=self.n_orders)
            self.distribution_totals += totals
            rec["distributions"] = geometry.distribution_counts(totals, n_orders=self.n_orders)
        for rep in reversed(geometry.COUNT_REPORTS):
            if rep.name in self.requested:
                gc = ev[rep.name]["graph_counts"][g0:g1].to(torch.int64)
                self.counts[rep.name].append(gc)
                rec[rep.name] = rep.summarise_totals(rep.totals(gc))["counts"]
        if "interactions" in self.requested:
            gc, terms = ev["interactions"]["graph_counts"][g0:g1].to(torch.int64), ev["interactions"]["graph_terms"][g0:g1]
            self.interactions.append((gc, terms))
            rec["interactions"] = geometry.summarise_interactions(gc, terms)["counts"]
        if "groups" in self.requested:
            gc = ev["groups"]["graph_counts"][g0:g1].to(torch.int64)
            self.groups.append(gc)
            rec["groups"] = geometry.summarise_groups(gc)["counts"]
        if "diversity" in self.requested:
            div = ev["diversity"]
            ptr = div["group_ptr"].tolist()
            found = [p for p in range(len(ptr) - 1) if (ptr[p], ptr[p + 1]) == (g0, g1)]
            if not found:
                raise ValueError(f"the graphs {g0} ... {g1} are no group of the group_ptr the diversity report was evaluated with")
            p = found[0]
            row = div["group_counts"][p]
            self.diversity.append(row.clone())
            q0, q1 = int(div["pair_ptr"][p]), int(div["pair_ptr"][p + 1])
            rec["similarity_micro"] = geometry.similarity_matrix(div["pair_sim"][q0:q1], (div["graph_counts"][g0:g1, -1] == 0).tolist())
            rec["diversity"] = geometry.diversity_counts(row)
        if "native" in self.requested:
            nat = ev["native"]
            ptr = nat["group_ptr"].tolist()
            found = [p for p in range(len(ptr) - 1) if (ptr[p], ptr[p + 1]) == (g0, g1)]
            if not found:
                raise ValueError(f"the graphs {g0} ... {g1} are no group of the group_ptr the native report was evaluated with")
            p = found[0]
            micro = self._score_micro(nat["interaction_counts"][g0:g1], nat["interaction_terms"][g0:g1])
            theirs = self._score_micro(nat["native_interaction_counts"][p:p + 1], nat["native_interaction_terms"][p:p + 1])[0]
            metrics = geometry.native_pocket_metrics(micro, nat["contact_counts"][g0:g1, 1].tolist(), theirs)
            rec["native_comparison"] = geometry.native_pocket_counts(nat["group_counts"][p], metrics)
            self.native.append(rec["native_comparison"])
        return rec

    def pocket_files(self, stem, samples, ev, g0):
        """(file name, text) of what is written beside a pocket's record ``stem``.pt: with --sdf one V2000 record per sample of the pocket
        (``samples``: its records, graphs g0 ... of the batch), bond types: the Kekule orders of --valence where that report evaluated the
        sample (no type 4 but on a system without a Kekule structure), else from --aromatic where that report did, else the table-bond orders; a sample ``sdf_record`` refuses is left out and counted"""
        if "sdf" not in self.requested:
            return []
        bonds, gc = ev["bonds"], ev["bonds"]["graph_counts"]
        atoms, rows, records = ranges(gc[:, 0]), ranges(gc[:, 1]), []
        for j, smp in enumerate(samples):
            (a0, _), (b0, b1) = atoms[g0 + j], rows[g0 + j]
            evaluated = "aromatic" in self.requested and int(ev["aromatic"]["graph_counts"][g0 + j, 9]) == 0
            types = ev["aromatic"]["bond_type"][b0:b1] if evaluated else bonds["bond_order"][b0:b1]
            if "valence" in self.requested and int(ev["valence"]["graph_counts"][g0 + j, -1]) == 0:
                types = ev["valence"]["bond_kekule"][b0:b1]
            try:
                records.append(geometry.sdf_record(f"{stem}_sample_{j}", smp["pos"], smp["atom"], bonds["bond_index"][:, b0:b1] - a0, types))
                self.sdf_written += 1
            except ValueError:
                self.sdf_left_out += 1
        return [(stem + ".sdf", "".join(records))]

    # ---- the job -------------------------------------------------------------------------------------------------------------------------
    def finish(self, out_dir, rank, dev):
        """integer totals of all ranks, summed: the job's numbers do not depend on how the pockets were sharded.  Rank 0 writes
        {out_dir}/<report>_summary.json and prints the report's line"""
        def save(name, summary):
            with open(os.path.join(out_dir, name + "_summary.json"), "w") as f:
                json.dump(summary, f, indent=1, sort_keys=True)

        for name in ("geometry", "bonds", "rings", "distributions", "aromatic", "valence"):
            if name not in self.requested:
                continue
            if name == "distributions":
                self._finish_distributions(save, rank, dev)
                continue
            rep, (ratios, tail) = _COUNT_REPORTS[name], _LINE[name]
            totals = rep.totals(torch.cat(self.counts[name]) if self.counts[name] else torch.zeros(0, len(rep.graph_columns)))
            summary = rep.summarise_totals(sharding.sum_counts(totals, device=dev))
            if rank == 0:
                save(name, summary)
                print(f"{name}: " + ", ".join(f"{k} {summary[k]:.4f}" for k in ratios) + f" ({tail(summary['counts'])})")
        if "interactions" in self.requested:
            totals = [0] * len(geometry.INTERACTION_COUNT_KEYS)
            for gc, terms in self.interactions:      # integer totals: pocket by pocket is the whole
                totals = [a + b for a, b in zip(totals, geometry.interaction_totals(gc, terms))]
            summary = geometry.summarise_interaction_totals(sharding.sum_counts(totals, device=dev))
            if rank == 0:
                save("interactions", summary)
                cnt = summary["counts"]
                print("interactions: " + ", ".join(f"{k} {summary[k]:.4f}" for k in geometry.INTERACTION_RATIOS)
                      + f" ({cnt['n_mol_evaluated']} of {cnt['n_mol']} molecules evaluated, n_mol_over_limit {cnt['n_mol_over_limit']}; a score "
                        f"in Vina's functional form, not the Vina program)")
        if "groups" in self.requested:
            totals = [0] * len(geometry.GROUP_COUNT_KEYS)
            for gc in self.groups:                   # integer totals: pocket by pocket is the whole
                totals = [a + b for a, b in zip(totals, geometry.group_totals(gc))]
            summary = geometry.summarise_group_totals(sharding.sum_counts(totals, device=dev))
            if rank == 0:
                if self.groups_reference:
                    summary.update(geometry.groups_against(summary, load_reference_groups(self.groups_reference)))
                save("groups", summary)
                cnt = summary["counts"]
                top = sorted(range(geometry.GROUP_CLASSES), key=lambda k: (-cnt[f"n_fg_{k}"], k))[:3]
                print("groups: " + ", ".join(f"{k} {summary[k]:.4f}" for k in geometry.GROUP_RATIOS)
                      + "; most frequent: " + ", ".join(f"{geometry.GROUP_NAMES[k]} {cnt[f'n_fg_{k}']}" for k in top)
                      + f" ({cnt['n_mol_evaluated']} of {cnt['n_mol']} molecules evaluated, n_mol_over_limit {cnt['n_mol_over_limit']}; "
                        f"marking rules of this library's own, not the EFGs program)")
        if "diversity" in self.requested:
            totals = geometry.diversity_totals(torch.stack(self.diversity) if self.diversity else np.zeros((0, 7), np.int64))
            summary = geometry.summarise_diversity_totals(sharding.sum_counts(totals, device=dev))
            if rank == 0:
                save("diversity", summary)
                cnt = summary["counts"]
                print("diversity: " + ", ".join(f"{k} {summary[k]:.4f}" for k in geometry.DIVERSITY_RATIOS)
                      + f" ({cnt['n_mol_evaluated']} of {cnt['n_mol']} molecules evaluated in {cnt['n_pockets']} pockets, n_mol_over_limit "
                        f"{cnt['n_mol_over_limit']}; uniqueness per pocket by a hash of colour refinement, not an isomorphism test; a "
                        f"fingerprint of this library's own, not RDKit's)")
        if "native" in self.requested:
            summary = geometry.summarise_native_totals(sharding.sum_counts(geometry.native_totals(self.native), device=dev))
            if rank == 0:
                save("native", summary)
                cnt = summary["counts"]
                print("native: " + ", ".join(f"{k} {summary[k]:.4f}" for k in geometry.NATIVE_RATIOS)
                      + f" ({cnt['n_pockets_evaluated']} of {cnt['n_pockets']} pockets evaluated, n_pockets_positive_native "
                        f"{cnt['n_pockets_positive_native']}, n_pockets_native_not_evaluated {cnt['n_pockets_native_not_evaluated']}, "
                        f"n_pockets_no_sample {cnt['n_pockets_no_sample']}; the reference's MPBG / IMP / LBE formulas on a score in Vina's "
                        f"functional form, not the Vina program; a fingerprint of this library's own, not RDKit's)")
        if "sdf" in self.requested:
            left_out, written = sharding.sum_counts([self.sdf_left_out, self.sdf_written], device=dev)
            if rank == 0:
                print(f"sdf: {written} records written, {left_out} samples left out (above 999 atoms or bonds, or an element outside "
                      f"H C N O F P S Cl)")

    def _finish_distributions(self, save, rank, dev):
        summary = geometry.summarise_distribution_totals(sharding.sum_counts(self.distribution_totals.tolist(), device=dev),
                                                         n_orders=self.n_orders)
        if rank != 0:
            return
        if self.reference:
            summary.update(geometry.jsd_against(summary, load_reference_distributions(self.reference), n_orders=self.n_orders))
        save("distributions", summary)
        cnt, all_12a = summary["counts"], summary["pair_length"]["All_12A"]
        edges = geometry.default_pair_edges()[0]
        mode_bin = int(np.argmax(all_12a["distribution"])) if all_12a["count"] else -1
        # bin b > 0 holds edges[b - 1] < d <= edges[b]; bin 0 the distances that are exactly edges[0]
        centre = float("nan") if mode_bin < 0 else float(edges[0] if mode_bin == 0 else 0.5 * (edges[mode_bin - 1] + edges[mode_bin]))
        print(f"distributions: {cnt['n_mol']} molecules, {cnt['n_bonds']} bonds, {cnt['n_angles']} angles, "
              f"All_12A modal bin centre {centre:.3f} A, n_mol_over_limit {cnt['n_mol_over_limit']}")
