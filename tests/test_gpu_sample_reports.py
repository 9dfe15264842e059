"""The reports of sample_cli compose: a report is what it is whichever other reports run beside it, and whoever supplies its bond list and
its ring report.  Three runs of the T = 20 fixture config on two synthetic pockets x two samples (--noise counter, one saved random
checkpoint, --streams 1, one pocket per batch: two batches): A with every report, B with --aromatic --distributions --sdf (bonds and rings
made on the fly and not written), C with --geometry --bonds --rings.  Every comparison is ``==`` / ``torch.equal``: the kernels are
deterministic."""
import os

import pytest
import torch

import cbgbench_amd as C
from cbgbench_amd import geometry as G
from tests.test_gpu_aromatic import BOND_FIELDS, RING_FIELDS
from tests.test_gpu_rings import _records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARIES = ("geometry", "bonds", "rings", "aromatic", "distributions")


def _same(a, b):
    """equal values, dtypes and shapes; nan (the cosine of a degenerate angle) equals nan"""
    if not torch.is_tensor(a):
        return type(a) is type(b) and a == b
    if not torch.is_tensor(b) or a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())
    return torch.equal(a, b)


def _files(d, suffix):
    out = {}
    for name in sorted(os.listdir(d)):
        if name.endswith(suffix):
            with open(os.path.join(d, name), "rb") as f:
                out[name] = f.read()
    return out


def test_sample_cli_reports_compose(tmp_path, monkeypatch):
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    config, _ = C.load_config(cfg)
    C.set_num_atom_type(config)
    torch.manual_seed(123)
    ckpt = tmp_path / "random_init.pt"
    torch.save({"model": C.get_model(config.model).state_dict()}, ckpt)
    common = ["--config", cfg, "--synthetic", "2", "--num_samples", "2", "--checkpoint", str(ckpt), "--seed", "2024", "--noise", "counter",
              "--no_translate", "--pockets_per_batch", "1", "--streams", "1"]
    n_batches = 2
    calls = {"ligand_bonds": 0, "ligand_rings": 0}

    def counted(name):
        inner = getattr(G, name)

        def wrapper(*args, **kwargs):
            calls[name] += 1
            return inner(*args, **kwargs)
        return wrapper

    def go(tag, *flags):
        out = tmp_path / tag
        assert sample_cli.main(common + ["--out_root", str(out)] + list(flags)) == 0
        d = str(out / "targetdiff_T20")
        return d, _records(d)

    with monkeypatch.context() as m:
        for name in calls:
            m.setattr(G, name, counted(name))
        dir_a, rec_a = go("a", "--geometry", "--bonds", "--rings", "--aromatic", "--distributions", "--sdf")
    calls_a = dict(calls)
    dir_b, rec_b = go("b", "--aromatic", "--distributions", "--sdf")
    dir_c, rec_c = go("c", "--geometry", "--bonds", "--rings")

    for other, want_pocket in ((rec_b, {"aromatic", "distributions"}), (rec_c, {"geometry", "bonds", "rings"})):
        for ra, ro in zip(rec_a, other):
            assert set(ro) - {"pocket_index", "samples"} == want_pocket and set(ro) <= set(ra)
            for k in ro:
                if k != "samples":
                    assert ra[k] == ro[k], k
            assert len(ra["samples"]) == len(ro["samples"]) == 2
            for sa, so in zip(ra["samples"], ro["samples"]):
                assert set(so) <= set(sa)
                for k in so:
                    assert _same(sa[k], so[k]), k
    # B made its bonds and rings on the fly: none of either is written
    for rb in rec_b:
        for sb in rb["samples"]:
            assert not set(sb) & set(BOND_FIELDS + RING_FIELDS)
    # (and the shared fields above are not vacuous)
    assert {"aromatic_bond", "bond_type", "angle_index", "angle_type"} <= set(rec_b[0]["samples"][0])
    assert set(BOND_FIELDS + RING_FIELDS) | {"nr_bonds", "mol_stable"} <= set(rec_c[0]["samples"][0])

    sdf_a, sdf_b = _files(dir_a, ".sdf"), _files(dir_b, ".sdf")
    assert sorted(sdf_a) == [f"pocket_{i:05d}.sdf" for i in range(2)] and sdf_a == sdf_b and not _files(dir_c, ".sdf")
    json_a, json_b, json_c = (_files(d, "_summary.json") for d in (dir_a, dir_b, dir_c))
    assert sorted(json_a) == sorted(f"{k}_summary.json" for k in SUMMARIES)
    assert sorted(json_b) == ["aromatic_summary.json", "distributions_summary.json"]
    assert sorted(json_c) == ["bonds_summary.json", "geometry_summary.json", "rings_summary.json"]
    for other in (json_b, json_c):
        for name, data in other.items():
            assert data == json_a[name], name

    # with every report asked for, the bond list and the ring report are made once per batch and shared
    print("calls in run A:", calls_a, "batches:", n_batches)
    assert calls_a == {"ligand_bonds": n_batches, "ligand_rings": n_batches}
