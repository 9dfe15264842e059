"""Reference-made DiffBP training fixtures with ligands of more than 48 atoms, where the reference's ``interior_loss`` restricts every
protein atom to its 48 nearest ligand atoms (``torch_cluster.knn(..., k=48)``, diffbp.py:18-28).  The generators, the reference
loader and the output format are those of ``oracle/make_golden.py``; this file only adds two cases.

    python scripts/make_golden_large_ligands.py        # writes tests/golden/train_loss_diffbp_big{,_ctx}.npz

Needs the reference checkout, like ``python -m oracle.make_golden``."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.argv = sys.argv[:1]      # oracle.make_golden reads its case filter from the command line: none here

from oracle import make_golden as MG  # noqa: E402

CASES = {
    # graphs of 60 / 12 / 52 ligand atoms: two of the three are restricted
    "train_loss_diffbp_big": lambda: (MG.small_batch([(64, 60), (50, 12), (57, 52)], seed=83), 31),
    # 75 / 49 / 20 atoms with 20 / 0 / 6 context atoms, interleaved with the generated ones
    "train_loss_diffbp_big_ctx": lambda: (MG.sidechain_order(MG.small_batch([(70, 75), (60, 49), (48, 20)], seed=84, ctx=[20, 0, 6]),
                                                             seed=5), 32),
}


def main():
    for name, make in CASES.items():
        batch, seed = make()
        MG.diffbp_train_case(name, batch, seed=seed)


if __name__ == "__main__":
    main()
