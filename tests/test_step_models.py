"""CPU side of tests/test_gpu_step_kernels.py: the cases and references of tests/step_models.py are sound on their own.

* the case grid covers what it claims, the layout is what the GPU tests rely on;
* the restated TargetDiff score wrapper is oracle.targetdiff.type_backward (every case, both dtypes) and reproduces the recorded
  c_next of the three teacher-forced reference steps;
* on every case the GPU file uses, the share of contested rows computed from the fp32 and fp64 references alone stays under the 1 %
  cap and the fp32 oracle's discrete outcomes equal the fp64 ones on every other row -- so a change of seed cannot silently make
  the GPU comparison vacuous;
* DiffSBDD.step_tables(), the host-side fp32 coefficients fed to cbgx_diffsbdd_step, against fp64;
* the empty-graph convention (a zero mean) that include/cbgx.h promises."""
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import diffbp as OB
from oracle import diffsbdd as OS
from oracle import targetdiff as OT
from tests import step_models as SM

F32, F64 = torch.float32, torch.float64


def test_targetdiff_grid_is_pairwise_covering():
    grid = SM.targetdiff_grid()
    axes = (SM.TD_C, SM.TD_STEPS, SM.TD_SCALES, SM.TD_NLIG)
    for i, j in itertools.combinations(range(4), 2):
        assert {(p[i], p[j]) for p in grid} == set(itertools.product(axes[i], axes[j])), (i, j)
    assert SM.TD_C == (1, 3, 4, 5, 8, 13, 32) and SM.TD_STEPS == (0, 1, 500, 999) and SM.TD_NLIG == (1, 255, 256, 257)
    assert SM.TD_SCALES == (3.0, 150.0) and SM.TD_HAND in {(p[0], p[1]) for p in grid}


def _all_layout_cases():
    yield from SM.targetdiff_cases()
    yield SM.diffbp_case(13, 0, 1000, 1)
    yield SM.diffbp_case(13, 12, 4, 2, SM.SIZES_B)
    yield SM.diffsbdd_case(8, 1, SM.SIZES_A, True, 1, 1)
    yield SM.diffsbdd_case(5, 0, SM.SIZES_B, False, 1, 1)


def test_layout_of_the_cases():
    """lig_rows injective, inside its graph's rows, not monotone; ligand and pocket rows interleaved; gen mixed; sizes within the
    budget of a quick test; denoiser outputs NaN off the ligand rows"""
    for d in _all_layout_cases():
        rows, n, N = d["lig_rows"].long(), d["n_lig"], d["N"]
        assert N > n and n <= 1300 and N <= 3000 and rows.shape[0] == n
        assert rows.unique().shape[0] == n and int(rows.min()) >= 0 and int(rows.max()) < N
        gp, lp = d["graph_ptr"].long(), d["lig_ptr"].long()
        assert int(lp[-1]) == n and int(gp[-1]) == N
        for g in range(d["B"]):
            r = rows[lp[g]:lp[g + 1]]
            assert bool(((r >= gp[g]) & (r < gp[g + 1])).all())
        assert torch.equal(d["lig_flag"].bool().nonzero().flatten(), rows.sort().values)
        if n >= 8:
            assert bool((rows[1:] < rows[:-1]).any()) and bool((rows[1:] > rows[:-1]).any())
            flag = d["lig_flag"].bool()
            assert int((flag[1:] != flag[:-1]).sum()) > 4
            assert 0 < int(d["gen"].sum()) < n
        off = torch.ones(N, dtype=torch.bool)
        off[rows] = False
        for k in ("x_den", "logits", "x_in", "x_com"):
            if k in d:
                assert bool(torch.isnan(d[k][off]).all()) and bool(torch.isfinite(d[k][rows]).all()), (d["name"], k)
    assert list(SM.SIZES_A) == [0, 1, 63, 64, 65, 128, 129, 200, 0, 7] and SM.SIZES_B[-1] == 0
    d = SM.diffsbdd_case(8, 1, SM.SIZES_A, False, 1, 1)
    assert 0 in [p for s, p in zip(d["lig_sizes"], d["pocket_sizes"]) if s > 0] and max(d["pocket_sizes"]) <= 40


def test_score_wrapper_is_type_backward_on_every_case():
    pos, typ = SM.targetdiff_tables()
    for d in SM.targetdiff_cases():
        rows, gen = d["lig_rows"].long(), d["gen"].bool()
        t = torch.full((d["B"],), d["t"], dtype=torch.long)
        for dt in (F32, F64):
            tb = {k: v.to(dt) for k, v in typ.items()}
            args = (tb, d["C"], d["logits"][rows].to(dt), d["c_lig"].to(dt), t, d["bl"], gen, d["u"].to(dt))
            c0, v0 = OT.type_backward(*args)
            c1, v1, score = SM.targetdiff_type_scores(*args)
            assert torch.equal(v0, v1) and torch.equal(c0, c1), (d["name"], dt)
            assert bool(torch.isfinite(score).all()), (d["name"], dt)
            ref = SM.targetdiff_reference(d, dt)
            assert torch.equal(ref["v_next"], v0) and ref["x_next"].dtype == dt and ref["score"].dtype == dt


@pytest.mark.parametrize("case", ["step_t500", "step_t0", "step_t999_linker"])
def test_score_wrapper_reproduces_the_reference_steps(golden_dir, synthetic_sd, case):
    """the golden's eps / u and the oracle's network output into the wrapper: the recorded c_next, exactly"""
    z = np.load(os.path.join(golden_dir, case + ".npz"))
    g = {k: torch.from_numpy(z[k]) if z[k].ndim else z[k].item() for k in z.files}
    batch = {k[len("batch_"):]: v for k, v in g.items() if k.startswith("batch_")}
    c_lig = torch.nn.functional.one_hot(batch["ligand_atom_type"], 13).float()
    _, _, _, c_pred = OT.denoise_step(synthetic_sd, batch, batch["ligand_pos"], c_lig, int(g["t_idx"]), g["eps"], g["u"], 13,
                                      return_net_out=True)
    bl = batch["ligand_element_batch"]
    gen = batch.get("ligand_gen_flag", torch.ones(c_lig.shape[0], dtype=torch.bool))
    t = torch.full((int(bl.max()) + 1,), int(g["t_idx"]), dtype=torch.long)
    _, typ = OT.tables_from_state_dict(synthetic_sd)
    c_next, v_next, _ = SM.targetdiff_type_scores(typ, 13, c_pred, c_lig, t, bl, gen, g["u"])
    assert torch.equal(c_next, g["c_next"]) and torch.equal(v_next, g["c_next"].argmax(-1))


def test_targetdiff_contested_share_and_fp32_agreement():
    worst = 0.0
    for d in SM.targetdiff_cases():
        r32, r64 = SM.targetdiff_reference(d, F32), SM.targetdiff_reference(d, F64)
        gen = d["gen"].bool()
        con, err = SM.contested_rows(r32["score"], r64["score"], gen, d["tie_rows"])
        share = SM.contested_share(con, gen)
        worst = max(worst, share)
        print(f"{d['name']}: fp32 score error {err:.2e}, contested {100 * share:.2f} %")
        assert share <= SM.CONTEST_CAP, d["name"]
        assert torch.equal(r32["v_next"][~con], r64["v_next"][~con]), d["name"]
        for k, win in d["tie_rows"].items():          # the exact ties: the lower class, in both precisions
            want = win if gen[k] else int(d["c_lig"][k].argmax())
            assert int(r32["v_next"][k]) == int(r64["v_next"][k]) == want
            assert float(r64["score"][k, 2]) == float(r64["score"][k, 5]) == float(r64["score"][k].max())
        for k in d["current_rows"]:                   # the current type wins on flat logits and equal u
            assert int(r64["v_next"][k]) == int(d["c_lig"][k].argmax()) == 4
        assert torch.equal(r64["x_next"][~gen].float(), d["x_lig"][~gen]) and torch.equal(r64["c_next"][~gen].float(), d["c_lig"][~gen])
    print(f"largest contested share {100 * worst:.2f} %")
    hand = [d for d in SM.targetdiff_cases() if d["tie_rows"]]
    assert len(hand) == 1 and len(hand[0]["tie_rows"]) == 2 and len(hand[0]["current_rows"]) == 2
    u = hand[0]["u"]
    assert bool((u[-8:-6] == 0).all()) and bool((u[-6:-4] == SM.U_MAX).all()) and hand[0]["gen"][-8:].tolist() == [1, 0] * 4


def _diffbp_cases():
    for C in SM.BP_C:
        for absorbing in (0, C - 1):
            yield from SM.diffbp_cases(C, absorbing)


def test_diffbp_contested_share_and_fp32_agreement():
    for d in _diffbp_cases():
        r32, r64 = SM.diffbp_reference(d, F32), SM.diffbp_reference(d, F64)
        decided = SM.diffbp_decided(d)
        con, err = SM.contested_rows(r32["score"], r64["score"], decided, d["tie_rows"])
        assert err == 0.0 and SM.contested_share(con, decided) <= SM.CONTEST_CAP, d["name"]
        assert torch.equal(r32["v_next"][~con], r64["v_next"][~con]), d["name"]
        cur, gen, u = d["c_lig"].argmax(-1), d["gen"].bool(), d["u"]
        assert bool(((u - d["prob"]).abs() >= SM.U_MARGIN).all()) or (d["T"], d["t"]) == (4, 2)
        # every kind of row is present: absorbing or not, generated or context, changing or not; and some tie row does change
        for a in (True, False):
            for b in (True, False):
                assert bool(((cur == d["absorbing"]) == a)[gen == b].any()), d["name"]
        assert bool(decided.any()) and (d["prob"] == 1.0 or bool((~decided & gen & (cur == d["absorbing"])).any())), d["name"]
        two = d["c_lig"][d["double_rows"]]
        assert len(d["double_rows"]) > 1 and bool((two.sum(-1) == 2).all()) and bool((two[:, d["absorbing"]] == 1).all()) and bool(gen[d["double_rows"]].all())
        ties = [k for k in d["tie_rows"] if decided[k]]
        assert ties, d["name"]
        for k in ties:
            assert int(r64["v_next"][k]) == int(r32["v_next"][k]) == d["tie_rows"][k]
        assert torch.equal(r64["v_next"][~decided], cur[~decided])
        if (d["T"], d["t"]) == (4, 2):
            elig = gen & (cur == d["absorbing"])
            half, below = elig & (u == 0.5), elig & (u == SM.U_BELOW_HALF)
            assert bool(half.any()) and bool(below.any())
            assert torch.equal(r64["v_next"][half], cur[half])
            assert torch.equal(r64["v_next"][below], d["logits"][d["lig_rows"].long()][below].argmax(-1))


@pytest.mark.parametrize("T", [5, 20, 1000])
def test_diffsbdd_step_tables_against_fp64(T):
    """every k of 1 / alpha_ts, sigma2_ts / alpha_ts / sigma_t, sigma_ts sigma_s / sigma_t: finite, and within 8 x the fp32 oracle's
    own error + 2e-6 of the table's magnitude of the same expressions in fp64 (the yardstick of tests/test_gpu_range.py)"""
    tabs = SM.diffsbdd_step_tables(T)
    c32, c64 = SM.diffsbdd_coefficients(T, F32), SM.diffsbdd_coefficients(T, F64)
    for name, tab, r32, r64 in zip(("1/alpha_ts", "coef", "sigma"), tabs, c32, c64):
        assert len(tab) == T and all(isinstance(v, float) for v in tab)
        got = torch.tensor(tab, dtype=F64)
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(r64).all()), name
        assert torch.equal(got.float().double(), got), name           # fp32 values: what the C ABI's float arguments carry
        scale = float(r64.abs().max())
        e_tab, e_32 = float((got - r64).abs().max()), float((r32.double() - r64).abs().max())
        print(f"T={T} {name}: magnitude {scale:.3g}, step_tables err {e_tab:.2e}, fp32 oracle err {e_32:.2e}")
        assert e_tab <= 8 * e_32 + 2e-6 * scale, (name, e_tab, e_32)
        assert float(r64.min()) >= 0.0 and float(got.min()) >= 0.0, name
    assert float(c64[0].min()) >= 1.0


def test_empty_graphs_have_a_zero_mean():
    """scatter_mean divides by clamp(count, min=1): an empty graph's mean is 0 -- the max(a1 - a0, 1) of the kernels, and what
    include/cbgx.h states for shift / frame_shift of a ligand-free graph"""
    src, idx = torch.tensor([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]], dtype=F64), torch.tensor([1, 1])
    for f in (OB.scatter_mean, OS.scatter_mean):
        m = f(src, idx, 4)
        assert torch.equal(m, torch.tensor([[0.0] * 3, [2.0] * 3, [0.0] * 3, [0.0] * 3], dtype=F64))
    d = SM.diffsbdd_case(8, 1, SM.SIZES_A, True, 1, 1)
    r = SM.diffsbdd_reference(d, F64)
    empty = [g for g, s in enumerate(d["lig_sizes"]) if s == 0]
    assert empty == [0, 8] and bool((r["shift"][empty] == 0).all())
    assert torch.equal(r["frame"][empty], d["frame0"][empty].double())
    assert bool((r["shift"][[2, 5]] != 0).all())
    b = SM.diffbp_reference(SM.diffbp_case(13, 0, 1000, 1, SM.SIZES_B), F64)
    assert bool(torch.isfinite(b["x_next"]).all())


def test_diffsbdd_reference_modes():
    """update_positions = 0 / update_types = 0 leave the state alone, and only then"""
    for do_x, do_c in itertools.product((0, 1), (0, 1)):
        d = SM.diffsbdd_case(8, 999, SM.SIZES_B, True, do_x, do_c)
        r = SM.diffsbdd_reference(d, F64)
        assert torch.equal(r["x_next"].float(), d["x_lig"]) == (not do_x)
        assert torch.equal(r["c_next"].float(), d["c_lig"]) == (not do_c)
        assert bool(torch.isfinite(r["h"]).all()) and r["h"].shape == (d["n_lig"], SM.H)
