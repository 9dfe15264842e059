"""The step kernels of csrc/step.hip in isolation, through the C ABI, against the oracle's own step functions evaluated in fp64
(tests/step_models.py; no denoiser in the loop, made-up denoiser outputs): step_prologue_kernel, step_epilogue_kernel,
step_boundary_kernel, diffbp_epilogue_kernel, diffsbdd_step_kernel at the shapes and inputs the samplers never produce -- ligands
over one wave trip, empty graphs, the 256-thread block edge, 1 .. 32 classes, saturated logits, u at 0 and at 1 - 2^-24, exact ties,
u == prob, a non-NULL shift, update_positions / update_types = 0, a non-zero starting frame_shift, absorbing_state != 0.

Continuous outputs: the fp32-grade yardstick of tests/test_gpu_range.py (error against fp64 <= 8 x the fp32 oracle's own + 2e-6 of
the magnitude, and inside 1e-4 of it).  Discrete outcomes: equal to fp64 on every row that is not contested (a fp64 margin below
16 x the fp32 oracle's largest score error on the case), contested rows at most 1 % of a case.  Everything the kernels must not
touch, copy through or compute exactly is compared on the bits.  The worst figures of every test go to step_kernel_errors.md in the
run-output directory, beside the tables of tests/test_gpu_range.py and tests/test_gpu_parity.py."""
import ctypes
import os
import re

import pytest
import torch

from cbgbench_amd import _native
from tests import step_models as SM
from tests.test_gpu_range import assert_fp32_grade

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
REPORT = []        # (what, magnitude, kernel err / magnitude, fp32 oracle err / magnitude)
SHARES = []        # (what, generated rows, contested share, fp32 score error)
NAN_BITS = 0x7FC00000


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _untouched(t):
    return bool((_bits(t) == NAN_BITS).all())


def _others(d):
    off = torch.ones(d["N"], dtype=torch.bool)
    off[d["lig_rows"].long()] = False
    return off


class Grades:
    """assert_fp32_grade on every case of a test; the worst row per output goes to the report"""

    def __init__(self, title):
        self.title, self.rows = title, {}

    def check(self, key, got, r32, r64, d):
        rows = []
        assert_fp32_grade(got, r32, r64, f"{d['name']}: {key}", rows)
        self.rows.setdefault(key, []).append(rows[0])

    def close(self):
        for key, rows in self.rows.items():
            what, scale, e_gpu, e_cpu = max(rows, key=lambda r: r[2])
            REPORT.append((f"{self.title}: {key}" + (f" (worst of {len(rows)}: {what.split(':')[0]})" if len(rows) > 1 else ""),
                           scale, e_gpu, e_cpu))


def _one_hot_outcome(c_next, C, what):
    assert bool(((c_next == 0) | (c_next == 1)).all()) and bool((c_next.sum(-1) == 1).all()), what
    v = c_next.argmax(-1)
    assert int(v.min()) >= 0 and int(v.max()) < C
    return v


# ---- TargetDiff -----------------------------------------------------------------------------------------------------------------
def _targetdiff_args(d):
    t = {k: _dev(d[k]) for k in ("x_den", "logits", "lig_rows", "x_lig", "c_lig", "gen", "eps", "u")}
    t["tabs_t"] = [_dev(x) for x in SM.targetdiff_kernel_tables(d["T"])]
    t["tabs"] = (ctypes.c_void_p * 7)(*[x.data_ptr() for x in t["tabs_t"]])
    t["emb"] = [_dev(w) for w in d["emb"]]
    return t


def _targetdiff_head(d, a, C=None, t=None):
    p = _native.ptr
    return (p(a["x_den"]), p(a["logits"]), p(a["lig_rows"]), p(a["x_lig"]), p(a["c_lig"]), p(a["gen"]), d["n_lig"],
            d["C"] if C is None else C, d["t"] if t is None else t, d["T"], a["tabs"])


@pytest.mark.parametrize("point", SM.targetdiff_grid(), ids=lambda p: f"C{p[0]}-t{p[1]}-s{p[2]:g}-n{p[3]}")
def test_targetdiff_step_kernels_against_fp64(point):
    d = SM.targetdiff_case(*point)
    r32, r64 = SM.targetdiff_reference(d, F32), SM.targetdiff_reference(d, F64)
    lib, p, s = _native.lib(), _native.ptr, _native.current_stream(DEV)
    n, N, C, a = d["n_lig"], d["N"], d["C"], _targetdiff_args(d)
    head, emb = _targetdiff_head(d, a), tuple(p(w) for w in a["emb"])
    x_next, c_next, v_next = _nan(n, 3), _nan(n, C), torch.full((n,), -1, dtype=torch.int32, device=DEV)
    _native.check(lib.cbgx_targetdiff_epilogue(*head, p(a["eps"]), p(a["u"]), p(x_next), p(c_next), p(v_next), s), "epilogue")
    bx, bc, X, Hb = _nan(n, 3), _nan(n, C), _nan(N, 3), _nan(N, SM.H)
    _native.check(lib.cbgx_targetdiff_step_boundary(*head, p(a["eps"]), p(a["u"]), p(bx), p(bc), *emb, p(X), p(Hb), s), "step_boundary")
    PX, PH = _nan(N, 3), _nan(N, SM.H)
    _native.check(lib.cbgx_targetdiff_prologue(p(a["x_lig"]), p(a["c_lig"]), p(a["lig_rows"]), n, C, *emb, p(PX), p(PH), s), "prologue")
    torch.cuda.synchronize()
    x_next, c_next, v_next, bx, bc, X, Hb, PX, PH = (t.cpu() for t in (x_next, c_next, v_next, bx, bc, X, Hb, PX, PH))
    rows, gen, off = d["lig_rows"].long(), d["gen"].bool(), _others(d)
    # continuous
    g = Grades(d["name"])
    g.check("x_next", x_next, r32["x_next"], r64["x_next"], d)
    g.close()
    # context rows keep the bits of their state
    assert _same_bits(x_next[~gen], d["x_lig"][~gen]) and _same_bits(c_next[~gen], d["c_lig"][~gen])
    # discrete: an exact one-hot, v_next its index, equal to fp64 on every uncontested row
    v = _one_hot_outcome(c_next, C, d["name"])
    assert torch.equal(v_next.long(), v)
    con, err = SM.contested_rows(r32["score"], r64["score"], gen, d["tie_rows"])
    share = SM.contested_share(con, gen)
    SHARES.append((d["name"], int(gen.sum()), share, err))
    print(f"{d['name']}: contested {int(con.sum())} of {int(gen.sum())} generated rows ({100 * share:.2f} %), fp32 score error {err:.2e}")
    keep = ~con
    for k in d["tie_rows"]:
        keep[k] = False
    bad = torch.nonzero(v[keep] != r64["v_next"][keep]).flatten()
    assert bad.numel() == 0, (d["name"], "uncontested rows differ from fp64", torch.nonzero(keep).flatten()[bad][:8].tolist())
    assert share <= SM.CONTEST_CAP, (d["name"], share)
    for k, win in d["tie_rows"].items():               # bit-equal scores: the first index
        assert int(v[k]) == (win if gen[k] else int(d["c_lig"][k].argmax())), (d["name"], k)
    # the boundary kernel: the epilogue's outputs bit for bit, and the composed rows of the next step
    assert _same_bits(bx, x_next) and _same_bits(bc, c_next)
    assert _same_bits(X[rows], x_next) and _same_bits(Hb[rows], SM.onehot_features(d["emb"], v))
    assert _untouched(X[off]) and _untouched(Hb[off])
    # the prologue: the current state's rows
    assert _same_bits(PX[rows], d["x_lig"]) and _same_bits(PH[rows], SM.onehot_features(d["emb"], d["c_lig"].argmax(-1)))
    assert _untouched(PX[off]) and _untouched(PH[off])


def test_targetdiff_bad_sizes_are_rejected_without_a_launch():
    """C = 33 (> MAXC) and t = T: CBGX_E_INVALID, nothing written"""
    d = SM.targetdiff_case(13, 1, 3.0, 256)
    lib, p, s = _native.lib(), _native.ptr, _native.current_stream(DEV)
    n, N, a = d["n_lig"], d["N"], _targetdiff_args(d)
    emb = tuple(p(w) for w in a["emb"])
    out = [_nan(n, 3), _nan(n, 33), _nan(N, 3), _nan(N, SM.H)]
    v_next = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    for C, t in ((33, None), (None, d["T"]), (0, None), (None, -1)):
        head = _targetdiff_head(d, a, C=C, t=t)
        with pytest.raises(ValueError):
            _native.check(lib.cbgx_targetdiff_epilogue(*head, p(a["eps"]), p(a["u"]), p(out[0]), p(out[1]), p(v_next), s), "epilogue")
        with pytest.raises(ValueError):
            _native.check(lib.cbgx_targetdiff_step_boundary(*head, p(a["eps"]), p(a["u"]), p(out[0]), p(out[1]), *emb, p(out[2]),
                                                            p(out[3]), s), "step_boundary")
    with pytest.raises(ValueError):
        _native.check(lib.cbgx_targetdiff_prologue(p(a["x_lig"]), p(a["c_lig"]), p(a["lig_rows"]), n, 33, *emb, p(out[2]), p(out[3]), s),
                      "prologue")
    torch.cuda.synchronize()
    assert all(_untouched(t.cpu()) for t in out) and bool((v_next == -1).all())


# ---- DiffBP ---------------------------------------------------------------------------------------------------------------------
def _diffbp_call(d, x_next, c_next, n_lig=None, lig_ptr=None):
    lib, p, s = _native.lib(), _native.ptr, _native.current_stream(DEV)
    tb = SM.diffbp_tables(d["T"])
    a = {k: _dev(d[k]) for k in ("x_den", "x_com", "x_in", "logits", "lig_rows", "lig_ptr", "x_lig", "c_lig", "gen", "eps", "u")}
    a["acp"], a["betas"] = _dev(tb["alphas_cumprod"]), _dev(tb["betas"])
    if lig_ptr is not None:
        a["lig_ptr"] = _dev(lig_ptr)
    rc = lib.cbgx_diffbp_epilogue(p(a["x_den"]), p(a["x_com"]), p(a["x_in"]), p(a["logits"]), p(a["lig_rows"]), p(a["lig_ptr"]),
                                  p(a["x_lig"]), p(a["c_lig"]), p(a["gen"]), d["n_lig"] if n_lig is None else n_lig, d["B"], d["C"],
                                  d["t"], d["T"], p(a["acp"]), p(a["betas"]), d["absorbing"], p(a["eps"]), p(a["u"]), p(x_next),
                                  p(c_next), s)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("C,absorbing", [(C, a) for C in SM.BP_C for a in (0, C - 1)])
def test_diffbp_epilogue_against_fp64(C, absorbing):
    g = Grades(f"diffbp C={C} absorbing={absorbing}")
    for d in SM.diffbp_cases(C, absorbing):
        r32, r64 = SM.diffbp_reference(d, F32), SM.diffbp_reference(d, F64)
        n = d["n_lig"]
        x_next, c_next = _nan(n, 3), _nan(n, C)
        _native.check(_diffbp_call(d, x_next, c_next), "cbgx_diffbp_epilogue")
        x_next, c_next = x_next.cpu(), c_next.cpu()
        g.check("x_next", x_next, r32["x_next"], r64["x_next"], d)
        gen, cur = d["gen"].bool(), d["c_lig"].argmax(-1)
        assert _same_bits(x_next[~gen], d["x_lig"][~gen]) and _same_bits(c_next[~gen], d["c_lig"][~gen]), d["name"]
        v = _one_hot_outcome(c_next, C, d["name"])
        # `u < prob` and the argmax of the logits are exact in every precision (u is kept off prob, or sits on it exactly):
        # nothing is contested but the built-in ties, and those take the first index
        decided = SM.diffbp_decided(d)
        con, err = SM.contested_rows(r32["score"], r64["score"], decided, d["tie_rows"])
        assert err == 0.0 and not bool(con.any())
        SHARES.append((d["name"], int(gen.sum()), 0.0, err))
        bad = torch.nonzero(v != r64["v_next"]).flatten()
        assert bad.numel() == 0, (d["name"], "types differ from fp64", bad[:8].tolist())
        for k, win in d["tie_rows"].items():
            assert int(v[k]) == (win if decided[k] else int(cur[k])), (d["name"], k)
        if (d["T"], d["t"]) == (4, 2):      # prob == 0.5 exactly: u == prob stays, the next float below changes
            elig = gen & (cur == absorbing)
            at, below = elig & (d["u"] == 0.5), elig & (d["u"] == SM.U_BELOW_HALF)
            assert bool(at.any()) and bool(below.any())
            assert torch.equal(v[at], cur[at]) and torch.equal(v[below], d["logits"][d["lig_rows"].long()][below].argmax(-1))
    g.close()


# ---- DiffSBDD -------------------------------------------------------------------------------------------------------------------
def _diffsbdd_call(d, out, n_lig=None, lig_ptr=None, shift=True):
    lib, p, s = _native.lib(), _native.ptr, _native.current_stream(DEV)
    a = {k: _dev(d[k]) for k in ("x_den", "logits", "graph_ptr", "lig_rows", "lig_ptr", "lig_flag", "x_lig", "c_lig", "eps_x", "eps_c")}
    if lig_ptr is not None:
        a["lig_ptr"] = _dev(lig_ptr)
    emb = [_dev(w) for w in d["emb"]]
    inv_alpha, coef, sigma = d["coef"]
    rc = lib.cbgx_diffsbdd_step(p(a["x_den"]), p(a["logits"]), p(a["graph_ptr"]), p(a["lig_rows"]), p(a["lig_ptr"]), p(a["lig_flag"]),
                                p(a["x_lig"]), p(a["c_lig"]), d["n_lig"] if n_lig is None else n_lig, d["B"], d["C"], inv_alpha, coef,
                                sigma, d["do_x"], d["do_c"], p(a["eps_x"]), p(a["eps_c"]), *(p(w) for w in emb), p(out["x_next"]),
                                p(out["c_next"]), p(out["x"]), p(out["h"]), p(out["shift"]) if shift else None, p(out["frame"]), s)
    torch.cuda.synchronize()
    return rc


def _diffsbdd_outputs(d):
    return dict(x_next=_nan(d["n_lig"], 3), c_next=_nan(d["n_lig"], d["C"]), x=_dev(d["x"].clone()), h=_nan(d["N"], SM.H),
                shift=_nan(d["B"], 3), frame=_dev(d["frame0"].clone()) if d["framed"] else None)


@pytest.mark.parametrize("t_idx", SM.SB_STEPS)
@pytest.mark.parametrize("framed", [False, True], ids=["unframed", "framed"])
def test_diffsbdd_step_against_fp64(framed, t_idx):
    g = Grades(f"diffsbdd {'framed' if framed else 'unframed'} t={t_idx}")
    for i, d in enumerate(SM.diffsbdd_cases(framed, t_idx)):
        r32, r64 = SM.diffsbdd_reference(d, F32), SM.diffsbdd_reference(d, F64)
        out = _diffsbdd_outputs(d)
        _native.check(_diffsbdd_call(d, out), "cbgx_diffsbdd_step")
        o = {k: (v.cpu() if v is not None else None) for k, v in out.items()}
        rows, rec, off, bl = d["lig_rows"].long(), d["rec_rows"], _others(d), d["bl"]
        empty = torch.tensor([k for k, sz in enumerate(d["lig_sizes"]) if sz == 0], dtype=torch.long)
        # next ligand state
        if d["do_x"]:
            g.check("x_next", o["x_next"], r32["x_next"], r64["x_next"], d)
            g.check("shift", o["shift"], r32["shift"], r64["shift"], d)
            assert bool((_bits(o["shift"][empty]) == 0).all()), d["name"]             # a ligand-free graph removes a zero mean
        else:
            assert _same_bits(o["x_next"], d["x_lig"]) and bool((_bits(o["shift"]) == 0).all()), d["name"]
        if d["do_c"]:
            g.check("c_next", o["c_next"], r32["c_next"], r64["c_next"], d)
        else:
            assert _same_bits(o["c_next"], d["c_lig"]), d["name"]
        # composed rows of the next step
        g.check("h rows", o["h"][rows], r32["h"], r64["h"], d)
        assert _untouched(o["h"][off]), d["name"]
        if framed:
            if d["do_x"]:
                g.check("frame_shift", o["frame"], r32["frame"], r64["frame"], d)
                assert _same_bits(o["frame"][empty], d["frame0"][empty]), d["name"]
            else:
                assert _same_bits(o["frame"], d["frame0"]), d["name"]
            assert _same_bits(o["x"][rows], o["x_next"] + o["frame"][bl]), d["name"]  # as the kernel computes it
            assert _same_bits(o["x"][rec], d["x"][rec]), d["name"]                   # the pocket rows are never touched
        else:
            assert _same_bits(o["x"][rows], o["x_next"]), d["name"]
            if d["do_x"]:
                g.check("moved pocket rows", o["x"][rec], r32["x_rec"], r64["x_rec"], d)
            else:
                assert _same_bits(o["x"][rec], d["x"][rec]), d["name"]
        if i == 0:      # shift == NULL: the same step, nothing else changes
            out2 = _diffsbdd_outputs(d)
            _native.check(_diffsbdd_call(d, out2, shift=False), "cbgx_diffsbdd_step")
            for k in ("x_next", "c_next", "x", "h", "frame"):
                assert out2[k] is None or torch.equal(_bits(out2[k]), _bits(out[k])), (d["name"], k)
            assert _untouched(out2["shift"].cpu())
    g.close()


def test_no_ligand_atoms_is_ok_and_writes_nothing():
    """include/cbgx.h: n_lig == 0 (with any n_graphs) or n_graphs == 0 returns CBGX_OK before anything is looked at -- no output, not
    shift and not frame_shift, is written"""
    d = SM.diffbp_case(13, 0, 1000, 1, SM.SIZES_B)
    x_next, c_next = _nan(d["n_lig"], 3), _nan(d["n_lig"], 13)
    zeros = torch.zeros(d["B"] + 1, dtype=torch.int32)
    assert _diffbp_call(d, x_next, c_next, n_lig=0, lig_ptr=zeros) == 0
    assert _untouched(x_next.cpu()) and _untouched(c_next.cpu())
    d = SM.diffsbdd_case(8, 1, SM.SIZES_B, True, 1, 1)
    out = _diffsbdd_outputs(d)
    assert _diffsbdd_call(d, out, n_lig=0, lig_ptr=zeros) == 0
    assert all(_untouched(out[k].cpu()) for k in ("x_next", "c_next", "h", "shift"))
    assert _same_bits(out["x"].cpu(), d["x"]) and _same_bits(out["frame"].cpu(), d["frame0"])


def _report_dir():
    """the run-output directory of the repository, where the other report tests store their tables: the first entry `<name>_out/` of
    .gitignore (it is kept out of history, so a clean checkout has to create it)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, ".gitignore")) as f:
        name = next(line.strip().rstrip("/") for line in f if re.fullmatch(r"\w+_out/", line.strip()))
    out = os.path.join(root, name)
    os.makedirs(out, exist_ok=True)
    return out


def test_zz_report_step_kernel_errors():
    """prints the error table and the contested shares collected above and stores them in the run-output directory"""
    if not REPORT:
        pytest.skip("no rows collected (run the whole file)")
    lines = ["case | magnitude | libcbgx err / magnitude | fp32 oracle err / magnitude", "---|---|---|---"]
    lines += [f"{w} | {s:.3g} | {a:.2e} | {b:.2e}" for w, s, a, b in REPORT]
    td = [r for r in SHARES if r[0].startswith("targetdiff")]
    lines += ["", "case | generated rows | contested share | fp32 oracle score err", "---|---|---|---"]
    lines += [f"{w} | {n} | {100 * sh:.2f} % | {e:.2e}" for w, n, sh, e in td]
    bp = [r for r in SHARES if r[0].startswith("diffbp")]
    lines += ["", f"diffbp: {len(bp)} cases, contested share 0.00 % in each (the logits are compared as they are; score err "
                  f"{max([r[3] for r in bp], default=0.0):.1e})"]
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(_report_dir(), "step_kernel_errors.md"), "w") as f:
        f.write(text + "\n")
