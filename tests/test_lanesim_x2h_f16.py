"""Lane-level model of the two split-f16 contractions of edge_x2h_f16_kernel (CPU only): the operand maps of the scores
and of the aggregation (one v_mfma_f32_16x16x16_f16 step per tile and half each), the split
hi = f16(v), lo = f16(v - hi) with the three products hi hi + lo hi + hi lo, and the power-of-two scale rules of edge_body.h /
edge_common.h (split_exponent, LN_OUT_MAX, W_UP), on layer 0 of the golden two-graph case.

Bound: the project's split-f16 bound 2^-21 sum |a| |b| against the fp64 contraction of the same fp32 operands."""
import os

import numpy as np
import pytest

from tests import lanesim as LS

L, C_, Q_ = LS.L, LS.C_, LS.Q_
LN_OUT_MAX = np.float32(11.27)      # edge_common.h: >= sqrt(127)
W_UP = np.float32(16384.0)
SPLIT_K_MAX = 126


def split_exponent(m, zero_is_one):
    """edge_common.h split_exponent: k with m 2^k in [2^14, 2^15), clamped to +-126; zero (or subnormal) m -> 0 when zero_is_one"""
    E = int((np.float32(m).view(np.uint32) >> 23) & 0xff)
    if zero_is_one and E == 0:
        return 0
    return max(-SPLIT_K_MAX, min(SPLIT_K_MAX, 141 - E))


def pow2(k):
    return np.float32(np.ldexp(1.0, k))


def kh_of(gamma, beta):
    return split_exponent(np.float32(LN_OUT_MAX * np.abs(gamma).max() + np.abs(beta).max()), False)


def scores_lane_model(hid, qt, kh):
    """hid [32 edges][128] = ReLU(LayerNorm) output times 2^kh (fp32), qt [16 heads][128] fp32 -> scores [16][32] as the kernel
    leaves them: lane (c = head, q) reg r <-> edge 4q + r + 16hf, un-scaled by 2^-kq 2^-kh"""
    out = np.zeros((16, 32), np.float32)
    m = np.abs(qt).max(1)                                               # row maximum per head (xrow_max over the four q lanes)
    kq = np.array([split_exponent(v, True) for v in m])
    qs = (qt * np.array([pow2(k) for k in kq])[:, None]).astype(np.float32)
    assert np.isfinite(qs.astype(np.float16)).all()
    for hf in range(2):
        acc = [np.zeros((4, 64), np.float32), np.zeros((4, 64), np.float32)]
        for t in range(8):
            ch = [16 * t + 4 * Q_ + j for j in range(4)]                    # the lane's four channels of tile t
            a = np.stack([hid[C_ + 16 * hf, ch[j]] for j in range(4)])      # A: lane (c = edge, q)
            b = np.stack([qs[C_, ch[j]] for j in range(4)])                 # B: lane (c = head, q), same channels
            ah, al = LS.split_f16(a)
            bh, bl = LS.split_f16(b)
            k = t & 1                                                       # tile t -> out0, tile t + 1 -> out1
            for x, y in ((ah, bh), (al, bh), (ah, bl)):
                acc[k] = LS.mfma_f16(x, y, acc[k])
        un = np.array([pow2(-k) for k in kq])[C_] * pow2(-kh)
        res = (acc[0] + acc[1]) * un
        for r in range(4):
            out[C_, 4 * Q_ + r + 16 * hf] = res[r]
    return out


def aggregate_lane_model(hid, w, kh):
    """hid [32][128] (times 2^kh), w [16 heads][32 edges] in [0, 1] -> S [16][128]"""
    S = np.zeros((16, 128), np.float32)
    for t in range(8):
        acc = np.zeros((4, 64), np.float32)
        for hf in range(2):
            a = np.stack([hid[4 * Q_ + r + 16 * hf, LS.m_chan(t, C_)] for r in range(4)])    # A: lane (c = channel column, q)
            b = np.stack([w[C_, 4 * Q_ + r + 16 * hf] * W_UP for r in range(4)])              # B: lane (c = head, q)
            ah, al = LS.split_f16(a)
            bh, bl = LS.split_f16(b.astype(np.float32))
            for x, y in ((ah, bh), (al, bh), (ah, bl)):
                acc = LS.mfma_f16(x, y, acc)
        un = pow2(-kh) * (np.float32(1.0) / W_UP)
        for r in range(4):
            S[C_, LS.m_chan(t, 4 * Q_ + r)] = acc[r] * un
    return S


def bound(a, b):
    return 2.0 ** -21 * (np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)))


def subnormal_floor(a_scaled, b_scaled):
    """The bound above is relative per term; an operand whose `lo` (or the value itself) falls below the smallest normal f16, 2^-14,
    is only carried to half the subnormal quantum, 2^-25 ABSOLUTE in scaled units -- i.e. 2^-39 of the operand's largest possible
    value.  For a contraction of scaled operands that adds at most 2^-25 (sum |a'| + sum |b'|) per output (times the un-scale factor).
    Only the stress cases below need it (a saturated softmax at gamma = 30 leaves weights of 1e-10 next to weights of 1)."""
    A, B = np.abs(a_scaled.astype(np.float64)), np.abs(b_scaled.astype(np.float64))
    return 2.0 ** -25 * (A.sum(1)[:, None] + B.sum(0)[None, :])


# ---- layer-0 operands of the golden case ------------------------------------------------------------------------------------------
def _case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return {k: z[k] for k in z.files}


def _ln(v):
    v = v - v.mean(-1, keepdims=True)
    return v / np.sqrt((v * v).mean(-1, keepdims=True) + 1e-5)


def node_operands(g, W, tabs, i):
    """-> (normalised k hidden [32][128], normalised v hidden, Qt[i] [16][128], gate values [32], degree): the LayerNorm outputs
    BEFORE the affine, so that the tests can apply any (gamma, beta); invalid slots repeat the node itself, as in the kernel"""
    PDk, PDv, PSk, PSv, Qt = [t.astype(np.float64) for t in tabs]
    x, lig = g["x"].astype(np.float64), g["lig_flag"].astype(bool)
    src = g["edge_index"][0][g["edge_index"][1] == i]
    d = len(src)
    ew = np.zeros(32)
    ew[:d] = g["e_w"][g["edge_index"][1] == i, 0]
    j = np.concatenate([src, np.full(32 - d, i)]).astype(int)
    dist = np.sqrt(((x[i] - x[j]) ** 2).sum(-1))
    rbf = np.exp(-0.5 * (dist[:, None] - LS.MU[None, :].astype(np.float64)) ** 2) * (np.arange(32) < d)[:, None]
    et = np.where(lig[j], 0 if lig[i] else 1, 2 if lig[i] else 3)
    tp = 2 if lig[i] else 3
    out = []
    for PD, PS, Wt, Wr in ((PDk, PSk, W.Wt_k, W.Wr_k), (PDv, PSv, W.Wt_v, W.Wr_v)):
        pre = PD[i] + PS[j] + (Wt[et] - Wt[tp]) + np.einsum("eg,egm->em", rbf, Wr[et].astype(np.float64))
        out.append(_ln(pre))
    return out[0], out[1], Qt[i], ew, d


@pytest.fixture(scope="module")
def layer0(golden_dir, synthetic_sd):
    g = _case(golden_dir, "denoiser_2graphs")
    W = LS.Weights(synthetic_sd, "denoiser.blocks.0.x2h_layers.0", True)
    tabs = W.node_tables(g["h"], g["lig_flag"])
    return g, W, {i: node_operands(g, W, tabs, i) for i in (0, 5, 69, 70, 78, 146)}


def _hidden(norm, gamma, beta, kh):
    """what the kernel's LayerNorm tail produces from the affine it scaled in LDS: ReLU(norm (gamma 2^kh) + beta 2^kh), fp32"""
    up = pow2(kh)
    return np.maximum(norm.astype(np.float32) * (gamma.astype(np.float32) * up) + beta.astype(np.float32) * up, 0).astype(np.float32)


def _check_node(nk, nv, qt, ew, d, gk, bk, gv, bv, floor=False):
    khk, khv = kh_of(gk, bk), kh_of(gv, bv)
    hk, hv = _hidden(nk, gk, bk, khk), _hidden(nv, gv, bv, khv)
    for hd in (hk, hv):
        assert np.isfinite(hd.astype(np.float16)).all() and float(hd.max(initial=0.0)) < 2.0 ** 15
    qt32 = qt.astype(np.float32)
    sc = scores_lane_model(hk, qt32, khk)
    hk_true = hk.astype(np.float64) * 2.0 ** -khk                       # exact: power of two
    ref = qt32.astype(np.float64) @ hk_true.T
    tol = bound(qt32, hk_true.T)
    if floor:
        kq = np.array([split_exponent(v, True) for v in np.abs(qt32).max(1)])
        tol = tol + subnormal_floor(qt32 * 2.0 ** kq[:, None], hk.T) * 2.0 ** -(kq[:, None] + khk)
    assert (np.abs(sc - ref) <= tol + 1e-300).all(), np.abs(sc - ref).max()
    # softmax over the valid slots and the gate: the aggregation weights alpha e_w in [0, 1]
    valid = np.arange(32) < d
    s = np.where(valid, ref, -np.inf)
    ex = np.where(valid, np.exp(s - s.max(1, keepdims=True)), 0.0) if d else np.zeros_like(ref)
    w = (ex / np.maximum(ex.sum(1, keepdims=True), 1e-300) * ew).astype(np.float32)
    assert 0.0 <= float(w.min()) and float(w.max()) <= 1.0
    S = aggregate_lane_model(hv, w, khv)
    hv_true = hv.astype(np.float64) * 2.0 ** -khv
    refS = w.astype(np.float64) @ hv_true
    tol = bound(w, hv_true)
    if floor:
        tol = tol + subnormal_floor(w * float(W_UP), hv) * 2.0 ** -(14 + khv)
    assert (np.abs(S - refS) <= tol + 1e-300).all(), np.abs(S - refS).max()


def test_scores_and_aggregation_within_the_split_f16_bound(layer0):
    g, W, nodes = layer0
    for i, (nk, nv, qt, ew, d) in nodes.items():
        _check_node(nk, nv, qt, ew, d, W.g_k, W.be_k, W.g_v, W.be_v)


@pytest.mark.parametrize("gscale", [0.0, 1e-3, 30.0])
def test_layernorm_affine_scale_rule(layer0, gscale):
    """gamma = 0 (all hidden values equal ReLU(beta)), |gamma| = 1e-3 and 30: the scaled hidden values stay inside the f16 range,
    the bound sits in [2^14, 2^15) whenever it is a normal number, and the results keep the bound"""
    g, W, nodes = layer0
    sign = np.where(np.arange(128) % 3 == 0, -1.0, 1.0).astype(np.float32)
    gk = gv = (sign * np.float32(gscale)).astype(np.float32)
    for beta in (W.be_k, np.zeros(128, np.float32)):
        kh = kh_of(gk, beta)
        b = np.float32(LN_OUT_MAX * np.abs(gk).max() + np.abs(beta).max())
        assert -SPLIT_K_MAX <= kh <= SPLIT_K_MAX and np.isfinite(pow2(kh)) and np.isfinite(pow2(-kh)) and pow2(-kh) >= 2.0 ** -126
        if b > 0:
            assert 2.0 ** 14 <= float(b) * 2.0 ** kh < 2.0 ** 15
        else:
            assert kh == SPLIT_K_MAX            # zero affine: 0 2^k = 0 whatever k
        for i in (5, 70):
            nk, nv, qt, ew, d = nodes[i]
            assert np.abs(nk).max() <= float(LN_OUT_MAX) and np.abs(nv).max() <= float(LN_OUT_MAX)
            _check_node(nk, nv, qt, ew, d, gk, beta, gv, beta, floor=True)


@pytest.mark.parametrize("mag", [0.0, 1e-6, 1e6])
def test_query_row_scale_rule(layer0, mag):
    """a zero query row gets scale 1 (and scores 0); rows of magnitude 1e-6 and 1e6 are brought to [2^14, 2^15)"""
    g, W, nodes = layer0
    nk, nv, qt, ew, d = nodes[70]
    qt = qt.copy()
    qt[3] = 0.0 if mag == 0.0 else qt[3] / np.abs(qt[3]).max() * mag
    qt[7] = 0.0
    m = np.abs(qt.astype(np.float32)).max(1)
    for a in range(16):
        k = split_exponent(m[a], True)
        if m[a] == 0:
            assert k == 0
        else:
            assert 2.0 ** 14 <= float(m[a]) * 2.0 ** k < 2.0 ** 15
    khk = kh_of(W.g_k, W.be_k)
    sc = scores_lane_model(_hidden(nk, W.g_k, W.be_k, khk), qt.astype(np.float32), khk)
    assert (sc[7] == 0).all() and np.isfinite(sc).all()
    _check_node(nk, nv, qt, ew, d, W.g_k, W.be_k, W.g_v, W.be_v, floor=True)
