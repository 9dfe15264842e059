"""CPU lane model of node_query_kernel's first product (cbgbench_amd/csrc/node_mfma.hip) against the model of the chain it replaces.

The chain computes the q-hidden columns as MFMA(A = activations, B = weights): lane (c, q) of the A operand holds node c, of the B
operand output column c of a tile, both with K slot j of instruction u <-> k = 16 (2u + (j >> 2)) + 4q + (j & 3); register r of the
result is [node 4q + r][column c].  node_query_kernel swaps the operands, MFMA(A = weights, B = activations): the result's register r
of tile t in lane (c, q) is [channel 16t + 4q + r][node c] -- element z[4t + r] of the A-layout register file the LayerNorm and the
second product of node_qmlp_kernel work on, so no transpose is needed.  Modelled here: the v_mfma_f32_16x16x32_f16 operand layouts
(A[i = c][k = 8q + j], B[k = 8q + j][n = c], C register r <-> [4q + r][c]), the pack order of the new weight table, and the
arithmetic (exact f16 products, fp32 accumulation once per instruction -- tests/lanesim_node.py's model): every element must come out
with the bits of ``lanesim_node.split_gemm``."""
import os

import numpy as np

from tests import lanesim_node as LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128


def k_slot(u, q, j):
    return 16 * (2 * u + (j >> 2)) + 4 * q + (j & 3)


def mfma_16x16x32(a_lanes, b_lanes, acc):
    """a_lanes / b_lanes [64][8] f16 (lane (c, q) = c + 16 q: A[c][8q + j] / B[8q + j][c]); acc [64][4] f32, register r <-> [4q + r][c]"""
    A = np.zeros((16, 32)); B = np.zeros((32, 16))
    for lane in range(64):
        c, q = lane & 15, lane >> 4
        A[c, 8 * q:8 * q + 8] = a_lanes[lane].astype(np.float64)
        B[8 * q:8 * q + 8, c] = b_lanes[lane].astype(np.float64)
    C = A @ B                                   # exact: products of two f16, 32 terms, in float64
    out = np.empty_like(acc)
    for lane in range(64):
        c, q = lane & 15, lane >> 4
        for r in range(4):
            out[lane, r] = np.float32(np.float64(acc[lane, r]) + C[4 * q + r, c])
    return out


def pack_table(Wq):
    """pack_nquery_kernel: [part hi|lo][t 8][u 4][lane 64][j 8] f16 of Wq[k][16t + c] 2^kc; returns (table, kc)"""
    kc = LN.col_pow2(np.abs(Wq).max(0))
    Ws = np.ldexp(Wq, kc[None, :].astype(np.int32)).astype(np.float32)
    hi, lo = LN.split_f16(Ws)
    tab = np.zeros((2, 8, 4, 64, 8), np.float16)
    for idx in range(H * H):
        j, lane, u, t = idx & 7, (idx >> 3) & 63, (idx >> 9) & 3, idx >> 11
        c, q = lane & 15, lane >> 4
        tab[0, t, u, lane, j] = hi[k_slot(u, q, j), 16 * t + c]
        tab[1, t, u, lane, j] = lo[k_slot(u, q, j), 16 * t + c]
    return tab, kc


def test_pack_order_in_the_source_is_the_one_modelled():
    src = open(os.path.join(ROOT, "cbgbench_amd", "csrc", "node_mfma.hip")).read()
    assert "const int j = idx & 7, lane = (idx >> 3) & 63, u = (idx >> 9) & 3, t = idx >> 11;" in src
    assert "const int col = 4 * H + 16 * t + c, k = 16 * (2 * u + (j >> 2)) + 4 * q + (j & 3);" in src
    # operand order of the swapped product and its epilogue
    for term in ("MFMAH32(wl[j], ah[u], acc[j])", "MFMAH32(wh[j], al[u], acc[j])", "MFMAH32(wh[j], ah[u], acc[j])"):
        assert term in src
    assert src.index("MFMAH32(wl[j], ah[u], acc[j])") < src.index("MFMAH32(wh[j], al[u], acc[j])") < src.index("MFMAH32(wh[j], ah[u], acc[j])")
    assert "z[4 * t + 0] = fmaf(acc[j][0] * inv, ci.x, b.x);" in src


def test_swapped_product_gives_the_chain_bits_in_the_qmlp_register_order():
    rng = np.random.default_rng(0)
    h = (rng.standard_normal((16, H)) * np.exp(rng.uniform(-3, 3, (16, 1)))).astype(np.float32)
    h[3] *= np.float32(2.0 ** 20)               # a row far outside f16's range before scaling
    h[7] = 0.0                                  # an all-zero row
    Wq = (rng.standard_normal((H, H)) * np.exp(rng.uniform(-4, 1, (1, H)))).astype(np.float32)
    bq0 = rng.standard_normal(H).astype(np.float32)
    ref = LN.split_gemm(h, Wq, bq0)             # the chain: [node][channel]
    tab, kc = pack_table(Wq)
    # the activation operand: node_proj_kernel's ah[u] / al[u] -- lane c = node, slots k(u, q, j)
    ka = LN.row_pow2(np.abs(h).max(1))
    hs = np.ldexp(h, ka[:, None].astype(np.int32)).astype(np.float32)
    ah, al = LN.split_f16(hs)
    act = np.zeros((2, 4, 64, 8), np.float16)
    for u in range(4):
        for lane in range(64):
            c, q = lane & 15, lane >> 4
            for j in range(8):
                act[0, u, lane, j] = ah[c, k_slot(u, q, j)]
                act[1, u, lane, j] = al[c, k_slot(u, q, j)]
    rinv = np.ldexp(np.float32(1), (-ka).astype(np.int32)).astype(np.float32)
    cinv = np.ldexp(np.float32(1), (-kc).astype(np.int32)).astype(np.float32)
    z = np.zeros((64, 32), np.float32)          # the lane's register file: z[4t + r]
    for t in range(8):
        acc = np.zeros((64, 4), np.float32)
        for u in range(4):                      # per u: ah wl, al wh, ah wh
            acc = mfma_16x16x32(tab[1, t, u], act[0, u], acc)
            acc = mfma_16x16x32(tab[0, t, u], act[1, u], acc)
            acc = mfma_16x16x32(tab[0, t, u], act[0, u], acc)
        for lane in range(64):
            c, q = lane & 15, lane >> 4
            for r in range(4):
                ch = 16 * t + 4 * q + r
                scaled = np.float32(acc[lane, r] * rinv[c])
                z[lane, 4 * t + r] = np.float32(np.float64(scaled) * np.float64(cinv[ch]) + np.float64(bq0[ch]))   # one fma
    # node_qmlp_kernel's register file: z[4u + i] of lane (c, q) = P[node c][512 + 16u + 4q + i]
    for lane in range(64):
        c, q = lane & 15, lane >> 4
        want = np.array([ref[c, 16 * u + 4 * q + i] for u in range(8) for i in range(4)], np.float32)
        assert np.array_equal(z[lane].view(np.uint32), want.view(np.uint32)), lane
    assert np.array_equal(z[7], np.array([bq0[16 * u + i] for u in range(8) for i in range(4)], np.float32))   # lane (7, 0): the zero row


def test_table_holds_the_values_of_the_chunk_tables_in_another_order():
    """A_NQ_FRAG against A_NPROJ_FRAG chunks 8 and 9 ([ch][part][ct][u][lane][j], column 64 ch + 4c + ct): the same multiset of f16
    pieces per (column, k)"""
    rng = np.random.default_rng(1)
    Wq = rng.standard_normal((H, H)).astype(np.float32)
    tab, kc = pack_table(Wq)
    Ws = np.ldexp(Wq, kc[None, :].astype(np.int32)).astype(np.float32)
    hi, lo = LN.split_f16(Ws)
    for ch in range(2):
        for ct in range(4):
            for u in range(4):
                for lane in range(0, 64, 7):
                    c, q = lane & 15, lane >> 4
                    col = 64 * ch + 4 * c + ct
                    t, cc = col >> 4, col & 15
                    for j in range(8):
                        k = k_slot(u, q, j)
                        assert tab[0, t, u, cc + 16 * q, j] == hi[k, col] and tab[1, t, u, cc + 16 * q, j] == lo[k, col]
