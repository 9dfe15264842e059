"""Register / scratch / LDS budget and MFMA mix of the ligand-row h2x edge kernel (edge_h2x_lig.hip), read from the gfx950 ISA that
hipcc emits, and the addressing of its LDS image (layout.h A_IMG_H2L) restated in Python (no GPU needed; the recipe of
tests/test_isa_budget.py)."""
import os
import re

import pytest

from tests.test_isa_budget import CSRC, HIPCC, find, kernel_resources

H, HEADS, NT, G, FRAG_BLK = 128, 16, 4, 20, 320


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_h2x_lig_kernel_fits_its_budget(tmp_path):
    res, text = kernel_resources("edge_h2x_lig.hip", tmp_path)
    k = find(res, "edge_h2x_lig_kernelILi8ELb1E")
    assert k["scratch"] == 0 and k["vgpr"] <= 256, k          # 8 waves per CU = 2 per SIMD; a spill's reload drains the gathers
    assert k["lds"] <= 160 * 1024 and k["lds"] >= 4 * (29440 + G), k
    start = re.search(r"^_ZN4cbgx19edge_h2x_lig_kernelILi8ELb1E\S*:", text, flags=re.M).start()
    body = text[start:text.index(".end_amdhsa_kernel", start)]
    mfma32 = len(re.findall(r"^\s+v_mfma_f32_16x16x4", body, flags=re.M))
    mfma16 = len(re.findall(r"^\s+v_mfma_f32_16x16x16_f16", body, flags=re.M))
    # as edge_mfma_kernel<false, 8, true>: scores and values, 4 halves x 8 tiles x 4 exact-fp32 MFMAs; the rbf pre-activation, 4 halves
    # x 2 source-class passes x 8 tiles x 4 split-f16 MFMAs.  The fold: 8 tiles x 8 d x 2 packed FMAs on top of the LayerNorm tails'
    assert mfma32 == 128 and mfma16 == 256, (mfma32, mfma16)
    assert body.count("v_pk_fma_f32") >= 128


def test_image_layout_and_table_bases():
    """the image [k type 0 | v type 0 | k type 2 | v type 2 | dwt | ln | wbv | wfold] against what the shared body computes from its
    biased bases: etype() = 0 / 2 with lig_i = 1, the dwt rows of lig_i = 1, and the sizes in layout.h"""
    layout = open(os.path.join(CSRC, "layout.h")).read()
    slot = 8 * FRAG_BLK
    h2l_wt = 4 * slot
    h2l_ln, h2l_wbv, h2l_wfold = h2l_wt + 2 * H, h2l_wt + 2 * H + 4 * H, h2l_wt + 2 * H + 4 * H + HEADS * H
    size = h2l_wfold + H * H
    assert size == 29440 and 4 * (size + G) <= 163840
    for line in ("constexpr size_t H2L_WT = H2L_FRAG + 4 * 8 * FRAG_BLK;", "constexpr size_t H2L_LN = H2L_WT + 2 * H;",
                 "constexpr size_t H2L_WBV = H2L_LN + 4 * H;", "constexpr size_t H2L_WFOLD = H2L_WBV + (size_t)HEADS * H;",
                 "constexpr size_t H2L_IMG_SIZE = H2L_WFOLD + (size_t)H * H;", "constexpr size_t A_IMG_H2L = A_NQ_FRAG + (size_t)H * H;",
                 "constexpr size_t ATT_SIZE = A_IMG_H2L + H2L_IMG_SIZE;"):
        assert line in layout, line
    body = [l.split("//")[0] for l in open(os.path.join(CSRC, "edge_body.h"))]
    for expr in ("HL ? lds + H2L_FRAG : lds + IMG_FRAG_K", "HL ? lds + H2L_FRAG + 8 * (int)FRAG_BLK : lds + IMG_FRAG_V",
                 "HL ? lds + H2L_WT - 2 * H : lds + IMG_WT", "HL ? lds + H2L_WFOLD + 4 * lane : nullptr",
                 "HL ? lds + H2L_WBV + 4 * lane : lds + IMG_WBV + 4 * lane"):
        assert any(expr in l for l in body), expr
    pack = open(os.path.join(CSRC, "edge_h2x_lig.hip")).read()
    assert "v = img[((slot & 1) ? IMG_FRAG_V : IMG_FRAG_K) + (size_t)(slot & 2) * SLOT + u];" in pack
    assert "v = img[IMG_WT + 2 * H + (idx - H2L_WT)];" in pack
    assert "const int r = u & 3, lane = (u >> 2) & 63, d = (u >> 8) & 7, t = u >> 11;" in pack       # as pack_pp_image_kernel
    etype = lambda src_lig, lig_i: (0 if lig_i else 1) if src_lig else (2 if lig_i else 3)
    # source of every image slot in the general image (frag_k at 0, frag_v at NT * slot), as the pack kernel copies it ...
    src_of = {s: ((NT * slot if s & 1 else 0) + (s & 2) * slot) for s in range(4)}
    for kv, base in ((0, 0), (1, slot)):                       # ... and what the body reads: base + etype * slot
        for src_lig in (False, True):
            t = etype(src_lig, 1)
            assert t in (0, 2)
            image_slot = (base + t * slot) // slot
            assert src_of[image_slot] == kv * NT * slot + t * slot
    # dwt: the body reads base + lig_i * 2H + kv * H with base = H2L_WT - 2H; the pack kernel copies IMG_WT[lig_i = 1]
    for kv in (0, 1):
        assert (h2l_wt - 2 * H) + 1 * 2 * H + kv * H == h2l_wt + kv * H
