// Tiling table of the general conv kernel (kernels_conv.h): which instantiation a configuration number means.  Internal to the translation units that
// instantiate the family -- ddif_conv_k3.cpp / ddif_conv_k3e.cpp (3x3 convs), ddif_conv_k1.cpp (1x1 convs), ddif_xf.cpp (x_conv folds) -- so that the kernels
// build in parallel and the plan builder (ddif_plan.cpp) no longer recompiles them.
#pragma once
#include "ddif_plan.h"
#include "kernels_conv.h"

namespace ddif {
namespace {

// One instantiation as the host sees it: the kernel, and every launch parameter read from the kernel's own geometry (ConvGeom).  Site first, then the tiling.
template <int KS, int S, int U, int PRO, int VEC, int EPI, int TH, int TW, int CK, int WM, int WN, int MB, int NB, int MATH, int ABL = 0>
ConvVariant conv_variant(const char* name = "") {
    using G = ConvGeom<KS, S, TH, TW, CK, WM, WN, NB, PRO, EPI, MATH>;
    ConvVariant v;
    v.fn = conv_mfma_kernel<KS, S, U, TH, TW, CK, WM, WN, MB, NB, PRO, VEC, EPI, ABL, MATH>;
    v.smem = G::smem;
    v.th = TH;
    v.tw = TW;
    v.nt = G::NT;
    v.nthr = G::NTHR;
    v.x3 = G::X3;
    v.f16 = G::F16;
    v.b1 = G::B1;
    v.wr = G::WR;
    v.nbs = G::NBS;
    v.name = name;
    return v;
}

// cfg -> pixel tile x couts, waves, operand format (KM_*: kernels_conv.h).  20 / 21 are the low-resolution kernel (ddif_lr.cpp), never looked up here.
//    0  8x16 x 32   4  exact        2  8x8  x 64   4  exact        every conv
//    1  8x16 x 64   4  exact        3  8x16 x 128  4  exact        4  8x8 x 128  4  exact        1x1 only: a wide cout tile stages -- and for PRO_GN_DW
//                                                                  recomputes -- the input once instead of once per 32 couts
//   12 13 15 14 16  = 0 1 3 2 4 on bf16x3;   52 53 55 54 56  = the same on bf16x1 (the throughput variant; the 32-cout tile too: no split to pay for)
//    5 16x16 x 32   8  exact        6 16x16 x 64   8  exact        plain 3x3 convs at the high-resolution levels: twice the MFMAs per staged input /
//                                                                  weight element (kernels_conv.h)
//    7 16x16 x 32   8  bf16x3       8  8x16 x 32   4  bf16x3       9  8x8 x 64   4  bf16x3       3x3;   47 48 49 = the same on bf16x1
//   27 16x16 x 32   8  f16x2       28  8x16 x 32   4  f16x2       29  8x8 x 64   4  f16x2        3x3 (7 / 8 / 9 + 20); also the stem (27 / 28) and the
//                                                                  stride-2 Downsample convs (28 / 29: 17 x 33 / 17 x 17 staged pixels)
//   37 = 27 with RESIDENT weights (KM_F16X2_WR, round 5): 32 input channels as ONE stage per work item, the cout tile's weights copied into LDS once per
//        workgroup.  Same pack, same accumulation order, same partials as 27 -- bit-identical results, 3-6 % faster in isolation
//        (profiles/r05/a_mbench_resident.txt).  Chosen by add_conv for 32 -> <= 32 channel convs.
//   67 16x16 x 64   8  f16x2       68  8x16 x 64   4  f16x2        = 27 / 28 with 64-cout work items (NB = 2, round 7): the halo tile is staged, normalised and
//        split once per 64 couts and an item walks half the stages per cout.  Same pack, same products and K order per (pixel, cout); the statistics partials
//        stay per 32-cout block, at the indices and in the summation order of 27 / 28 (ConvGeom::SPLIT) -- bit-identical outputs AND partials, so add_conv may
//        choose by the item count.  (The 16x16 x 64 tiling that rounds 4-5 measured and dropped regrouped the partials with the item count.)
// A row exists for a (KS, S, U, CK, PRO, VEC, EPI) site only where its group's predicate below holds: nothing else is instantiated.
template <int KS, int S, int U, int CK, int PRO, int VEC, int EPI = 0>
ConvVariant variant_for_cfg(int cfg) {
#define TILING(...) conv_variant<KS, S, U, PRO, VEC, EPI, __VA_ARGS__>()  // (TH, TW, CK, WM, WN, MB, NB, MATH) of this site
    constexpr bool K1 = KS == 1 && VEC == 1;         // 1x1 convs with float4 staging: the wide cout tiles
    constexpr bool K1_SPLIT = K1 && CK == 32;        // ... and their split-operand forms
    constexpr bool K3 = KS == 3 && S == 1 && VEC == 1;
    constexpr bool K3_EXACT8 = K3 && U == 0;         // the eight-wave exact-fp32 tilings
    // f16x2: stride-1 3x3 convs without a prologue or behind GroupNorm + SiLU; the stem (cat[self_cond, x] inside ONE 16-channel chunk: float4 staging with
    // a per-thread source select); the Downsample convs
    constexpr bool F16_S1 = K3 && (PRO == PRO_NONE || PRO == PRO_GN_SILU);
    constexpr bool F16_STEM = KS == 3 && S == 1 && U == 0 && VEC == 2 && PRO == PRO_NONE && EPI == 0;
    constexpr bool F16_DOWN = KS == 3 && S == 2 && U == 0 && VEC == 1 && PRO == PRO_NONE && EPI == 0;
    constexpr bool F16_WR = F16_S1 && U == 0;
    // 64-cout items: only the epilogues the 64-channel sites of the 64 x 64 / 32 x 32 levels use.  The eight-wave form with a GroupNorm prologue AND residual or
    // per-sample time-bias operands needs more than the 256 registers two waves per SIMD leave (24 / 36 bytes of scratch per lane, profiles/r11): the GroupNorm
    // sites (ResnetBlock convs; block1 needs its time-bias twin on the same tiling) have the four-wave form 68 only (one wave per SIMD, 512 registers, no scratch).
    constexpr bool F16_NB2 = F16_S1 && U == 0 && (EPI == 0 || EPI == EPI_RES || EPI == EPI_SILU || EPI == EPI_TBS);
    constexpr bool F16_NB2_EIGHT = F16_NB2 && PRO == PRO_NONE;
    switch (cfg) {
        case 0: return TILING(8, 16, CK, 4, 1, 1, 1, KM_EXACT);
        case 2: return TILING(8, 8, CK, 2, 2, 1, 1, KM_EXACT);
        case 1: if constexpr (K1) return TILING(8, 16, CK, 4, 1, 1, 2, KM_EXACT); break;
        case 3: if constexpr (K1) return TILING(8, 16, CK, 4, 1, 1, 4, KM_EXACT); break;
        case 4: if constexpr (K1) return TILING(8, 8, CK, 2, 2, 1, 2, KM_EXACT); break;
        case 12: if constexpr (K1_SPLIT) return TILING(8, 16, CK, 4, 1, 1, 1, KM_BF16X3); break;
        case 13: if constexpr (K1_SPLIT) return TILING(8, 16, CK, 4, 1, 1, 2, KM_BF16X3); break;
        case 15: if constexpr (K1_SPLIT) return TILING(8, 16, CK, 4, 1, 1, 4, KM_BF16X3); break;
        case 14: if constexpr (K1_SPLIT) return TILING(8, 8, CK, 2, 2, 1, 1, KM_BF16X3); break;
        case 16: if constexpr (K1_SPLIT) return TILING(8, 8, CK, 2, 2, 1, 2, KM_BF16X3); break;
        case 52: if constexpr (K1_SPLIT) return TILING(8, 16, CK, 4, 1, 1, 1, KM_BF16X1); break;
        case 53: if constexpr (K1_SPLIT) return TILING(8, 16, CK, 4, 1, 1, 2, KM_BF16X1); break;
        case 55: if constexpr (K1_SPLIT) return TILING(8, 16, CK, 4, 1, 1, 4, KM_BF16X1); break;
        case 54: if constexpr (K1_SPLIT) return TILING(8, 8, CK, 2, 2, 1, 1, KM_BF16X1); break;
        case 56: if constexpr (K1_SPLIT) return TILING(8, 8, CK, 2, 2, 1, 2, KM_BF16X1); break;
        case 7: if constexpr (K3) return TILING(16, 16, CK, 8, 1, 1, 1, KM_BF16X3); break;
        case 8: if constexpr (K3) return TILING(8, 16, CK, 4, 1, 1, 1, KM_BF16X3); break;
        case 9: if constexpr (K3) return TILING(8, 8, CK, 2, 2, 1, 1, KM_BF16X3); break;
        case 47: if constexpr (K3) return TILING(16, 16, CK, 8, 1, 1, 1, KM_BF16X1); break;
        case 48: if constexpr (K3) return TILING(8, 16, CK, 4, 1, 1, 1, KM_BF16X1); break;
        case 49: if constexpr (K3) return TILING(8, 8, CK, 2, 2, 1, 1, KM_BF16X1); break;
        case 27: if constexpr (F16_S1 || F16_STEM) return TILING(16, 16, CK, 8, 1, 1, 1, KM_F16X2); break;
        case 28: if constexpr (F16_S1 || F16_STEM || F16_DOWN) return TILING(8, 16, CK, 4, 1, 1, 1, KM_F16X2); break;
        case 29: if constexpr (F16_S1 || F16_DOWN) return TILING(8, 8, CK, 2, 2, 1, 1, KM_F16X2); break;
        case 37: if constexpr (F16_WR) return TILING(16, 16, 32, 8, 1, 1, 1, KM_F16X2_WR); break;
        case 67: if constexpr (F16_NB2_EIGHT) return TILING(16, 16, CK, 8, 1, 1, 2, KM_F16X2); break;
        case 68: if constexpr (F16_NB2) return TILING(8, 16, CK, 4, 1, 1, 2, KM_F16X2); break;
        case 5: if constexpr (K3_EXACT8) return TILING(16, 16, CK, 8, 1, 1, 1, KM_EXACT); break;
        case 6: if constexpr (K3_EXACT8) return TILING(16, 16, CK, 8, 1, 1, 2, KM_EXACT); break;
        default: break;
    }
    return ConvVariant();
#undef TILING
}
template <int KS, int S, int U, int CK, int PRO, int VEC>
ConvVariant variant_small_tiles(int cfg) {  // stride-2: the 8x16 halo would not fit comfortably in LDS
    return (cfg >= 2) ? variant_for_cfg<KS, S, U, CK, PRO, VEC>(cfg) : ConvVariant();
}
}  // namespace
}  // namespace ddif
