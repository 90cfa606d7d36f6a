// EPI_XF instantiations of the conv kernel (kernels_conv.h): a 3x3 conv with 32 output channels whose epilogue ALSO computes the next block's
// CondInjection -- y = (x_conv(out) + b) * (1 + scale) + shift (reference models/sr3_dwt.py:376-396) -- from its accumulator registers and writes it
// as a second output with its own GroupNorm partials.  One translation unit of its own so that it builds beside the main kernel family.
// Only the f16x2 tilings the inference plans of the engine configuration pick for these producers are instantiated:
//   the stem (cat[self_cond, x], VEC = 2), ResnetBlock.block2 (GroupNorm + SiLU prologue, + residual) and the Downsample conv (stride 2).
#include "conv_variants.h"

namespace ddif {

namespace {
// one fold: the f16x2 tiling TH x TW on NW waves with NB 32-cout blocks per item (conv_variants.h: 27 / 37 = 16x16 on eight, 28 / 68 = 8x16 on four)
template <int S, int TH, int TW, int CK, int NW, int NB, int PRO, int VEC, int EPI, int MATH>
ConvVariant xf(const char* name) { return conv_variant<3, S, 0, PRO, VEC, EPI, TH, TW, CK, NW, 1, 1, NB, MATH>(name); }
}  // namespace

// cfg: the tiling add_conv() chose for the conv WITHOUT the fold (27 = 16x16 pixels on eight waves, 28 = 8x16 on four, 37 = 27 with resident weights);
// epi: its epilogue bits without the fold (0 or EPI_RES); nbx: 32-cout blocks of the x_conv (1 or 2).  Null fn: no such instantiation -> no fold.
ConvVariant get_xf_variant(int stride, int pro, int cfg, int vec, int epi, int nbx) {
    if (stride == 1 && pro == PRO_GN_SILU && vec == 1 && epi == EPI_RES && nbx == 1) {  // ResnetBlock.block2 -> next block's x_conv 32 -> 32
        if (cfg == 37) return xf<1, 16, 16, 32, 8, 1, PRO_GN_SILU, 1, EPI_RES | EPI_XF1, KM_F16X2_WR>("conv3x3_gn_silu_res_xfilm");
        if (cfg == 27) return xf<1, 16, 16, 16, 8, 1, PRO_GN_SILU, 1, EPI_RES | EPI_XF1, KM_F16X2>("conv3x3_gn_silu_res_xfilm");
        if (cfg == 28) return xf<1, 8, 16, 16, 4, 1, PRO_GN_SILU, 1, EPI_RES | EPI_XF1, KM_F16X2>("conv3x3_gn_silu_res_xfilm");
    }
    if (stride == 1 && pro == PRO_NONE && vec == 2 && epi == 0 && nbx == 1) {  // stem -> first block's x_conv 32 -> 32
        if (cfg == 27) return xf<1, 16, 16, 16, 8, 1, PRO_NONE, 2, EPI_XF1, KM_F16X2>("conv3x3_cat_xfilm");
        if (cfg == 28) return xf<1, 8, 16, 16, 4, 1, PRO_NONE, 2, EPI_XF1, KM_F16X2>("conv3x3_cat_xfilm");
    }
    // ResnetBlock.block2 with 64 couts as ONE 64-cout item per pixel tile (conv_variants.h cfg 68) -> next block's x_conv 64 -> 64 (round 7).  Only the four-wave
    // 8 x 16 form: the eight-wave one has no registers left for it (conv_variants.h).  Its smem includes the x_conv's A fragments (ConvGeom::XWL).
    if (stride == 1 && pro == PRO_GN_SILU && vec == 1 && epi == EPI_RES && nbx == 2 && cfg == 68)
        return xf<1, 8, 16, 16, 4, 2, PRO_GN_SILU, 1, EPI_RES | EPI_XF2, KM_F16X2>("conv3x3_gn_silu_res_xfilm64");
    if (stride == 2 && pro == PRO_NONE && vec == 1 && epi == 0 && nbx == 2) {  // Downsample 32 -> 32 -> next block's x_conv 32 -> 64
        if (cfg == 28) return xf<2, 8, 16, 16, 4, 1, PRO_NONE, 1, EPI_XF2, KM_F16X2>("conv3x3_s2_xfilm");
    }
    return ConvVariant();
}

}  // namespace ddif
