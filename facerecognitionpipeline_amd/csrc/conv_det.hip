// Detector instances of the implicit-GEMM conv kernel (conv_mfma_impl.h): no pre-BN, two
// epilogues per tile: conv + BN + ReLU (EPI_AFFINE_PRELU with zero PReLU slopes) and BasicBlock
// conv2 + BN + residual + ReLU (EPI_AFFINE_RES_PRELU), on the three tiles the SCRFD layer shapes
// use (conv_dispatch.cpp); any other tile or epilogue is refused.  The detector's EPI_AFFINE and
// EPI_AFFINE_RES convs run on the embedding set's instances (conv_f32_w4 / conv_f32_w8).  f32 only.
#include "conv_mfma_impl.h"

namespace frhip {

hipError_t launch_conv_det(const ConvParams& p, ConvTile tile, Epi epi, int nsplit, hipStream_t s) {
  switch (tile) {
    case TILE_128x64_W8: return launch_tile<128, 64, 4, 2, false, 1>(p, false, epi, nsplit, s);
    case TILE_128x128_W8: return launch_tile<128, 128, 2, 4, false, 1>(p, false, epi, nsplit, s);
    case TILE_256x128_W8: return launch_tile<256, 128, 4, 2, false, 1>(p, false, epi, nsplit, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace frhip
