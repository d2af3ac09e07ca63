// Packed conv-weight images: the tile constants that fix their padding, shared by the packers (weight_image.hip, where
// set_fill_pack_desc turns them into a layout) and by the launch code of the kernels that read the images.
#pragma once
#include "common.h"

// fp32 small-tile (SET_IMG_F32, conv1d_mfma_kernel): 32-row blocks, input channels in LDS chunks of KC
constexpr int KC = 16;
// fp32 big-tile (SET_IMG_F32_BIG, conv1d_mfma_v2_kernel): 128 * RB rows per block, channels padded to 16 and walked in LDS chunks of
// at most V2_CH -- half of that when a chunk with its halo would not leave room for two blocks per CU
constexpr int V2_CH = 256, V2_CIN_PAD = 16;
static inline int v2_rb(int Cout) { return Cout >= 384 ? 4 : (Cout >= 192 ? 2 : 1); }
static inline int v2_ch_max(int halo) { return (64 + halo) * V2_CH * 4 > 96 * 1024 ? 128 : V2_CH; }
// bf16 (SET_IMG_BF16, bf16.hip): rows padded to 128, input channels to chunks of 32
constexpr int BF16_IMG_ROWS = 128, BF16_IMG_CH = 32;
