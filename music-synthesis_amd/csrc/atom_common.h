// Shared pieces of the fused ResidualAtom kernels (atom_fused.hip: one atom per launch, forward / training / backward
// data; stack_fused.hip: a whole ResidualStack per launch, inference): the layout of the pre-split weight images.  (The operand
// splits and scales: operand_split.h.)
#pragma once
#include "operand_split.h"

namespace {

// NP = 2: weights are packed as the fp16 pieces of S_w w, S_w the weight_scale PER CONV.  A pack is two launches: partial maxima
// (W_NPART workgroups per conv, written into the image's tail), then the pack proper, whose threads reduce the partials and
// whose first thread leaves 1 / S_w in the tail for the consuming kernels.
constexpr int W_NPART = 16;               // partial maxima per conv
// tail of an NP = 2 image (floats): [conv][W_NPART] partial maxima, then [conv] 1 / S_w
__host__ __device__ constexpr int wtail_floats(int nconv) { return nconv * W_NPART + nconv; }

// ---- weight image ------------------------------------------------------------------------------------------
// image[conv][ms][chunk][tap][piece][lane] (16 B each): lane's A fragment of the 32x32x16 MFMA for output rows
// ms*32 + (lane & 31), contraction channels chunk*16 + 8*(lane >> 5) + 0..7, tap `tap`.
__host__ __device__ constexpr size_t atom_conv_image_u4(int C, int NP) { return (size_t)(C / 32) * (C / 16) * 3 * NP * 64; }


}  // namespace
