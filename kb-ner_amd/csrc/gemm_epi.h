// Epilogue flags of the GEMM kernels (gemm.hip, gemm_tile.h): the KBNER_EPI_* values of the C ABI under the names the kernels use,
// so the ABI's numbers and the kernels' cannot drift apart.
#pragma once
#include "kbner.h"

#define EPI_BIAS KBNER_EPI_BIAS          // + bias[n]
#define EPI_GELU KBNER_EPI_GELU          // C = gelu(pre), out2 = gelu'(pre) (bf16): what the backward EPI_DGELU multiplies by
#define EPI_ADD KBNER_EPI_ADD            // + addend[m,n] (bf16)
#define EPI_DGELU KBNER_EPI_DGELU        // * aux[m,n]  (aux = the gelu'(pre) the forward epilogue stored)
#define EPI_ATOMIC32 KBNER_EPI_ATOMIC32  // atomicAdd into C32 (fp32), no bf16 output
#define EPI_RMW32 KBNER_EPI_RMW32        // C32[m,n] += result, non-atomic 16-byte RMW (each output element owned by one lane)
#define EPI_COLSUM KBNER_EPI_COLSUM      // colsum[n] += sum_m out[m,n] (bias gradient of the producing layer), fp32 atomics, 2 per column per tile
#define EPI_DROP KBNER_EPI_DROP          // dropout on (acc*alpha + bias) BEFORE the residual add (BertSelfOutput / BertOutput); not with COLSUM
#define EPI_STORE32 KBNER_EPI_STORE32    // C32[m,n] = result (fp32, plain stores): one split-K slab, summed by kbner_splitk_finish
#define EPI_COLSUM_WS KBNER_EPI_COLSUM_WS  // with EPI_COLSUM: colsum is a workspace f32 [2 * M/256, N]; row 2*tile_row + wave_row receives this
                                           // tile's column sums by plain stores (no atomics); kbner_colsum_rows_f32 folds the rows afterwards
#define EPI_GELU_FWD KBNER_EPI_GELU_FWD  // C = gelu(pre), NO derivative output: the forward of inference (evaluate, frozen stack encoders)
