// Entry points of the two round-6 GEMM experiments (gemm128x.hip, gemm128s.hip in this directory), called from the
// -DKBNER_GEMM_LAB block of kb-ner_amd/csrc/gemm256.hip.  Lab builds only (README.md here): the product library has none of this.
#pragma once
#include "gemm_tile.h"

// gemm128x.hip: 128 x 256 tiles, epilogue of tile i-1 under the K loop of tile i (K = 1024 problems only); returns 1 when the
// launch is not one of its specialisations (the caller then takes the 256-row path), 0 / -hipError otherwise
int kbner_launch128x(int layout, const GroupArgs& ga, hipStream_t stream);
bool kbner_can128x(int layout, int M, int N, int K, int epi);
// gemm128s.hip: the same tiles with wave-specialised epilogues (4 MFMA waves hand the tile to 4 epilogue waves through LDS)
int kbner_launch128s(int layout, const GroupArgs& ga, hipStream_t stream);
