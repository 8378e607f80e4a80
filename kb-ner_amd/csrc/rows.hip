// Row-indexed helper kernels for gfx950: first-subtoken gather (+scatter backward), the T-wide
// emission head (fwd / dX / dW,db) and bf16 column sums (bias gradients).  All HBM/L2-bound
// integer-indexed row moves with 16-byte vector accesses; none of this is GEMM-shaped enough
// (N = T = 29) to belong on MFMA.
//
// Replaces: the per-token pooling loop + assign_batch_features + .cpu()/.to(device) bounce
// (flair/embeddings.py:3288-3345,108-124; sequence_tagger_model.py:909), the remove_x compaction
// loop (sequence_tagger_model.py:2474-2488: the host passes row indices of the kept tokens so
// gather and compaction are ONE gather), and self.linear (sequence_tagger_model.py:1027).
#include "common.h"

// wave-per-row kernels: 4 rows per block
static inline int rows_grid(int R) {
  int g = (R + 3) / 4;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return g;
}
// one thread per flat index 0..n: blocks of 256
#define FLAT_LAUNCH(kernel, n, stream, ...) \
  hipLaunchKernelGGL(kernel, dim3((unsigned)(((size_t)(n) + 255) / 256)), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__)

// ---- gather / scatter

// out[r,:] = idx[r] >= 0 ? src[idx[r],:] : 0        (bf16 rows, H % 8 == 0)
__global__ __launch_bounds__(256) void gather_rows_kernel(const bf16_t* __restrict__ src, const int* __restrict__ idx,
                                                          bf16_t* __restrict__ out, int R, int H) {
  const int lane = threadIdx.x % 64;
  const int wave = blockIdx.x * 4 + threadIdx.x / 64;
  const int nwave = gridDim.x * 4;
  for (int r = wave; r < R; r += nwave) {
    const int s = idx[r];
    for (int h0 = lane * 8; h0 < H; h0 += 512) {
      uint4 u = make_uint4(0, 0, 0, 0);
      if (s >= 0) u = *reinterpret_cast<const uint4*>(src + (size_t)s * H + h0);
      *reinterpret_cast<uint4*>(out + (size_t)r * H + h0) = u;
    }
  }
}

// dsrc[idx[r],:] = dout[r,:] for idx[r] >= 0 (indices are unique by construction: one first
// subtoken per word token); the caller zero-fills dsrc beforehand.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const bf16_t* __restrict__ dout, const int* __restrict__ idx,
                                                           bf16_t* __restrict__ dsrc, int R, int H) {
  const int lane = threadIdx.x % 64;
  const int wave = blockIdx.x * 4 + threadIdx.x / 64;
  const int nwave = gridDim.x * 4;
  for (int r = wave; r < R; r += nwave) {
    const int s = idx[r];
    if (s < 0) continue;
    for (int h0 = lane * 8; h0 < H; h0 += 512)
      *reinterpret_cast<uint4*>(dsrc + (size_t)s * H + h0) = *reinterpret_cast<const uint4*>(dout + (size_t)r * H + h0);
  }
}

// gather_rows / scatter_rows with the tagger head's two dropout sites on the token features (sequence_tagger_model.py:959-964):
// torch.nn.Dropout -- element (row r, column h) of site e -- and flair's LockedDropout (flair/nn.py:142-159) -- ONE mask per
// (sentence, column), shared by the n rows of a sentence: element (r / n, h) of site l; rows are laid out [B, n].
//     gather : out[r,:]       = idx[r] >= 0 ? bf16(src[idx[r],:] * m[r,:]) : 0
//     scatter: dsrc[idx[r],:] = bf16(dout[r,:] * m[r,:])   for idx[r] >= 0                m = m_e * m_l, formed in fp32
// (m_x = kept ? 1/(1-p_x) : 0; thresh 0: every element kept, scale 1).  Same shape as the plain pair: one wave per row, 16-byte
// accesses; the column keys of both sites depend on h alone, so the 512-column chunk is the OUTER loop and they stay in
// registers over the rows.  The row keys are wave-uniform (scalar registers).  SCATTER: idx addresses the output rows.
template <bool SCATTER>
__global__ __launch_bounds__(256) void rows_drop_kernel(const bf16_t* __restrict__ in, const int* __restrict__ idx,
                                                        bf16_t* __restrict__ out, int R, int H, int n, uint32_t seed_e,
                                                        uint32_t thresh_e, uint32_t seed_l, uint32_t thresh_l) {
  const int lane = threadIdx.x % 64;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64);
  const int nwave = gridDim.x * 4;
  const float scale = drop_scale(thresh_e) * drop_scale(thresh_l);
  for (int h0 = lane * 8; h0 < H; h0 += 512) {
    uint32_t cke[8], ckl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cke[j] = drop_colkey(seed_e, (uint32_t)(h0 + j));
      ckl[j] = drop_colkey(seed_l, (uint32_t)(h0 + j));
    }
    for (int r = wave; r < R; r += nwave) {
      const int s = idx[r];
      if (s < 0) {
        if (!SCATTER) *reinterpret_cast<uint4*>(out + (size_t)r * H + h0) = make_uint4(0, 0, 0, 0);
        continue;
      }
      const uint32_t rke = drop_rowkey(seed_e, (uint32_t)r);
      const uint32_t rkl = drop_rowkey(seed_l, (uint32_t)(r / n));
      float v[8];
      unpack8bf(*reinterpret_cast<const uint4*>(in + (size_t)(SCATTER ? r : s) * H + h0), v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] *= (drop_keep(rke, cke[j], thresh_e) && drop_keep(rkl, ckl[j], thresh_l)) ? scale : 0.0f;
      *reinterpret_cast<uint4*>(out + (size_t)(SCATTER ? s : r) * H + h0) = pack8bf(v);
    }
  }
}

// Encoder layer selection (TransformerWordEmbeddings(layers=..., use_scalar_mix=...), flair/embeddings.py:2983-2991, 3315-3343): the token
// feature is the first-sub-token row of k hidden states, concatenated ([R, k * H]) or averaged (torch.mean over the k rows, :3337;
// [R, H]), with the head's two dropout sites of rows_drop_kernel keyed by the OUTPUT column of the W-wide row:
//     concat: out[r, j * H + h] = idx[r] >= 0 ? bf16(src_j[idx[r], h] * m[r, j * H + h]) : 0
//     mean  : out[r, h]         = idx[r] >= 0 ? bf16((sum_j src_j[idx[r], h], fp32, j ascending) * fp32(1 / k) * m[r, h]) : 0
// The k source pointers travel BY VALUE in the kernel arguments (as ColsumBatch does): nothing is allocated on the device and the launch
// can be captured into a graph.  Same shape as rows_drop_kernel: one wave per row, 16-byte accesses, the 512-column chunk of the OUTPUT
// row as the outer loop, so the chunk's source (concat: one source per 8 columns, H % 8 == 0) and its column keys stay in registers over
// the rows.  DROP = false (both sites off): the mask code is compiled out -- a copy (concat) or the plain mean.
#define LAYERS_MAX 32
struct LayerSrcs {
  const bf16_t* p[LAYERS_MAX];
};
template <bool MEAN, bool DROP>
__global__ __launch_bounds__(256) void gather_rows_layers_kernel(const LayerSrcs srcs, int k, const int* __restrict__ idx,
                                                                 bf16_t* __restrict__ out, int R, int H, int n, uint32_t seed_e,
                                                                 uint32_t thresh_e, uint32_t seed_l, uint32_t thresh_l) {
  const int lane = threadIdx.x % 64;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64);
  const int nwave = gridDim.x * 4;
  const int W = MEAN ? H : k * H;
  const float scale = drop_scale(thresh_e) * drop_scale(thresh_l);
  const float inv_k = 1.0f / (float)k;
  for (int c0 = lane * 8; c0 < W; c0 += 512) {
    const int h0 = MEAN ? c0 : c0 % H;
    const bf16_t* __restrict__ src = srcs.p[MEAN ? 0 : c0 / H];
    uint32_t cke[8], ckl[8];
    if (DROP) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        cke[j] = drop_colkey(seed_e, (uint32_t)(c0 + j));
        ckl[j] = drop_colkey(seed_l, (uint32_t)(c0 + j));
      }
    }
    for (int r = wave; r < R; r += nwave) {
      const int s = idx[r];
      uint4 u = make_uint4(0, 0, 0, 0);
      if (s >= 0) {
        u = *reinterpret_cast<const uint4*>(src + (size_t)s * H + h0);
        if (MEAN || DROP) {
          float v[8];
          unpack8bf(u, v);
          if (MEAN) {
            for (int q = 1; q < k; ++q) {
              float x[8];
              unpack8bf(*reinterpret_cast<const uint4*>(srcs.p[q] + (size_t)s * H + h0), x);
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] += x[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] *= inv_k;
          }
          if (DROP) {
            const uint32_t rke = drop_rowkey(seed_e, (uint32_t)r);
            const uint32_t rkl = drop_rowkey(seed_l, (uint32_t)(r / n));
#pragma unroll
            for (int j = 0; j < 8; ++j)
              v[j] *= (drop_keep(rke, cke[j], thresh_e) && drop_keep(rkl, ckl[j], thresh_l)) ? scale : 0.0f;
          }
          u = pack8bf(v);
        }
      }
      *reinterpret_cast<uint4*>(out + (size_t)r * W + c0) = u;
    }
  }
}

// Sub-token pooling of a FROZEN encoder's hidden states (TransformerWordEmbeddings(pooling_operation=..., layers=..., use_scalar_mix=...)
// in the stacked tagger, flair/embeddings.py:3303-3345): word r owns the encoder-matrix rows span_rows[span_ptr[r] .. span_ptr[r + 1])
// -- its sub-tokens in order, not necessarily consecutive (a word may straddle a sliding-window seam) -- and its feature is a segmented
// reduction of those rows over k hidden states, written straight into the embedding's column block of the stack's input matrix
// (row stride ld_out; only columns [0, W) of rows [0, R) are written).  With m = the span's length, per layer j:
//     first: p_j = src_j[rows[0]]     last: p_j = src_j[rows[m - 1]]     first_last: p_j = [src_j[rows[0]], src_j[rows[m - 1]]]  (2 H wide)
//     mean : p_j = (sum over the span in order, fp32) * fp32(1 / m)
// and the row is p_0 .. p_{k-1} side by side or, LMEAN, (sum_j p_j, fp32, j ascending) * fp32(1 / k); ONE rounding to bf16, at the
// store.  m == 0 (a word the tokenizer dropped, :3306-3308): zeros.  first / last / first_last without LMEAN copy: the output bits are
// the source bits.  Same shape as gather_rows_layers_kernel: one wave per row, 16-byte accesses, the 512-column chunk of the OUTPUT row
// as the outer loop, so the chunk's layer, half and source column stay in registers over the rows (H % 8 == 0: an 8-column group lies in
// one layer and one half); span bounds and row numbers are wave-uniform.
#define POOL_FIRST 0
#define POOL_LAST 1
#define POOL_FIRST_LAST 2
#define POOL_MEAN 3
template <int OP, bool LMEAN>
__global__ __launch_bounds__(256) void pool_rows_layers_kernel(const LayerSrcs srcs, int k, const int* __restrict__ span_ptr,
                                                               const int* __restrict__ span_rows, bf16_t* __restrict__ out, int ld_out,
                                                               int R, int H) {
  const int lane = threadIdx.x % 64;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64);
  const int nwave = gridDim.x * 4;
  const int Wp = OP == POOL_FIRST_LAST ? 2 * H : H;
  const int W = LMEAN ? Wp : k * Wp;
  const int nj = LMEAN ? k : 1;
  const float inv_k = 1.0f / (float)k;
  for (int c0 = lane * 8; c0 < W; c0 += 512) {
    const int j0 = LMEAN ? 0 : c0 / Wp;
    const int cp = LMEAN ? c0 : c0 % Wp;
    const bool tail = OP == POOL_LAST || (OP == POOL_FIRST_LAST && cp >= H);
    const int h0 = (OP == POOL_FIRST_LAST && cp >= H) ? cp - H : cp;
    for (int r = wave; r < R; r += nwave) {
      const int lo = __builtin_amdgcn_readfirstlane(span_ptr[r]);
      const int hi = __builtin_amdgcn_readfirstlane(span_ptr[r + 1]);
      uint4 u = make_uint4(0, 0, 0, 0);
      if (hi > lo) {
        if (OP != POOL_MEAN && !LMEAN) {
          const int s = span_rows[tail ? hi - 1 : lo];
          u = *reinterpret_cast<const uint4*>(srcs.p[j0] + (size_t)s * H + h0);
        } else {
          const float inv_m = 1.0f / (float)(hi - lo);
          float acc[8];
          for (int q = 0; q < nj; ++q) {
            const bf16_t* __restrict__ src = srcs.p[j0 + q];
            float p[8];
            if (OP == POOL_MEAN) {
              unpack8bf(*reinterpret_cast<const uint4*>(src + (size_t)span_rows[lo] * H + h0), p);
              for (int t = lo + 1; t < hi; ++t) {
                float x[8];
                unpack8bf(*reinterpret_cast<const uint4*>(src + (size_t)span_rows[t] * H + h0), x);
#pragma unroll
                for (int i = 0; i < 8; ++i) p[i] += x[i];
              }
#pragma unroll
              for (int i = 0; i < 8; ++i) p[i] *= inv_m;
            } else {
              unpack8bf(*reinterpret_cast<const uint4*>(src + (size_t)span_rows[tail ? hi - 1 : lo] * H + h0), p);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = q == 0 ? p[i] : acc[i] + p[i];
          }
          if (LMEAN) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] *= inv_k;
          }
          u = pack8bf(acc);
        }
      }
      *reinterpret_cast<uint4*>(out + (size_t)r * ld_out + c0) = u;
    }
  }
}

// The backward of one source's share: columns [col0, col0 + H) of the W-wide feature gradient (row stride ld) are ADDED to the rows of
// that source's gradient idx names -- added, because the matrix already holds what the layers above sent down:
//     dst[idx[r], h] = bf16(f32(dst[idx[r], h]) + f32(dout[r * ld + col0 + h]) * (m[r, col0 + h] * scale))      for idx[r] >= 0
// (m as above, keyed by the column of the W-wide row; scale = 1 for a concatenated block, 1 / k under the mean).  Indices are unique
// (one first sub-token per word token): a plain read-modify-write; rows idx does not name are not touched.
template <bool DROP>
__global__ __launch_bounds__(256) void scatter_add_rows_ld_kernel(const bf16_t* __restrict__ dout, int ld, int col0,
                                                                  const int* __restrict__ idx, bf16_t* __restrict__ dst, int R, int H,
                                                                  float scale, int n, uint32_t seed_e, uint32_t thresh_e,
                                                                  uint32_t seed_l, uint32_t thresh_l) {
  const int lane = threadIdx.x % 64;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64);
  const int nwave = gridDim.x * 4;
  const float dscale = drop_scale(thresh_e) * drop_scale(thresh_l);
  for (int h0 = lane * 8; h0 < H; h0 += 512) {
    uint32_t cke[8], ckl[8];
    if (DROP) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        cke[j] = drop_colkey(seed_e, (uint32_t)(col0 + h0 + j));
        ckl[j] = drop_colkey(seed_l, (uint32_t)(col0 + h0 + j));
      }
    }
    for (int r = wave; r < R; r += nwave) {
      const int s = idx[r];
      if (s < 0) continue;
      float d[8], a[8];
      unpack8bf(*reinterpret_cast<const uint4*>(dout + (size_t)r * ld + col0 + h0), d);
      unpack8bf(*reinterpret_cast<const uint4*>(dst + (size_t)s * H + h0), a);
      if (DROP) {
        const uint32_t rke = drop_rowkey(seed_e, (uint32_t)r);
        const uint32_t rkl = drop_rowkey(seed_l, (uint32_t)(r / n));
#pragma unroll
        for (int j = 0; j < 8; ++j)
          a[j] += d[j] * (((drop_keep(rke, cke[j], thresh_e) && drop_keep(rkl, ckl[j], thresh_l)) ? dscale : 0.0f) * scale);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += d[j] * scale;
      }
      *reinterpret_cast<uint4*>(dst + (size_t)s * H + h0) = pack8bf(a);
    }
  }
}

// fp32 row gather (evaluation path: compaction of the [B*n, T] emissions to the non-S-X rows before Viterbi / CRF loss):
// out[r,:] = idx[r] >= 0 ? src[idx[r],:] : 0
__global__ __launch_bounds__(256) void gather_rows_f32_kernel(const float* __restrict__ src, const int* __restrict__ idx,
                                                              float* __restrict__ out, int R, int W) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R * W) return;
  const int r = i / W, c = i % W;
  const int s = idx[r];
  out[i] = s >= 0 ? src[(size_t)s * W + c] : 0.0f;
}

// Strided variant of gather_rows for the stacked-embedding concat of BASELINE config 5 (sequence_tagger_model.py:879-891:
// torch.cat of every embedding's [B, n, D_i] features): embedding i's pooled rows are written straight into its column block
// of the concatenated [rows, ld_out] matrix -- out[r, 0:H] = idx[r] >= 0 ? src[idx[r], 0:H] * mul : 0 -- so the concatenation
// never exists as a separate copy.  16-byte accesses (H % 8 == 0, ld_out % 8 == 0, out 16-byte aligned).
__global__ __launch_bounds__(256) void gather_rows_ld_kernel(const bf16_t* __restrict__ src, int ld_src, const int* __restrict__ idx,
                                                             bf16_t* __restrict__ out, int ld_out, int R, int H8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)R * H8) return;
  const int r = (int)(i / H8), c = (int)(i % H8);
  const int s = idx[r];
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (s >= 0) v = *reinterpret_cast<const uint4*>(src + (size_t)s * ld_src + c * 8);
  *reinterpret_cast<uint4*>(out + (size_t)r * ld_out + c * 8) = v;
}

// The stacked tagger's padded input matrix assembled from STORED feature rows (kbner/stack.py FeatureStore: compact bf16 rows
// [tokens, ld_store], computed once while the embeddings are frozen), with the embedding selection (sequence_tagger_model.py:879-891:
// features * selection[idx]) and the head's pre-RNN dropouts (:959-964, the two sites of rows_drop_kernel, same keys) applied on the
// way through:
//     out[r, c] = (r < R && c < W && idx[r] >= 0 && block_on[blk(c)]) ? bf16(store[idx[r], c] * m[r, c]) : 0      r < R_out, c < ld_out
// blk(c): the block with block_col[b] <= c < block_col[b + 1] (boundaries are multiples of 8, so a 16-byte chunk lies in one block;
// columns outside every block are zero).  The kernel writes EVERY element of out[0:R_out, 0:ld_out] -- the rows behind R and the
// columns behind W are the training layout's padding -- so nothing is zero-filled beforehand.  Same shape as rows_drop_kernel: one
// wave per row, the 512-column chunk of the output row as the outer loop, so the chunk's block switch and column keys stay in
// registers over the rows.  DROP = false (both sites off): a copy.
template <bool DROP>
__global__ __launch_bounds__(256) void gather_rows_blocks_kernel(const bf16_t* __restrict__ store, int ld_store,
                                                                 const int* __restrict__ idx, const int* __restrict__ block_col,
                                                                 const unsigned char* __restrict__ block_on, int nblk,
                                                                 bf16_t* __restrict__ out, int ld_out, int R, int R_out, int W, int n,
                                                                 uint32_t seed_e, uint32_t thresh_e, uint32_t seed_l,
                                                                 uint32_t thresh_l) {
  const int lane = threadIdx.x % 64;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64);
  const int nwave = gridDim.x * 4;
  const float scale = drop_scale(thresh_e) * drop_scale(thresh_l);
  for (int c0 = lane * 8; c0 < ld_out; c0 += 512) {
    bool on = false;
    if (c0 < W)
      for (int b = 0; b < nblk; ++b)
        if (block_col[b] <= c0 && c0 < block_col[b + 1]) on = block_on[b] != 0;
    uint32_t cke[8], ckl[8];
    if (DROP) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        cke[j] = drop_colkey(seed_e, (uint32_t)(c0 + j));
        ckl[j] = drop_colkey(seed_l, (uint32_t)(c0 + j));
      }
    }
    for (int r = wave; r < R_out; r += nwave) {
      const int s = r < R ? idx[r] : -1;
      uint4 u = make_uint4(0, 0, 0, 0);
      if (on && s >= 0) {
        u = *reinterpret_cast<const uint4*>(store + (size_t)s * ld_store + c0);
        if (DROP) {
          const uint32_t rke = drop_rowkey(seed_e, (uint32_t)r);
          const uint32_t rkl = drop_rowkey(seed_l, (uint32_t)(r / n));
          float v[8];
          unpack8bf(u, v);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            v[j] *= (drop_keep(rke, cke[j], thresh_e) && drop_keep(rkl, ckl[j], thresh_l)) ? scale : 0.0f;
          u = pack8bf(v);
        }
      }
      *reinterpret_cast<uint4*>(out + (size_t)r * ld_out + c0) = u;
    }
  }
}

// fp32 row scatter (data-parallel exchange of the touched word-embedding gradient rows, kbner/dp.py): dst[idx[r],:] = rows[r,:];
// indices unique, 16-byte accesses (W % 4 == 0)
__global__ __launch_bounds__(256) void scatter_rows_f32_kernel(const float4* __restrict__ rows, const int* __restrict__ idx,
                                                               float4* __restrict__ dst, int R, int W4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)R * W4) return;
  const int r = (int)(i / W4), c = (int)(i % W4);
  const int d = idx[r];
  if (d >= 0) dst[(size_t)d * W4 + c] = rows[i];
}

// fp32 row scatter-ADD, any width: dst[idx[r],:] += rows[r,:] for idx[r] >= 0 (indices unique: plain read-modify-write).
// The knowledge-distillation step (kbner/engine.py:Tagger.kd_loss) folds the gradient of the gold-label NLL, computed on the
// rows left after the remove_x compaction, back into the gradient of the all-token emissions the KD terms are defined on
// (the backward of the masked_select compaction, sequence_tagger_model.py:2474-2488, under autograd in the reference).
__global__ __launch_bounds__(256) void scatter_add_rows_f32_kernel(const float* __restrict__ rows, const int* __restrict__ idx,
                                                                   float* __restrict__ dst, int R, int W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)R * W) return;
  const int r = (int)(i / W), c = (int)(i % W);
  const int d = idx[r];
  if (d >= 0) dst[(size_t)d * W + c] += rows[i];
}

extern "C" {
int kbner_gather_rows(const bf16_t* src, const int* idx, bf16_t* out, int R, int H, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0);
  if (R == 0) return 0;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, src, idx, out, R, H);
  KBNER_LAUNCH_RET();
}

int kbner_scatter_rows(const bf16_t* dout, const int* idx, bf16_t* dsrc, int R, int H, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0);
  if (R == 0) return 0;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, dout, idx, dsrc, R, H);
  KBNER_LAUNCH_RET();
}

// both thresholds 0: the plain kernels (the same bytes, no multiply)
int kbner_gather_rows_drop(const bf16_t* src, const int* idx, bf16_t* out, int R, int H, int n, uint32_t seed_e, uint32_t thresh_e,
                           uint32_t seed_l, uint32_t thresh_l, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0 && n >= 1 && R % n == 0);
  if (R == 0) return 0;
  if (thresh_e == 0 && thresh_l == 0)
    hipLaunchKernelGGL(gather_rows_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, src, idx, out, R, H);
  else
    hipLaunchKernelGGL(rows_drop_kernel<false>, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, src, idx, out, R, H, n, seed_e,
                       thresh_e, seed_l, thresh_l);
  KBNER_LAUNCH_RET();
}

int kbner_scatter_rows_drop(const bf16_t* dout, const int* idx, bf16_t* dsrc, int R, int H, int n, uint32_t seed_e, uint32_t thresh_e,
                            uint32_t seed_l, uint32_t thresh_l, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0 && n >= 1 && R % n == 0);
  if (R == 0) return 0;
  if (thresh_e == 0 && thresh_l == 0)
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, dout, idx, dsrc, R, H);
  else
    hipLaunchKernelGGL(rows_drop_kernel<true>, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, dout, idx, dsrc, R, H, n, seed_e,
                       thresh_e, seed_l, thresh_l);
  KBNER_LAUNCH_RET();
}

// srcs: HOST array of k device pointers (bf16 [*, H] each), copied into the launch's arguments
int kbner_gather_rows_layers(const bf16_t* const* srcs, int k, int mean, const int* idx, bf16_t* out, int R, int H, int n,
                             uint32_t seed_e, uint32_t thresh_e, uint32_t seed_l, uint32_t thresh_l, void* stream) {
  KBNER_CHECK_ARG(srcs != nullptr && k >= 1 && k <= LAYERS_MAX && R >= 0 && H > 0 && H % 8 == 0 && H <= 8192 && n >= 1 && R % n == 0);
  KBNER_CHECK_ARG(mean != 0 || (long long)k * H <= 8192);
  LayerSrcs b;
  for (int i = 0; i < LAYERS_MAX; ++i) {
    b.p[i] = srcs[i < k ? i : 0];
    KBNER_CHECK_ARG(b.p[i] != nullptr);
  }
  if (R == 0) return 0;
  KBNER_CHECK_ARG(idx != nullptr && out != nullptr);
  const bool drop = thresh_e != 0 || thresh_l != 0;
#define LAYERS_LAUNCH(MEAN, DROP)                                                                                                  \
  hipLaunchKernelGGL((gather_rows_layers_kernel<MEAN, DROP>), dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, b, k, idx, out, R, \
                     H, n, seed_e, thresh_e, seed_l, thresh_l)
  if (mean && drop) LAYERS_LAUNCH(true, true);
  else if (mean) LAYERS_LAUNCH(true, false);
  else if (drop) LAYERS_LAUNCH(false, true);
  else LAYERS_LAUNCH(false, false);
#undef LAYERS_LAUNCH
  KBNER_LAUNCH_RET();
}

// srcs: HOST array of k device pointers, as above; span_ptr i32 [R + 1], span_rows i32 [span_ptr[R]]: DEVICE memory.  What the tables
// must hold (span_ptr non-decreasing from 0, every span_rows entry a row of every source) cannot be checked here; kbner.ops checks the
// host copy before it uploads them.
int kbner_pool_rows_layers(const bf16_t* const* srcs, int k, int layer_mean, int op, const int* span_ptr, const int* span_rows,
                           bf16_t* out, int ld_out, int R, int H, void* stream) {
  KBNER_CHECK_ARG(srcs != nullptr && k >= 1 && k <= LAYERS_MAX && op >= POOL_FIRST && op <= POOL_MEAN && R >= 0 && H > 0 && H % 8 == 0);
  KBNER_CHECK_ARG(ld_out > 0 && ld_out % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0);
  const long long W = (long long)(op == POOL_FIRST_LAST ? 2 : 1) * H * (layer_mean ? 1 : k);
  KBNER_CHECK_ARG(W <= ld_out);
  LayerSrcs b;
  for (int i = 0; i < LAYERS_MAX; ++i) {
    b.p[i] = srcs[i < k ? i : 0];
    KBNER_CHECK_ARG(b.p[i] != nullptr);
  }
  if (R == 0) return 0;
  KBNER_CHECK_ARG(span_ptr != nullptr && span_rows != nullptr && out != nullptr);
#define POOL_LAUNCH(OP, LMEAN)                                                                                                      \
  hipLaunchKernelGGL((pool_rows_layers_kernel<OP, LMEAN>), dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, b, k, span_ptr,  \
                     span_rows, out, ld_out, R, H)
#define POOL_LAUNCH_OP(OP)            \
  do {                                \
    if (layer_mean) POOL_LAUNCH(OP, true); \
    else POOL_LAUNCH(OP, false);      \
  } while (0)
  if (op == POOL_FIRST) POOL_LAUNCH_OP(POOL_FIRST);
  else if (op == POOL_LAST) POOL_LAUNCH_OP(POOL_LAST);
  else if (op == POOL_FIRST_LAST) POOL_LAUNCH_OP(POOL_FIRST_LAST);
  else POOL_LAUNCH_OP(POOL_MEAN);
#undef POOL_LAUNCH_OP
#undef POOL_LAUNCH
  KBNER_LAUNCH_RET();
}

int kbner_scatter_add_rows_ld(const bf16_t* dout, int ld, int col0, const int* idx, bf16_t* dst, int R, int H, float scale, int n,
                              uint32_t seed_e, uint32_t thresh_e, uint32_t seed_l, uint32_t thresh_l, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0 && ld > 0 && ld % 8 == 0 && col0 >= 0 && col0 % 8 == 0 && col0 + H <= ld && n >= 1 &&
                  R % n == 0);
  if (R == 0) return 0;
  KBNER_CHECK_ARG(dout != nullptr && idx != nullptr && dst != nullptr);
  if (thresh_e == 0 && thresh_l == 0)
    hipLaunchKernelGGL(scatter_add_rows_ld_kernel<false>, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, dout, ld, col0, idx, dst,
                       R, H, scale, n, seed_e, thresh_e, seed_l, thresh_l);
  else
    hipLaunchKernelGGL(scatter_add_rows_ld_kernel<true>, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, dout, ld, col0, idx, dst,
                       R, H, scale, n, seed_e, thresh_e, seed_l, thresh_l);
  KBNER_LAUNCH_RET();
}

int kbner_gather_rows_f32(const float* src, const int* idx, float* out, int R, int W, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && W > 0);
  if (R == 0) return 0;
  FLAT_LAUNCH(gather_rows_f32_kernel, R * W, stream, src, idx, out, R, W);
  KBNER_LAUNCH_RET();
}

int kbner_gather_rows_ld(const bf16_t* src, int ld_src, const int* idx, bf16_t* out, int ld_out, int R, int H, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0 && ld_src % 8 == 0 && ld_out % 8 == 0);
  if (R == 0) return 0;
  FLAT_LAUNCH(gather_rows_ld_kernel, (size_t)R * (H / 8), stream, src, ld_src, idx, out, ld_out, R, H / 8);
  KBNER_LAUNCH_RET();
}

// idx, block_col, block_on: DEVICE memory.  What the tables must hold (block_col ascending multiples of 8, block_col[nblk] <= W) cannot
// be checked here; kbner.ops checks the host copy.  Whatever they hold, no access leaves store[idx[r], 0:W] or out[0:R_out, 0:ld_out].
int kbner_gather_rows_blocks_drop(const bf16_t* store, int ld_store, const int* idx, const int* block_col, const unsigned char* block_on,
                                  int nblk, bf16_t* out, int ld_out, int R, int R_out, int W, int n, uint32_t seed_e, uint32_t thresh_e,
                                  uint32_t seed_l, uint32_t thresh_l, void* stream) {
  KBNER_CHECK_ARG(nblk >= 1 && nblk <= 64 && R >= 0 && R <= R_out && n >= 1 && R % n == 0);
  KBNER_CHECK_ARG(W > 0 && W % 8 == 0 && ld_store % 8 == 0 && ld_out % 8 == 0 && W <= ld_store && W <= ld_out);
  if (R_out == 0) return 0;
  KBNER_CHECK_ARG(out != nullptr && block_col != nullptr && block_on != nullptr && (R == 0 || (store != nullptr && idx != nullptr)));
  if (thresh_e == 0 && thresh_l == 0)
    hipLaunchKernelGGL(gather_rows_blocks_kernel<false>, dim3(rows_grid(R_out)), dim3(256), 0, (hipStream_t)stream, store, ld_store, idx,
                       block_col, block_on, nblk, out, ld_out, R, R_out, W, n, seed_e, thresh_e, seed_l, thresh_l);
  else
    hipLaunchKernelGGL(gather_rows_blocks_kernel<true>, dim3(rows_grid(R_out)), dim3(256), 0, (hipStream_t)stream, store, ld_store, idx,
                       block_col, block_on, nblk, out, ld_out, R, R_out, W, n, seed_e, thresh_e, seed_l, thresh_l);
  KBNER_LAUNCH_RET();
}

int kbner_scatter_rows_f32(const float* rows, const int* idx, float* dst, int R, int W, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && W > 0 && W % 4 == 0);
  if (R == 0) return 0;
  FLAT_LAUNCH(scatter_rows_f32_kernel, (size_t)R * (W / 4), stream, reinterpret_cast<const float4*>(rows), idx,
              reinterpret_cast<float4*>(dst), R, W / 4);
  KBNER_LAUNCH_RET();
}

int kbner_scatter_add_rows_f32(const float* rows, const int* idx, float* dst, int R, int W, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && W > 0);
  if (R == 0) return 0;
  KBNER_CHECK_ARG(rows != nullptr && idx != nullptr && dst != nullptr);
  FLAT_LAUNCH(scatter_add_rows_f32_kernel, (size_t)R * W, stream, rows, idx, dst, R, W);
  KBNER_LAUNCH_RET();
}
}  // extern "C"

// ---- the emission head

#define HEAD_MAXT 64        // tags per thread in head_bwd_dw_kernel; wider tag sets walk blocks of HEAD_MAXT tags
#define HEAD_WIDE_MAXT 192  // the widest tag set the head takes (the wide CRF kernels of csrc/crf_wide.hip end there)
#define HEAD_NCH 2        // 16-byte chunks of a row per lane in the kernels that hold the row in registers
#define HEAD_MAXH 1024    // the widest row they take
static_assert(HEAD_MAXH == 64 * 8 * HEAD_NCH, "HEAD_NCH chunks of 64 lanes x 8 columns cover HEAD_MAXH columns");

// sum_j xv[j] * w[j], j = 0..7: ONE expression for the three forward kernels (the same bits from each)
static __device__ __forceinline__ float head_dot8(const float (&xv)[8], const float* __restrict__ w) {
  const float4 a = *reinterpret_cast<const float4*>(w);
  const float4 b = *reinterpret_cast<const float4*>(w + 4);
  return xv[0] * a.x + xv[1] * a.y + xv[2] * a.z + xv[3] * a.w + xv[4] * b.x + xv[5] * b.y + xv[6] * b.z + xv[7] * b.w;
}

// emissions: out[r,t] = sum_h x[r,h] * w[t,h] + b[t]    (x bf16, w/b/out fp32; one wave per row)
__global__ __launch_bounds__(256) void head_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, int R, int H,
                                                       int T) {
  const int lane = threadIdx.x % 64;
  const int wave = blockIdx.x * 4 + threadIdx.x / 64;
  const int nwave = gridDim.x * 4;
  for (int r = wave; r < R; r += nwave) {
    float xv[HEAD_NCH][8];
#pragma unroll
    for (int c = 0; c < HEAD_NCH; ++c) {
      const int h0 = (lane + 64 * c) * 8;
      if (h0 < H) {
        unpack8bf(*reinterpret_cast<const uint4*>(x + (size_t)r * H + h0), xv[c]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[c][j] = 0.0f;
      }
    }
    for (int t = 0; t < T; ++t) {
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < HEAD_NCH; ++c) {
        const int h0 = (lane + 64 * c) * 8;
        if (h0 < H) acc += head_dot8(xv[c], w + (size_t)t * H + h0);
      }
      acc = wave_sum(acc);
      if (lane == 0) out[(size_t)r * T + t] = acc + bias[t];
    }
  }
}

// The same for FEW rows (round 6: a 4-sentence step has ~64 kept tokens): one wave per (row, tag) instead of one wave per row walking
// the T tags one after the other -- 29 dependent load + reduce rounds on 16 workgroups were 33 us of latency for 2 MFLOP.
__global__ __launch_bounds__(256) void head_fwd_rt_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out, int R, int H,
                                                          int T) {
  const int lane = threadIdx.x % 64;
  const int id = blockIdx.x * 4 + threadIdx.x / 64;
  if (id >= R * T) return;
  const int r = id / T, t = id % T;
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < HEAD_NCH; ++c) {
    const int h0 = (lane + 64 * c) * 8;
    if (h0 < H) {
      float xv[8];
      unpack8bf(*reinterpret_cast<const uint4*>(x + (size_t)r * H + h0), xv);
      acc += head_dot8(xv, w + (size_t)t * H + h0);  // (and the same chunk order as head_fwd_kernel: the same bits)
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) out[(size_t)r * T + t] = acc + bias[t];
}

// head_fwd_kernel for wide rows (H > HEAD_MAXH: linear(2 * hidden -> T) behind the BiLSTM): the row is walked in 512-column chunks per tag
// instead of being held in registers
__global__ __launch_bounds__(256) void head_fwd_wide_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ out, int R,
                                                            int H, int T) {
  const int lane = threadIdx.x % 64;
  const int wave = blockIdx.x * 4 + threadIdx.x / 64;
  const int nwave = gridDim.x * 4;
  for (int r = wave; r < R; r += nwave) {
    for (int t = 0; t < T; ++t) {
      float acc = 0.0f;
      for (int h0 = lane * 8; h0 < H; h0 += 512) {
        float xv[8];
        unpack8bf(*reinterpret_cast<const uint4*>(x + (size_t)r * H + h0), xv);
        acc += head_dot8(xv, w + (size_t)t * H + h0);
      }
      acc = wave_sum(acc);
      if (lane == 0) out[(size_t)r * T + t] = acc + bias[t];
    }
  }
}

// dx[r,h] = sum_t de[r,t] * w[t,h]        (one wave per row; bf16 out)
__global__ __launch_bounds__(256) void head_bwd_dx_kernel(const float* __restrict__ de, const float* __restrict__ w,
                                                          bf16_t* __restrict__ dx, int R, int H, int T) {
  const int lane = threadIdx.x % 64;
  const int wave = blockIdx.x * 4 + threadIdx.x / 64;
  const int nwave = gridDim.x * 4;
  for (int r = wave; r < R; r += nwave) {
    float acc[HEAD_NCH][8];
#pragma unroll
    for (int c = 0; c < HEAD_NCH; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[c][j] = 0.0f;
    for (int t = 0; t < T; ++t) {
      const float d = de[(size_t)r * T + t];
#pragma unroll
      for (int c = 0; c < HEAD_NCH; ++c) {
        const int h0 = (lane + 64 * c) * 8;
        if (h0 < H) {
          const float4 a = *reinterpret_cast<const float4*>(w + (size_t)t * H + h0);
          const float4 b = *reinterpret_cast<const float4*>(w + (size_t)t * H + h0 + 4);
          acc[c][0] += d * a.x; acc[c][1] += d * a.y; acc[c][2] += d * a.z; acc[c][3] += d * a.w;
          acc[c][4] += d * b.x; acc[c][5] += d * b.y; acc[c][6] += d * b.z; acc[c][7] += d * b.w;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < HEAD_NCH; ++c) {
      const int h0 = (lane + 64 * c) * 8;
      if (h0 < H) *reinterpret_cast<uint4*>(dx + (size_t)r * H + h0) = pack8bf(acc[c]);
    }
  }
}

// head_bwd_dx_kernel for wide rows (H > HEAD_MAXH: the head behind a concatenation of encoder layers, linear(k * hidden -> T)): the row is
// walked in 512-column chunks, as head_fwd_wide_kernel walks it, each chunk summing the T tags in the same order
__global__ __launch_bounds__(256) void head_bwd_dx_wide_kernel(const float* __restrict__ de, const float* __restrict__ w,
                                                               bf16_t* __restrict__ dx, int R, int H, int T) {
  const int lane = threadIdx.x % 64;
  const int wave = blockIdx.x * 4 + threadIdx.x / 64;
  const int nwave = gridDim.x * 4;
  for (int r = wave; r < R; r += nwave) {
    for (int h0 = lane * 8; h0 < H; h0 += 512) {
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
      for (int t = 0; t < T; ++t) {
        const float d = de[(size_t)r * T + t];
        const float4 a = *reinterpret_cast<const float4*>(w + (size_t)t * H + h0);
        const float4 b = *reinterpret_cast<const float4*>(w + (size_t)t * H + h0 + 4);
        acc[0] += d * a.x; acc[1] += d * a.y; acc[2] += d * a.z; acc[3] += d * a.w;
        acc[4] += d * b.x; acc[5] += d * b.y; acc[6] += d * b.z; acc[7] += d * b.w;
      }
      *reinterpret_cast<uint4*>(dx + (size_t)r * H + h0) = pack8bf(acc);
    }
  }
}

// dw[t,h] += sum_r de[r,t] * x[r,h] ; db[t] += sum_r de[r,t]
// grid = (ceil(H/256), ceil(R/64)); thread owns column h; 64 rows of de staged in LDS.
// TMAX (32 for T <= 32: the 29 tags of the KB-NER dictionaries; 64 otherwise): the staged rows have a FIXED stride of TMAX floats,
// zero-padded behind T, so that a row's tag values leave LDS as TMAX / 4 broadcast ds_read_b128 and the tag loop is straight-line code
// (round 6: with the runtime stride T the compiler issued one ds_read_b32 per (row, tag) and waited for each -- 1856 exposed LDS
// latencies per block, 110 us per launch whatever the batch, 0.9 % of a 4-sentence optimizer step).
// RB rows per block: 64, or 16 when there are few rows (round 6: 64 kept tokens on 4 workgroups were 64 dependent rounds each, 31 us).
template <int TMAX, int RB = 64>
__global__ __launch_bounds__(256) void head_bwd_dw_kernel(const float* __restrict__ de, const bf16_t* __restrict__ x,
                                                          float* __restrict__ dw, float* __restrict__ db, int R, int H, int T) {
  __shared__ __attribute__((aligned(16))) float sde[RB * TMAX];
  const int h = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * RB;
  const int nr = min(RB, R - r0);
  for (int i = threadIdx.x; i < RB * TMAX; i += 256) {
    const int r = i / TMAX, t = i % TMAX;
    sde[i] = (r < nr && t < T) ? de[(size_t)(r0 + r) * T + t] : 0.0f;
  }
  __syncthreads();
  float acc[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) acc[t] = 0.0f;
  if (h < H) {
    for (int r = 0; r < nr; ++r) {
      const float xv = bf2f(x[(size_t)(r0 + r) * H + h]);
#pragma unroll
      for (int t4 = 0; t4 < TMAX / 4; ++t4) {
        const float4 d = *reinterpret_cast<const float4*>(&sde[r * TMAX + t4 * 4]);
        acc[t4 * 4 + 0] += d.x * xv;
        acc[t4 * 4 + 1] += d.y * xv;
        acc[t4 * 4 + 2] += d.z * xv;
        acc[t4 * 4 + 3] += d.w * xv;
      }
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t < T) atomicAdd(dw + (size_t)t * H + h, acc[t]);
  }
  if (blockIdx.x == 0 && threadIdx.x < T) {
    float s = 0.0f;
    for (int r = 0; r < nr; ++r) s += sde[r * TMAX + threadIdx.x];
    atomicAdd(db + threadIdx.x, s);
  }
}

// The same for T > HEAD_MAXT (tag sets of 65 to 192 tags): blockIdx.z walks the tags in blocks of HEAD_MAXT; a block stages and
// accumulates its own HEAD_MAXT tags (zero-padded behind T) and adds its own rows of dw and entries of db, so every db[t] still
// receives one add per row block.  A kernel of its own, so that the instantiations above stay what they were, to the byte.
__global__ __launch_bounds__(256) void head_bwd_dw_blk_kernel(const float* __restrict__ de, const bf16_t* __restrict__ x,
                                                              float* __restrict__ dw, float* __restrict__ db, int R, int H, int T) {
  constexpr int TMAX = HEAD_MAXT, RB = 64;
  __shared__ __attribute__((aligned(16))) float sde[RB * TMAX];
  const int h = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * RB;
  const int nr = min(RB, R - r0);
  const int t0 = blockIdx.z * TMAX;
  for (int i = threadIdx.x; i < RB * TMAX; i += 256) {
    const int r = i / TMAX, t = i % TMAX;
    sde[i] = (r < nr && t0 + t < T) ? de[(size_t)(r0 + r) * T + t0 + t] : 0.0f;
  }
  __syncthreads();
  float acc[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) acc[t] = 0.0f;
  if (h < H) {
    for (int r = 0; r < nr; ++r) {
      const float xv = bf2f(x[(size_t)(r0 + r) * H + h]);
#pragma unroll
      for (int t4 = 0; t4 < TMAX / 4; ++t4) {
        const float4 d = *reinterpret_cast<const float4*>(&sde[r * TMAX + t4 * 4]);
        acc[t4 * 4 + 0] += d.x * xv;
        acc[t4 * 4 + 1] += d.y * xv;
        acc[t4 * 4 + 2] += d.z * xv;
        acc[t4 * 4 + 3] += d.w * xv;
      }
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t0 + t < T) atomicAdd(dw + (size_t)(t0 + t) * H + h, acc[t]);
  }
  if (blockIdx.x == 0 && threadIdx.x < TMAX && t0 + threadIdx.x < T) {
    float s = 0.0f;
    for (int r = 0; r < nr; ++r) s += sde[r * TMAX + threadIdx.x];
    atomicAdd(db + t0 + threadIdx.x, s);
  }
}

extern "C" {
int kbner_head_fwd(const bf16_t* x, const float* w, const float* bias, float* out, int R, int H, int T, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0 && H <= 8192 && T > 0 && T <= HEAD_WIDE_MAXT);
  if (R == 0) return 0;
  if (H <= HEAD_MAXH && R <= 512)
    hipLaunchKernelGGL(head_fwd_rt_kernel, dim3((R * T + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, w, bias, out, R, H, T);
  else if (H <= HEAD_MAXH)
    hipLaunchKernelGGL(head_fwd_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, x, w, bias, out, R, H, T);
  else   // the BiLSTM tagger head of config 5: 2 x 1024 (padded) hidden columns
    hipLaunchKernelGGL(head_fwd_wide_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, x, w, bias, out, R, H, T);
  KBNER_LAUNCH_RET();
}

int kbner_head_bwd_dx(const float* de, const float* w, bf16_t* dx, int R, int H, int T, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0 && H <= 8192 && T > 0 && T <= HEAD_WIDE_MAXT);
  if (R == 0) return 0;
  if (H <= HEAD_MAXH)
    hipLaunchKernelGGL(head_bwd_dx_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, de, w, dx, R, H, T);
  else
    hipLaunchKernelGGL(head_bwd_dx_wide_kernel, dim3(rows_grid(R)), dim3(256), 0, (hipStream_t)stream, de, w, dx, R, H, T);
  KBNER_LAUNCH_RET();
}

int kbner_head_bwd_dw(const float* de, const bf16_t* x, float* dw, float* db, int R, int H, int T, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && T > 0 && T <= HEAD_WIDE_MAXT);
  if (R == 0) return 0;
  if (T <= 32 && R <= 512)
    hipLaunchKernelGGL((head_bwd_dw_kernel<32, 16>), dim3((H + 255) / 256, (R + 15) / 16), dim3(256), 0, (hipStream_t)stream, de, x, dw,
                       db, R, H, T);
  else if (T <= 32)
    hipLaunchKernelGGL(head_bwd_dw_kernel<32>, dim3((H + 255) / 256, (R + 63) / 64), dim3(256), 0, (hipStream_t)stream, de, x, dw,
                       db, R, H, T);
  else if (T <= HEAD_MAXT)
    hipLaunchKernelGGL(head_bwd_dw_kernel<HEAD_MAXT>, dim3((H + 255) / 256, (R + 63) / 64), dim3(256), 0, (hipStream_t)stream, de, x,
                       dw, db, R, H, T);
  else
    hipLaunchKernelGGL(head_bwd_dw_blk_kernel, dim3((H + 255) / 256, (R + 63) / 64, (T + HEAD_MAXT - 1) / HEAD_MAXT), dim3(256), 0,
                       (hipStream_t)stream, de, x, dw, db, R, H, T);
  KBNER_LAUNCH_RET();
}
}  // extern "C"

// ---- column sums

// out[n] += sum_m x[m,n]   (bf16 in, fp32 atomics out).  Block = 64 column-threads (16-byte loads, 512 columns)
// x 4 row-threads; the 4 row partials are combined in LDS so a block issues one atomic per column.
// grid = (ceil(N/512), ceil(M/rows_per_block))
__global__ __launch_bounds__(256) void colsum_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, int M, int N,
                                                     int ld, int rows_per_block) {
  __shared__ float red[4][512];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 64 + tx) * 8;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
  if (n0 < N) {
#pragma unroll 4
    for (int r = r0 + ty; r < r1; r += 4) {
      float f[8];
      unpack8bf(*reinterpret_cast<const uint4*>(x + (size_t)r * ld + n0), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ty][tx * 8 + j] = acc[j];
  __syncthreads();
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int n = blockIdx.x * 512 + c;
    if (n < N) atomicAdd(out + n, (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]));
  }
}

// out[n] += sum_r ws[r, n]: folds the per-(tile row, wave row) column sums a GEMM launched with KBNER_EPI_COLSUM_WS left in
// its workspace (rows = 2 * M / 256).  Two deterministic passes of one kernel: grid (ceil(N / 256), rows / chunk) blocks each
// fold `chunk` consecutive rows IN PLACE into the first row of their chunk (a block reads only its own chunk), then one row of
// blocks folds those first rows into out.  (A single pass with 16 blocks ran at 150 GB/s: 55 us for 8 MB.)
// block 256 columns x 4 row-lanes.
// What the two fold kernels share: a block is 256 columns x 4 row-lanes (COLSUM_FOLD_BLOCK: tx, ty, column n); lane ty sums ELEM
// (an expression in i and n) over the rows i = ty, ty + 4, ... < count into part[ty]; after the barrier COLSUM_FOLD_TOTAL is the
// column's sum, for its owner (ty == 0 && n < N) to store.  Macros: as inline functions (the row pointer an argument), or with
// the statements between them moved, the kernels' instruction streams change.
#define COLSUM_FOLD_BLOCK                                  \
  __shared__ float part[4][256];                           \
  const int tx = threadIdx.x & 255, ty = threadIdx.x >> 8; \
  const int n = blockIdx.x * 256 + tx
#define COLSUM_FOLD_LANES(count, ELEM)                     \
  float acc = 0.0f;                                        \
  if (n < N)                                               \
    for (int i = ty; i < count; i += 4) acc += ELEM;       \
  part[ty][tx] = acc;                                      \
  __syncthreads()
#define COLSUM_FOLD_TOTAL ((part[0][tx] + part[1][tx]) + (part[2][tx] + part[3][tx]))
__global__ __launch_bounds__(1024) void colsum_fold_kernel(float* __restrict__ ws, int first_stride, int stride, int count, int N,
                                                           float* __restrict__ out) {
  COLSUM_FOLD_BLOCK;
  float* base = ws + (size_t)blockIdx.y * first_stride * N;
  COLSUM_FOLD_LANES(count, base[(size_t)i * stride * N + n]);
  if (ty == 0 && n < N) {
    const float t = COLSUM_FOLD_TOTAL;
    if (out != nullptr) out[n] += t;
    else base[n] = t;
  }
}

// The single-pass fold for up to COLSUM_BATCH_MAX workspaces of one width in ONE launch (blockIdx.y picks the item): the FFN-up bias
// gradients of all layers at the end of a small-batch backward pass instead of one 4.8-us launch per layer.  Same summation order
// per column as the single pass above.
#define COLSUM_BATCH_MAX 64
struct ColsumItem {
  const float* ws;
  float* out;
  long long rows;
};
struct ColsumBatch {
  ColsumItem it[COLSUM_BATCH_MAX];
};
__global__ __launch_bounds__(1024) void colsum_fold_batched_kernel(const ColsumBatch batch, int N) {
  const ColsumItem& q = batch.it[blockIdx.y];
  COLSUM_FOLD_BLOCK;
  const int count = (int)q.rows;
  COLSUM_FOLD_LANES(count, q.ws[(size_t)i * N + n]);
  if (ty == 0 && n < N) q.out[n] += COLSUM_FOLD_TOTAL;
}

extern "C" {
int kbner_colsum(const bf16_t* x, float* out, int M, int N, int ld, void* stream) {
  KBNER_CHECK_ARG(M >= 0 && N > 0 && N % 8 == 0 && ld >= N && ld % 8 == 0);
  if (M == 0) return 0;
  int rpb = 128;
  hipLaunchKernelGGL(colsum_kernel, dim3((N + 511) / 512, (M + rpb - 1) / rpb), dim3(256), 0, (hipStream_t)stream, x, out,
                     M, N, ld, rpb);
  KBNER_LAUNCH_RET();
}

int kbner_colsum_rows_f32(float* ws, int rows, int N, float* out, void* stream) {
  KBNER_CHECK_ARG(ws != nullptr && out != nullptr && rows > 0 && N > 0);
  const int chunk = 16;
  const dim3 gx((N + 255) / 256);
  // (two passes only when there are enough partial rows to be worth a second launch: at 4 sentences per step the workspace has 32 rows
  // and the second launch was half of this call's 9.6 us, 48 times per step)
  if (rows > 4 * chunk && rows % chunk == 0) {
    hipLaunchKernelGGL(colsum_fold_kernel, dim3(gx.x, rows / chunk), dim3(1024), 0, (hipStream_t)stream, ws, chunk, 1, chunk, N,
                       (float*)nullptr);
    hipLaunchKernelGGL(colsum_fold_kernel, gx, dim3(1024), 0, (hipStream_t)stream, ws, 0, chunk, rows / chunk, N, out);
  } else {
    hipLaunchKernelGGL(colsum_fold_kernel, gx, dim3(1024), 0, (hipStream_t)stream, ws, 0, 1, rows, N, out);
  }
  KBNER_LAUNCH_RET();
}

// items (HOST memory, n <= 64 records of 3 x 64 bits: ws, out -- device pointers -- and the number of rows): out[c] += sum_r ws[r, c]
int kbner_colsum_rows_f32_batched(const long long* items, int n, int N, void* stream) {
  KBNER_CHECK_ARG(items != nullptr && n >= 0 && n <= COLSUM_BATCH_MAX && N > 0);
  if (n == 0) return 0;
  ColsumBatch b;
  for (int i = 0; i < n; ++i) {
    b.it[i].ws = reinterpret_cast<const float*>(items[3 * i]);
    b.it[i].out = reinterpret_cast<float*>(items[3 * i + 1]);
    b.it[i].rows = items[3 * i + 2];
    KBNER_CHECK_ARG(b.it[i].ws != nullptr && b.it[i].out != nullptr && b.it[i].rows > 0);
  }
  for (int i = n; i < COLSUM_BATCH_MAX; ++i) b.it[i] = b.it[0];
  hipLaunchKernelGGL(colsum_fold_batched_kernel, dim3((N + 255) / 256, n), dim3(1024), 0, (hipStream_t)stream, b, N);
  KBNER_LAUNCH_RET();
}
}  // extern "C"

// ---- split-K finish

// Split-K finish: C[m,n] = bf16( dropout( sum_s ws[s][m][n] + bias[n] ) + addend[m,n] ).  The forward / dgrad GEMMs of a small
// micro-batch have a few dozen 256x256 tiles, each a serial chain of K/64 DMA round trips; splitting a long K over up to 4
// workgroups (fp32 slabs written with plain stores by KBNER_EPI_STORE32) shortens that chain, this pass folds the slabs.
__global__ __launch_bounds__(256) void splitk_finish_kernel(const float* __restrict__ ws, int splits, size_t slab, const float* __restrict__ bias,
                                                            const bf16_t* __restrict__ addend, int ldadd, bf16_t* __restrict__ C, int ldc, int M,
                                                            int N, uint32_t drop_seed, uint32_t drop_thresh) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;  // 8 consecutive columns per thread
  if (i >= (size_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  *reinterpret_cast<uint4*>(C + (size_t)m * ldc + n) = splitk_fold8_pack(ws, splits, slab, bias, addend, ldadd, m, n, N, drop_seed, drop_thresh);
}

extern "C" int kbner_splitk_finish(const float* ws, int splits, const float* bias, const bf16_t* addend, int ldadd, bf16_t* C, int ldc,
                                   int M, int N, uint32_t drop_seed, uint32_t drop_thresh, void* stream) {
  KBNER_CHECK_ARG(ws != nullptr && C != nullptr && splits >= 1 && splits <= 8 && M > 0 && N > 0 && N % 8 == 0 && ldc % 8 == 0);
  KBNER_CHECK_ARG(addend == nullptr || ldadd % 8 == 0);
  FLAT_LAUNCH(splitk_finish_kernel, (size_t)M * N / 8, stream, ws, splits, (size_t)M * N, bias, addend, ldadd, C, ldc, M, N, drop_seed,
              drop_thresh);
  KBNER_LAUNCH_RET();
}

// Hidden dropout on COMPACT rows (the last encoder layer computed at the tagger head's rows only): row r of y stands for row
// row_ids[r] of the full [tokens, H] hidden state, and draws that row's mask -- the bits the GEMM epilogue / kbner_ln_bwd draw
// for it in the full path:
//     out[r,:] = bf16( keep(row_ids[r], c) ? (y[r,c] + bias[c]) / (1-p) : 0  (+ addend[r,c]) )
// y is fp32 (the compact GEMM's fp32 output, so the value is rounded once, as in the fused epilogue) or bf16.  The backward of
// these sites is kbner_ln_bwd_rows (csrc/layernorm.hip), which masks the fp32 dh.  8 columns per thread.
template <typename TY>
__global__ __launch_bounds__(256) void rows_drop_add_kernel(const TY* __restrict__ y, const float* __restrict__ bias,
                                                            const bf16_t* __restrict__ addend, const int* __restrict__ row_ids,
                                                            bf16_t* __restrict__ out, int R, int H, uint32_t seed, uint32_t thresh) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= (size_t)R * H) return;
  const int r = (int)(i / H), c = (int)(i % H);
  float v[8];
  if constexpr (sizeof(TY) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(y + i), b = *reinterpret_cast<const float4*>(y + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    unpack8bf(*reinterpret_cast<const uint4*>(y + i), v);
  }
  if (bias) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += bias[c + j];
  }
  const int row = row_ids[r];
  if (thresh && row >= 0) {
    const uint32_t rk = drop_rowkey(seed, (uint32_t)row);
    const float ds = drop_scale(thresh);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = drop_keep(rk, drop_colkey(seed, (uint32_t)(c + j)), thresh) ? v[j] * ds : 0.0f;
  }
  if (addend) {
    float a[8];
    unpack8bf(*reinterpret_cast<const uint4*>(addend + i), a);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += a[j];
  }
  *reinterpret_cast<uint4*>(out + i) = pack8bf(v);
}

extern "C" int kbner_rows_drop_add(const void* y, int y_is_f32, const float* bias, const bf16_t* addend, const int* row_ids, bf16_t* out,
                                   int R, int H, uint32_t drop_seed, uint32_t drop_thresh, void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 8 == 0);
  if (R == 0) return 0;
  KBNER_CHECK_ARG(y != nullptr && row_ids != nullptr && out != nullptr);
  if (y_is_f32)
    FLAT_LAUNCH(rows_drop_add_kernel<float>, (size_t)R * H / 8, stream, static_cast<const float*>(y), bias, addend, row_ids, out, R, H,
                drop_seed, drop_thresh);
  else
    FLAT_LAUNCH(rows_drop_add_kernel<bf16_t>, (size_t)R * H / 8, stream, static_cast<const bf16_t*>(y), bias, addend, row_ids, out, R, H,
                drop_seed, drop_thresh);
  KBNER_LAUNCH_RET();
}

// ---- the rest

// Multi-view training's representation term (FastSequenceTagger._calculate_multi_view_loss with calculate_l2_loss,
// sequence_tagger_model.py:1988-1996,2026-2035): mse_loss(orig view's token representations, the context view's (detached)) at the
// sentence's real tokens, forward and backward in one pass over the rows:
//     loss += sum_r w[r] * sum_h (a[r,h] - b[r,h])^2 ;   da[r,:] += 2 * gscale * w[r] * (a[r,:] - b[r,:])
// (w[r] = sentence weight / H, 0 for padding rows; da is the bf16 gradient of the pooled rows the head's backward just wrote).
// One wavefront per row.
__global__ __launch_bounds__(256) void l2_rows_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b,
                                                      const float* __restrict__ w, float gscale, bf16_t* __restrict__ da,
                                                      float* __restrict__ loss, int R, int H) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const float wr = w[r];
  if (wr == 0.0f) return;
  const bf16_t* ar = a + (size_t)r * H;
  const bf16_t* br = b + (size_t)r * H;
  bf16_t* dr = da + (size_t)r * H;
  float acc = 0.0f;
  for (int h = lane * 2; h < H; h += 128) {
    const f2v x = unpack2bf(*reinterpret_cast<const uint32_t*>(ar + h));
    const f2v y = unpack2bf(*reinterpret_cast<const uint32_t*>(br + h));
    const float d0 = x[0] - y[0], d1 = x[1] - y[1];
    acc += d0 * d0 + d1 * d1;
    if (da != nullptr) {
      const f2v g = unpack2bf(*reinterpret_cast<const uint32_t*>(dr + h));
      *reinterpret_cast<uint32_t*>(dr + h) = pack2bf(g[0] + 2.0f * gscale * wr * d0, g[1] + 2.0f * gscale * wr * d1);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) atomicAdd(loss, wr * acc);
}

// Materialise a dropout site's multiplier (tests / debugging only: the product kernels regenerate it in registers):
// out[z,i,j] = drop_keep(rowkey(seed, z*M+i), colkey(seed, z*N+j)) ? 1/(1-p) : 0.  Hidden-state sites: Z=1, [M tokens, H];
// attention-probability sites: Z = B*A heads, M = N = S.
__global__ __launch_bounds__(256) void dropout_mask_kernel(float* __restrict__ out, int Z, int M, int N, uint32_t seed,
                                                           uint32_t thresh) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)Z * M * N) return;
  const int j = (int)(i % N);
  const int r = (int)((i / N) % M);
  const int z = (int)(i / ((size_t)M * N));
  const bool keep = drop_keep(drop_rowkey(seed, (uint32_t)(z * M + r)), drop_colkey(seed, (uint32_t)(z * N + j)), thresh);
  out[i] = keep ? drop_scale(thresh) : 0.0f;
}

extern "C" {
int kbner_l2_rows(const bf16_t* a, const bf16_t* b, const float* w, float gscale, bf16_t* da, float* loss, int R, int H,
                             void* stream) {
  KBNER_CHECK_ARG(R >= 0 && H > 0 && H % 2 == 0);
  if (R == 0) return 0;
  KBNER_CHECK_ARG(a != nullptr && b != nullptr && w != nullptr && loss != nullptr);
  hipLaunchKernelGGL(l2_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, b, w, gscale, da, loss, R,
                     H);
  KBNER_LAUNCH_RET();
}

int kbner_dropout_mask(float* out, int Z, int M, int N, uint32_t seed, uint32_t thresh, void* stream) {
  KBNER_CHECK_ARG(out != nullptr && Z > 0 && M > 0 && N > 0);
  FLAT_LAUNCH(dropout_mask_kernel, (size_t)Z * M * N, stream, out, Z, M, N, seed, thresh);
  KBNER_LAUNCH_RET();
}
}  // extern "C"
