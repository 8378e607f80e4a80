// Linear-chain CRF kernels for tag sets wider than one wavefront (T <= 192): Viterbi decode, forward-algorithm NLL, its analytic
// backward and the token marginals.  csrc/crf.hip puts one tag on one lane of a single 64-lane wave and broadcasts the running
// score vector with v_readlane; here one WORKGROUP of TT = 64, 128 or 192 threads takes a sentence and thread t owns the "to"
// tag t:
//   - thread t keeps row t of the transition matrix ([to,from]) in TT registers for the whole scan, as csrc/crf.hip does
//     (entries behind T hold -inf: they never win a max and add exp(-inf) = 0 to a sum);
//   - the running score vector is exchanged through a double-buffered [2][TT] LDS array, read back as broadcast 16-byte loads,
//     with ONE __syncthreads() per step: a step reads buffer `cur` and writes buffer `cur ^ 1`, and nobody writes `cur` again
//     before every thread has passed the next barrier;
//   - the backward scan also needs COLUMN t (beta_i[from] sums over `to`): the matrix lives in LDS once, fp32, with the odd row
//     stride S = T | 1, read down a column -- consecutive lanes, consecutive banks.  Rows in registers (192) next to the
//     transition-gradient accumulator (192) fill the 512-register file of a wave that has a SIMD to itself, and 192 * 193 floats
//     are 148 224 B of the CU's 160 KiB: that is where the limit of 192 tags comes from.
// The f loops are unrolled over TT with compile-time register indices and walk 16 tags at a time under a workgroup-uniform
// `f0 < T`, so T = 137 does the work of 144 tags, not of 192.
//
// Barriers sit inside the scan loops, so (a) the trip count is the sentence's length, uniform over the workgroup, (b) the
// padding threads t >= T run every loop and reach every barrier: their values are masked (-inf rows, -1e12 scores), never
// their control flow, and they store to LDS only, (c) every index is in range for lens[b] = 0 and n = 0.
//
// Reference semantics restated (never copied), the call sites csrc/crf.hip cites:
//   _viterbi_decode   sequence_tagger_model.py:1248-1327
//   _forward_alg      sequence_tagger_model.py:1329-1394
//   _score_sentence   sequence_tagger_model.py:2544-2591
//   _backward_alg     sequence_tagger_model.py:1396-1470
// This file is compiled WITHOUT fast-math: Viterbi must reproduce the reference's fp32 adds bit-for-bit
// ((v[f] + trans[t,f]) -> first max over f -> + emit[t]).
#include "common.h"

#define CRFW_NEG (-1e12f)
#define CRFW_MAXT 192
#define CRFW_MAXW (CRFW_MAXT / 64)
#define CRFW_CHUNK 16          // tags per uniform guard of the unrolled f loops
#define CRFW_BP_BYTES 32768    // LDS staging area of the Viterbi backtrace

// whole-workgroup reductions through `sred` (CRFW_MAXW floats): every thread of the workgroup calls them
static __device__ __forceinline__ float crfw_block_sum(float v, float* sred) {
  v = wave_sum(v);
  __syncthreads();  // the previous reduction's readers are done with sred
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.0f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += sred[w];
  return r;
}
static __device__ __forceinline__ float crfw_block_max(float v, float* sred) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sred[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, sred[w]);
  return r;
}

static __device__ __forceinline__ int crfw_len(const int* __restrict__ lens, int b, int n) { return min(max(lens[b], 0), n); }

// row t of trans in registers, -inf behind T and on the padding threads
template <int TT>
static __device__ __forceinline__ void crfw_load_row(float (&row)[TT], const float* __restrict__ trans, int T, int t) {
  const bool live = t < T;
#pragma unroll
  for (int f = 0; f < TT; ++f) row[f] = (live && f < T) ? trans[t * T + f] : -INFINITY;
}

// ------------------------------------------------------------------------------------------
// Viterbi.  The scores v'_i (fp32) and the backpointers (u8, T <= 192) go to the workspace in global memory, so the sentence
// length is bounded by the workspace alone.  The backtrace stages the backpointers through LDS in chunks (one coalesced copy,
// then dependent LDS reads instead of dependent HBM reads).
// ------------------------------------------------------------------------------------------
template <int TT>
__global__ __launch_bounds__(TT) void crfw_viterbi_kernel(const float* __restrict__ emit, const float* __restrict__ trans,
                                                          const int* __restrict__ lens, int n, int T, int start, int stop,
                                                          int* __restrict__ tags, float* __restrict__ conf, int* __restrict__ popped,
                                                          float* __restrict__ wsv, unsigned char* __restrict__ wsb) {
  __shared__ __attribute__((aligned(16))) float sv[2][TT];
  __shared__ __attribute__((aligned(16))) uint32_t sbp[CRFW_BP_BYTES / 4];
  __shared__ float sredv[CRFW_MAXW];
  __shared__ int sredi[CRFW_MAXW];
  const int b = blockIdx.x;
  const int t = threadIdx.x;  // blockDim.x == TT
  const int L = crfw_len(lens, b, n);
  const bool live = t < T;
  float row[TT];
  crfw_load_row<TT>(row, trans, T, t);
  const float tstop = live ? trans[stop * T + t] : 0.0f;
  float vcur = (t == start) ? 0.0f : CRFW_NEG;
  sv[0][t] = vcur;
  int* tg = tags + (size_t)b * n;
  float* cf = conf + (size_t)b * n;
  for (int i = L + t; i < n; i += TT) {
    tg[i] = -1;
    cf[i] = 0.0f;
  }
  const float* e = emit + (size_t)b * n * T;
  float* wv = wsv + (size_t)b * n * T;
  unsigned char* wb = wsb + (size_t)b * n * T;
  float enext = (live && L > 0) ? e[t] : 0.0f;
  __syncthreads();
  int cur = 0;
  for (int i = 0; i < L; ++i) {
    const float et = enext;
    if (live && i + 1 < L) enext = e[(size_t)(i + 1) * T + t];
    const float4* v4 = reinterpret_cast<const float4*>(sv[cur]);
    float best = 0.0f;
    int arg = 0;
#pragma unroll
    for (int f0 = 0; f0 < TT; f0 += CRFW_CHUNK) {
      if (f0 < T) {
#pragma unroll
        for (int q = 0; q < CRFW_CHUNK / 4; ++q) {
          const float4 vv = v4[f0 / 4 + q];
          const float vs[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = f0 + 4 * q + j;
            const float c = vs[j] + row[f];
            if (f == 0) {
              best = c;
            } else if (c > best) {  // strict: first maximal index wins, as torch.max(dim) on CPU
              best = c;
              arg = f;
            }
          }
        }
      }
    }
    const float vnew = best + et;
    if (live) {
      wb[(size_t)i * T + t] = (unsigned char)arg;
      wv[(size_t)i * T + t] = vnew;
      vcur = vnew;
    }
    sv[cur ^ 1][t] = live ? vnew : CRFW_NEG;
    __syncthreads();
    cur ^= 1;
  }
  // terminal (:1279-1287): + trans[STOP,:], then STOP and START entries forced to -1e12; FIRST maximal index over the workgroup
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  if (live) {
    bv = vcur + tstop;
    if (t == stop || t == start) bv = CRFW_NEG;
    bi = t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((t & 63) == 0) {
    sredv[t >> 6] = bv;
    sredi[t >> 6] = bi;
  }
  __syncthreads();  // also: the workspace rows written above are visible to the whole workgroup
  bv = sredv[0];
  bi = sredi[0];
  for (int w = 1; w < TT / 64; ++w)
    if (sredv[w] > bv) {  // waves hold ascending tag ranges: strict keeps the first maximal index
      bv = sredv[w];
      bi = sredi[w];
    }
  // confidence of token i = max(softmax(v'_i)) = 1 / sum_t exp(v'_i[t] - max_t v'_i[t])   (:1295-1300): one wave per token,
  // coalesced over the tags
  {
    const int lane = t & 63;
    for (int i = t >> 6; i < L; i += TT / 64) {
      const float* v = wv + (size_t)i * T;
      float m = -INFINITY;
      for (int k = lane; k < T; k += 64) m = fmaxf(m, v[k]);
      m = wave_max(m);
      float sum = 0.0f;
      for (int k = lane; k < T; k += 64) sum += expf(v[k] - m);
      sum = wave_sum(sum);
      if (lane == 0) cf[i] = 1.0f / sum;
    }
  }
  // backtrace, last chunk first: rows [lo, hi) of the backpointers are copied as dwords from the 4-byte boundary at or below
  // their first byte (the workspace is 16-byte aligned and padded to 16 bytes, so both ends stay inside it)
  const unsigned char* sb = reinterpret_cast<const unsigned char*>(sbp);
  const int CH = (CRFW_BP_BYTES - 8) / T;  // rows whose bytes, plus 3 of misalignment and 3 of dword rounding, fit in sbp (>= 170)
  int best = bi;
  for (int hi = L; hi > 0; hi -= CH) {
    const int lo = max(hi - CH, 0);
    const uintptr_t g0 = reinterpret_cast<uintptr_t>(wb + (size_t)lo * T);
    const uintptr_t a0 = g0 & ~(uintptr_t)3;
    const int shift = (int)(g0 - a0);
    const int ndw = (shift + (hi - lo) * T + 3) >> 2;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a0);
    for (int k = t; k < ndw; k += TT) sbp[k] = src[k];
    __syncthreads();
    if (t == 0) {
      for (int i = hi - 1; i >= lo; --i) {
        tg[i] = best;
        best = sb[shift + (i - lo) * T + best];
      }
    }
    __syncthreads();
  }
  if (t == 0 && popped) popped[b] = (L > 0) ? best : start;  // the reference asserts this == START (:1302-1303)
}

// ------------------------------------------------------------------------------------------
// NLL forward: logZ (forward algorithm), gold path score, alpha saved for backward
// ------------------------------------------------------------------------------------------
template <int TT>
__global__ __launch_bounds__(TT) void crfw_nll_fwd_kernel(const float* __restrict__ emit, const float* __restrict__ trans,
                                                          const int* __restrict__ tags, const int* __restrict__ lens, int n, int T,
                                                          int start, int stop, float* __restrict__ logz, float* __restrict__ gold,
                                                          float* __restrict__ alpha) {
  __shared__ __attribute__((aligned(16))) float sv[2][TT];
  __shared__ float sred[CRFW_MAXW];
  const int b = blockIdx.x;
  const int t = threadIdx.x;  // blockDim.x == TT
  const int L = crfw_len(lens, b, n);
  const bool live = t < T;
  float row[TT];
  crfw_load_row<TT>(row, trans, T, t);
  const float tstop = live ? trans[stop * T + t] : 0.0f;
  const float* e = emit + (size_t)b * n * T;
  float* al = alpha + (size_t)b * (n + 1) * T;
  float acur = (t == start) ? 0.0f : CRFW_NEG;
  if (live) al[t] = acur;
  sv[0][t] = acur;
  float enext = (live && L > 0) ? e[t] : 0.0f;
  __syncthreads();
  int cur = 0;
  for (int i = 0; i < L; ++i) {
    const float et = enext;
    if (live && i + 1 < L) enext = e[(size_t)(i + 1) * T + t];
    const float4* v4 = reinterpret_cast<const float4*>(sv[cur]);
    // tag_var[t,f] = (emit[t] + trans[t,f]) + alpha[f]   (:1361-1367, that association)
    float x[TT];
    float m = -INFINITY;
#pragma unroll
    for (int f0 = 0; f0 < TT; f0 += CRFW_CHUNK) {
      if (f0 < T) {
#pragma unroll
        for (int q = 0; q < CRFW_CHUNK / 4; ++q) {
          const float4 vv = v4[f0 / 4 + q];
          const float vs[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = f0 + 4 * q + j;
            x[f] = (et + row[f]) + vs[j];
            m = fmaxf(m, x[f]);
          }
        }
      }
    }
    float s = 0.0f;
#pragma unroll
    for (int f0 = 0; f0 < TT; f0 += CRFW_CHUNK) {
      if (f0 < T) {
#pragma unroll
        for (int f = f0; f < f0 + CRFW_CHUNK; ++f) s += __expf(x[f] - m);
      }
    }
    const float anew = m + logf(s);
    if (live) {
      al[(size_t)(i + 1) * T + t] = anew;
      acur = anew;
    }
    sv[cur ^ 1][t] = live ? anew : CRFW_NEG;
    __syncthreads();
    cur ^= 1;
  }
  // terminal: lse(alpha_L + trans[STOP,:])   (:1383-1393)
  const float term = live ? acur + tstop : -INFINITY;
  const float m = crfw_block_max(term, sred);
  const float s = crfw_block_sum(live ? __expf(term - m) : 0.0f, sred);
  // gold path score (:2544-2591) on compacted rows: mask[k] = k < L
  const int* tg = tags + (size_t)b * n;
  float g = 0.0f;
  for (int k = t; k < L; k += TT) {
    const int tk = tg[k];
    const int prev = (k == 0) ? start : tg[k - 1];
    g += e[(size_t)k * T + tk] + trans[tk * T + prev];
  }
  g = crfw_block_sum(g, sred);
  if (t == 0) {
    const int last = (L > 0) ? tg[L - 1] : start;
    logz[b] = m + logf(s);
    gold[b] = g + trans[stop * T + last];
  }
}

// ------------------------------------------------------------------------------------------
// NLL backward: d/d emit and d/d trans of sum_b dloss[b] * (logZ_b - gold_b); POSTERIOR = true: the token marginals instead
// (the predict_posterior branch of _obtain_labels, :1182-1192), tags / dloss / dtrans unused.
// Thread t keeps row t of the transitions AND its row of the transition-gradient accumulator in registers (2 x TT compile-time
// indexed values, one wave per SIMD); the accumulator is added to dtrans with fp32 global atomics at the end as csrc/crf.hip does.
// Three vectors per step go through LDS, double-buffered: alpha_i, emit_i and beta_{i+1}; step i stages those of step i - 1
// before its barrier, so a step has one barrier.  Dynamic LDS: strans[T * S] (rounded up to 4 floats), then svec[2][3][TT].
// ------------------------------------------------------------------------------------------
static __host__ __device__ __forceinline__ int crfw_stride(int T) { return T | 1; }
static __host__ __device__ __forceinline__ int crfw_trans_floats(int T) { return (T * crfw_stride(T) + 3) & ~3; }

template <int TT, bool POSTERIOR>
__global__ __launch_bounds__(TT) void crfw_nll_bwd_kernel(const float* __restrict__ emit, const float* __restrict__ trans,
                                                          const int* __restrict__ tags, const int* __restrict__ lens,
                                                          const float* __restrict__ alpha, const float* __restrict__ logz,
                                                          const float* __restrict__ dloss, int n, int T, int start, int stop,
                                                          float* __restrict__ demit, float* __restrict__ dtrans) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = crfw_stride(T);
  float* strans = smem;
  float* svec = smem + crfw_trans_floats(T);  // [2][3][TT]: alpha_i, emit_i, beta_{i+1}
  const int b = blockIdx.x;
  const int t = threadIdx.x;  // blockDim.x == TT
  const int L = crfw_len(lens, b, n);
  const bool live = t < T;
  const int tt = live ? t : T - 1;
  const float w = POSTERIOR ? 1.0f : dloss[b];
  const float lz = logz[b];
  for (int idx = t; idx < T * T; idx += TT) {
    const int r = idx / T;
    strans[r * S + (idx - r * T)] = trans[idx];
  }
  float row[TT];
  crfw_load_row<TT>(row, trans, T, t);
  float dacc[POSTERIOR ? 1 : TT];  // d trans[t,:]
  if (!POSTERIOR) {
#pragma unroll
    for (int f = 0; f < TT; ++f) dacc[f] = 0.0f;
  }
  const float* e = emit + (size_t)b * n * T;
  const float* al = alpha + (size_t)b * (n + 1) * T;
  float* de = demit + (size_t)b * n * T;
  const int* tg = POSTERIOR ? nullptr : tags + (size_t)b * n;
  for (size_t i = (size_t)L * T + t; i < (size_t)n * T; i += TT) de[i] = 0.0f;
  // beta_L = trans[STOP,:]; terminal marginal d trans[STOP, t] (kept by thread t, added at the end)
  float beta = live ? trans[stop * T + t] : CRFW_NEG;
  const float dstop = live ? w * __expf(al[(size_t)L * T + t] + beta - lz) : 0.0f;
  float ai = (live && L > 0) ? al[(size_t)(L - 1) * T + t] : CRFW_NEG;
  float ei = (live && L > 0) ? e[(size_t)(L - 1) * T + t] : 0.0f;
  svec[t] = ai;  // the padding threads keep the slots behind T at (-1e12, 0, -1e12): finite, and nothing under exp
  svec[TT + t] = ei;
  svec[2 * TT + t] = beta;
  const float* col = strans + tt;
  __syncthreads();
  int cur = 0;
  for (int i = L - 1; i >= 0; --i) {
    float anext = CRFW_NEG, enext = 0.0f;
    if (live && i > 0) {
      anext = al[(size_t)(i - 1) * T + t];
      enext = e[(size_t)(i - 1) * T + t];
    }
    const float* sa = svec + cur * 3 * TT;
    const float* se = sa + TT;
    const float* sbt = sa + 2 * TT;
    // role "to" = t: pairwise marginals p[t,f] = exp(emit[t] + beta_{i+1}[t] - logZ + trans[t,f] + alpha_i[f])
    const float base = ei + beta - lz;
    const float4* sa4 = reinterpret_cast<const float4*>(sa);
    float rs = 0.0f;
#pragma unroll
    for (int f0 = 0; f0 < TT; f0 += CRFW_CHUNK) {
      if (f0 < T) {
#pragma unroll
        for (int q = 0; q < CRFW_CHUNK / 4; ++q) {
          const float4 vv = sa4[f0 / 4 + q];
          const float vs[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = f0 + 4 * q + j;
            const float p = __expf(base + row[f] + vs[j]);  // row[f] = -inf behind T: p = 0
            rs += p;
            if (!POSTERIOR) dacc[f] += w * p;
          }
        }
      }
    }
    if (live) de[(size_t)i * T + t] = POSTERIOR ? rs : w * rs - ((tg[i] == t) ? w : 0.0f);
    // role "from" = t: beta_i[t] = lse_to((emit[to] + trans[to,t]) + beta_{i+1}[to]); column t of strans, two passes
    float m = -INFINITY;
#pragma unroll 8
    for (int u = 0; u < T; ++u) m = fmaxf(m, (se[u] + col[u * S]) + sbt[u]);
    float s = 0.0f;
#pragma unroll 8
    for (int u = 0; u < T; ++u) s += __expf(((se[u] + col[u * S]) + sbt[u]) - m);
    beta = live ? m + logf(s) : CRFW_NEG;
    ai = anext;
    ei = enext;
    float* nx = svec + (cur ^ 1) * 3 * TT;
    nx[t] = ai;
    nx[TT + t] = ei;
    nx[2 * TT + t] = beta;
    __syncthreads();
    cur ^= 1;
  }
  if (POSTERIOR) return;  // behind the last barrier
  // d trans: thread t owns row t (pair marginals); row STOP additionally gets the terminal marginals; gold path: -w per used
  // transition (thread 0 walks the tags; contention-free through the same atomics)
  if (live) {
#pragma unroll
    for (int f = 0; f < TT; ++f)
      if (f < T && dacc[f] != 0.0f) atomicAdd(dtrans + t * T + f, dacc[f]);
    if (dstop != 0.0f) atomicAdd(dtrans + stop * T + t, dstop);
  }
  if (t == 0) {
    int prev = start;
    for (int k = 0; k < L; ++k) {
      const int tk = tg[k];
      atomicAdd(dtrans + tk * T + prev, -w);
      prev = tk;
    }
    atomicAdd(dtrans + stop * T + prev, -w);
  }
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
static inline bool crfw_args_ok(int B, int n, int T, int start, int stop) {
  return B >= 0 && n >= 0 && T > 0 && T <= CRFW_MAXT && start >= 0 && start < T && stop >= 0 && stop < T;
}
static inline size_t crfw_round16(size_t x) { return (x + 15) & ~(size_t)15; }

template <int TT, bool POSTERIOR>
static int crfw_launch_bwd(const float* emit, const float* trans, const int* tags, const int* lens, const float* alpha,
                           const float* logz, const float* dloss, int B, int n, int T, int start, int stop, float* demit,
                           float* dtrans, void* stream) {
  static std::atomic<unsigned long long> done{0};
  const size_t lds = ((size_t)crfw_trans_floats(T) + 6 * TT) * sizeof(float);
  const size_t lds_max = ((size_t)crfw_trans_floats(TT) + 6 * TT) * sizeof(float);  // 152 832 B at TT = 192, of 160 KiB
  int rc = kbner_set_max_lds_once(done, reinterpret_cast<const void*>(crfw_nll_bwd_kernel<TT, POSTERIOR>), (int)lds_max);
  if (rc) return rc;
  hipLaunchKernelGGL((crfw_nll_bwd_kernel<TT, POSTERIOR>), dim3(B), dim3(TT), lds, (hipStream_t)stream, emit, trans, tags, lens, alpha,
                     logz, dloss, n, T, start, stop, demit, dtrans);
  KBNER_LAUNCH_RET();
}

extern "C" {

// fp32 scores [B,n,T] + u8 backpointers [B,n,T], each region padded to 16 bytes
size_t kbner_crf_wide_viterbi_ws_bytes(int B, int n, int T) {
  if (B <= 0 || n <= 0 || T <= 0) return 0;
  const size_t cells = (size_t)B * n * T;
  return crfw_round16(cells * sizeof(float)) + crfw_round16(cells);
}

int kbner_crf_wide_viterbi(const float* emit, const float* trans, const int* lens, int B, int n, int T, int start, int stop,
                           int* tags, float* conf, int* popped, void* ws, void* stream) {
  KBNER_CHECK_ARG(crfw_args_ok(B, n, T, start, stop));
  KBNER_CHECK_ARG((size_t)B * n == 0 || (ws != nullptr && (reinterpret_cast<uintptr_t>(ws) & 15) == 0));
  if (B == 0) return 0;
  float* wsv = static_cast<float*>(ws);
  unsigned char* wsb = static_cast<unsigned char*>(ws) + crfw_round16((size_t)B * n * T * sizeof(float));
  if (T <= 64)
    hipLaunchKernelGGL(crfw_viterbi_kernel<64>, dim3(B), dim3(64), 0, (hipStream_t)stream, emit, trans, lens, n, T, start, stop, tags,
                       conf, popped, wsv, wsb);
  else if (T <= 128)
    hipLaunchKernelGGL(crfw_viterbi_kernel<128>, dim3(B), dim3(128), 0, (hipStream_t)stream, emit, trans, lens, n, T, start, stop, tags,
                       conf, popped, wsv, wsb);
  else
    hipLaunchKernelGGL(crfw_viterbi_kernel<192>, dim3(B), dim3(192), 0, (hipStream_t)stream, emit, trans, lens, n, T, start, stop, tags,
                       conf, popped, wsv, wsb);
  KBNER_LAUNCH_RET();
}

int kbner_crf_wide_nll_fwd(const float* emit, const float* trans, const int* tags, const int* lens, int B, int n, int T, int start,
                           int stop, float* logz, float* gold, float* alpha, void* stream) {
  KBNER_CHECK_ARG(crfw_args_ok(B, n, T, start, stop));
  if (B == 0) return 0;
  if (T <= 64)
    hipLaunchKernelGGL(crfw_nll_fwd_kernel<64>, dim3(B), dim3(64), 0, (hipStream_t)stream, emit, trans, tags, lens, n, T, start, stop,
                       logz, gold, alpha);
  else if (T <= 128)
    hipLaunchKernelGGL(crfw_nll_fwd_kernel<128>, dim3(B), dim3(128), 0, (hipStream_t)stream, emit, trans, tags, lens, n, T, start, stop,
                       logz, gold, alpha);
  else
    hipLaunchKernelGGL(crfw_nll_fwd_kernel<192>, dim3(B), dim3(192), 0, (hipStream_t)stream, emit, trans, tags, lens, n, T, start, stop,
                       logz, gold, alpha);
  KBNER_LAUNCH_RET();
}

int kbner_crf_wide_nll_bwd(const float* emit, const float* trans, const int* tags, const int* lens, const float* alpha,
                           const float* logz, const float* dloss, int B, int n, int T, int start, int stop, float* demit,
                           float* dtrans, void* stream) {
  KBNER_CHECK_ARG(crfw_args_ok(B, n, T, start, stop));
  if (B == 0) return 0;
  if (T <= 128)
    return crfw_launch_bwd<128, false>(emit, trans, tags, lens, alpha, logz, dloss, B, n, T, start, stop, demit, dtrans, stream);
  return crfw_launch_bwd<192, false>(emit, trans, tags, lens, alpha, logz, dloss, B, n, T, start, stop, demit, dtrans, stream);
}

// token marginals from the alpha / logZ that kbner_crf_wide_nll_fwd saved: marg f32[B,n,T] (rows >= lens[b] are zero)
int kbner_crf_wide_posterior(const float* emit, const float* trans, const int* lens, const float* alpha, const float* logz, int B,
                             int n, int T, int start, int stop, float* marg, void* stream) {
  KBNER_CHECK_ARG(crfw_args_ok(B, n, T, start, stop));
  if (B == 0) return 0;
  if (T <= 128)
    return crfw_launch_bwd<128, true>(emit, trans, nullptr, lens, alpha, logz, nullptr, B, n, T, start, stop, marg, nullptr, stream);
  return crfw_launch_bwd<192, true>(emit, trans, nullptr, lens, alpha, logz, nullptr, B, n, T, start, stop, marg, nullptr, stream);
}

}  // extern "C"
