// Character BiLSTM of FastCharacterEmbeddings for gfx950 (flair/embeddings.py:670-758: torch.nn.Embedding -> one-layer bidirectional
// torch.nn.LSTM over every word's characters, pack_padded_sequence(enforce_sorted=False), zero initial state -> hidden[0], the forward
// direction's h after the last character beside the backward direction's h after the first; trained by autograd in the reference).
// Two entry points, ONE launch each: the hidden size is at most 32, the words are independent sequences and the weights of both
// directions fit in LDS, so nothing here waits for another launch (the generic recurrence of csrc/lstm_train.hip costs a launch per
// time step and needs Hp % 64 == 0).
//   kbner_char_lstm_fwd   out[rows[w], 0:Hc | Hc:2Hc] = bf16(h_fwd | h_bwd) with the head's two pre-RNN dropout sites applied
//   kbner_char_lstm_bwd   back-propagation through time from dout (.) mask; ADDS to d_emb, d_wih, d_whh, d_bias_ih, d_bias_hh
//
// Shape of both kernels: a workgroup of 4 waves stages the weights once and then walks words, ONE WAVE PER WORD: lanes 0-31 are the
// hidden units of the forward direction, lanes 32-63 those of the backward direction (both run len[w] steps, so the halves stay in
// lockstep); c, h and the running gradients live in registers, x_t and h_{t-1} are handed between the lanes of a half through a
// per-wave LDS row (a wave executes its LDS instructions in order: a wavefront fence for the compiler is all the ordering needed).
// The word tables are read wave-uniformly.  No device allocation, no inter-workgroup communication.
//
// Forward LDS image: wl[d][kk][j] = float4 (i, f, g, o) of hidden unit j for input kk of [x (E, padded to Ep = 4 ceil(E / 4)) | h (Hc,
// padded likewise)], zero where padded: a lane reads its four gate weights of one input with one 16-byte read (consecutive lanes,
// consecutive slots: conflict-free) and four inputs with one 16-byte broadcast read.
// Backward LDS image: wT[d][r][kk] = [Wih | Whh] rows as torch stores them (r = q Hc + j), so lane k sums column k (dx) and column
// E + k (dh_{t-1}) over the 4Hc pre-activation gradients, read as broadcasts; the weight gradients accumulate in a per-workgroup LDS
// image (ds_add_f32: the 4 waves share it) and leave with one global atomic per element and workgroup; d_emb rows take one global
// atomic per (character, column).  Summation order therefore varies between runs (the tests compare under a tolerance).
#include "common.h"
#include "lstm_act.h"

#define CHAR_MAXD 32     // E and Hc limit: one lane per hidden unit / embedding column in a 32-lane half
#define CHAR_SAVED 6     // per (word, direction, step): i, f, g, o, c_t, h_t   (f32 [CHAR_SAVED][32])
#define CHAR_DWS 129     // row stride of the LDS weight-gradient image: [kk][q * 32 + j], odd so that the flush walks kk conflict-free

#define CHAR_WAVE_SYNC()                                  \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                      \
  } while (0)

static __host__ __device__ __forceinline__ int char_pad4(int x) { return (x + 3) & ~3; }
static inline int char_fwd_lds_bytes(int E, int Hc) { return (2 * (char_pad4(E) + char_pad4(Hc)) * 32 * 4 + 4 * 2 * 64 + 4 * 64) * 4; }
static inline int char_bwd_lds_bytes(int E, int Hc) {
  const int K = E + Hc;
  return (4 * 2 * 128 + 4 * 2 * 64 + 2 * 4 * Hc * K + 2 * 128 + 2 * K * CHAR_DWS) * 4;
}

static __device__ __forceinline__ int char_id(const int* __restrict__ cw, int pos, int V) {
  const int id = cw[pos];
  return id < 0 ? 0 : (id >= V ? V - 1 : id);   // the host wrapper refuses such a table; the kernel stays inside emb whatever it gets
}

// grid: min(ceil(W / 4), CUs) workgroups of 256.  ws == null: nothing saved.
__global__ __launch_bounds__(256) void char_lstm_fwd_kernel(const float* __restrict__ emb, const float* __restrict__ wih,
                                                           const float* __restrict__ whh, const float* __restrict__ bias_ih,
                                                           const float* __restrict__ bias_hh, const int* __restrict__ chars,
                                                           const int* __restrict__ lens, const int* __restrict__ rows,
                                                           bf16_t* __restrict__ out, int ld_out, int col0, float* __restrict__ ws, int W,
                                                           int Lmax, int V, int E, int Hc, int n, uint32_t seed_e, uint32_t thresh_e,
                                                           uint32_t seed_l, uint32_t thresh_l) {
  extern __shared__ float4 char_lds[];
  const int Ep = char_pad4(E), Hp = char_pad4(Hc), K = Ep + Hp;
  float4* wl = char_lds;                                          // [2][K][32]
  float* xh = reinterpret_cast<float*>(char_lds + 2 * K * 32);    // [4 waves][2][x 32 | h 32]
  float* ob = xh + 4 * 2 * 64;                                    // [4 waves][64]: the word's output row
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int d = lane >> 5, j = lane & 31;
  for (int i = tid; i < 2 * K * 32; i += 256) {
    const int jj = i & 31, kk = (i >> 5) % K, dd = (i >> 5) / K;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jj < Hc) {
      if (kk < E) {
        const float* p = wih + ((size_t)dd * 4 * Hc + jj) * E + kk;
        v = make_float4(p[0], p[(size_t)Hc * E], p[(size_t)2 * Hc * E], p[(size_t)3 * Hc * E]);
      } else if (kk >= Ep && kk - Ep < Hc) {
        const float* p = whh + ((size_t)dd * 4 * Hc + jj) * Hc + (kk - Ep);
        v = make_float4(p[0], p[(size_t)Hc * Hc], p[(size_t)2 * Hc * Hc], p[(size_t)3 * Hc * Hc]);
      }
    }
    wl[i] = v;
  }
  float b[4] = {0.f, 0.f, 0.f, 0.f};
  if (j < Hc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = bias_ih[(d * 4 + q) * Hc + j] + bias_hh[(d * 4 + q) * Hc + j];
  }
  __syncthreads();
  float* xs = xh + (wv * 2 + d) * 64;
  float* hs = xs + 32;
  float* obw = ob + wv * 64;
  const float4* wd = wl + (size_t)d * K * 32 + j;   // + kk * 32
  const uint32_t cke = drop_colkey(seed_e, (uint32_t)(col0 + d * Hc + j)), ckl = drop_colkey(seed_l, (uint32_t)(col0 + d * Hc + j));
  const float scale = drop_scale(thresh_e) * drop_scale(thresh_l);
  const int wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
  for (int w = wave0; w < W; w += gridDim.x * 4) {
    const int row = __builtin_amdgcn_readfirstlane(rows[w]);
    if (row < 0) continue;   // dropped by WordDropout: nothing written, nothing saved
    int len = __builtin_amdgcn_readfirstlane(lens[w]);
    len = len < 0 ? 0 : (len > Lmax ? Lmax : len);
    const int* cw = chars + (size_t)w * Lmax;
    float c = 0.f, h = 0.f, xn = 0.f;
    hs[j] = 0.f;
    if (len > 0 && j < E) xn = emb[(size_t)char_id(cw, d ? len - 1 : 0, V) * E + j];
    for (int t = 0; t < len; ++t) {
      xs[j] = xn;   // 0 in the lanes E .. 31: the padded inputs meet zero weights
      CHAR_WAVE_SYNC();
      if (t + 1 < len && j < E) xn = emb[(size_t)char_id(cw, d ? len - 2 - t : t + 1, V) * E + j];   // in flight under this step
      float a[4] = {b[0], b[1], b[2], b[3]};
      for (int k4 = 0; k4 < Ep; k4 += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(xs + k4);
        const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 wq = wd[(k4 + u) * 32];
          a[0] += x4[u] * wq.x;
          a[1] += x4[u] * wq.y;
          a[2] += x4[u] * wq.z;
          a[3] += x4[u] * wq.w;
        }
      }
      for (int k4 = 0; k4 < Hp; k4 += 4) {
        const float4 hv = *reinterpret_cast<const float4*>(hs + k4);
        const float h4[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 wq = wd[(Ep + k4 + u) * 32];
          a[0] += h4[u] * wq.x;
          a[1] += h4[u] * wq.y;
          a[2] += h4[u] * wq.z;
          a[3] += h4[u] * wq.w;
        }
      }
      const float ig = sigmoid_f(a[0]), fg = sigmoid_f(a[1]), gg = tanh_f(a[2]), og = sigmoid_f(a[3]);
      c = fg * c + ig * gg;
      h = og * tanh_f(c);
      CHAR_WAVE_SYNC();   // every read of h_{t-1} precedes the write of h_t
      hs[j] = h;          // lanes Hc .. 31: zero weights and zero bias give g = 0, so c = h = 0
      if (ws != nullptr) {
        float* s = ws + ((((size_t)w * 2 + d) * Lmax + t) * CHAR_SAVED) * 32 + j;
        s[0] = ig;
        s[32] = fg;
        s[64] = gg;
        s[96] = og;
        s[128] = c;
        s[160] = h;
      }
    }
    // the stored value is the bf16 rounding of h; the masks multiply THAT, as the row kernels do with stored features, so this
    // write equals kbner_gather_rows_drop over the unmasked write bit for bit (threshold 0: scale 1, everything kept)
    const bool keep = drop_keep(drop_rowkey(seed_e, (uint32_t)row), cke, thresh_e) &&
                      drop_keep(drop_rowkey(seed_l, (uint32_t)(row / n)), ckl, thresh_l);
    if (j < Hc) obw[d * Hc + j] = bf2f(f2bf(h)) * (keep ? scale : 0.0f);
    CHAR_WAVE_SYNC();
    bf16_t* orow = out + (size_t)row * ld_out;
    const int nfull = (2 * Hc) >> 3;   // 16-byte stores while eight columns lie inside the block, single columns for its tail
    if (lane < nfull) {
      *reinterpret_cast<uint4*>(orow + lane * 8) = pack8bf(obw + lane * 8);
    } else {
      const int cc = nfull * 8 + (lane - nfull);
      if (cc < 2 * Hc) orow[cc] = f2bf(obw[cc]);
    }
    CHAR_WAVE_SYNC();   // before the next word reuses the rows
  }
}

// grid: min(ceil(W / 4), 128) workgroups of 256 (every workgroup ends with 2 * 4Hc * (E + Hc + 2) global atomics).
__global__ __launch_bounds__(256) void char_lstm_bwd_kernel(const bf16_t* __restrict__ dout, int ld_out, int col0,
                                                           const float* __restrict__ emb, const float* __restrict__ wih,
                                                           const float* __restrict__ whh, const int* __restrict__ chars,
                                                           const int* __restrict__ lens, const int* __restrict__ rows,
                                                           const float* __restrict__ ws, float* __restrict__ d_emb,
                                                           float* __restrict__ d_wih, float* __restrict__ d_whh,
                                                           float* __restrict__ d_bias_ih, float* __restrict__ d_bias_hh, int W, int Lmax,
                                                           int V, int E, int Hc, int n, uint32_t seed_e, uint32_t thresh_e,
                                                           uint32_t seed_l, uint32_t thresh_l) {
  extern __shared__ float4 char_lds[];
  const int K = E + Hc, R4 = 4 * Hc;
  float* das = reinterpret_cast<float*>(char_lds);   // [4 waves][2][128]: pre-activation gradients, r = q Hc + j
  float* vs = das + 4 * 2 * 128;                     // [4 waves][2][64]: [x_t (E) | h_{t-1} (Hc)]
  float* wT = vs + 4 * 2 * 64;                       // [2][R4][K]
  float* dB = wT + 2 * R4 * K;                       // [2][q * 32 + j]
  float* dW = dB + 2 * 128;                          // [2][K][CHAR_DWS]: element (kk, q * 32 + j)
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int d = lane >> 5, j = lane & 31;
  for (int i = tid; i < 2 * R4 * K; i += 256) {
    const int kk = i % K, r = i / K;   // r = dd * R4 + row
    wT[i] = kk < E ? wih[(size_t)r * E + kk] : whh[(size_t)r * Hc + (kk - E)];
  }
  for (int i = tid; i < 2 * 128 + 2 * K * CHAR_DWS; i += 256) dB[i] = 0.f;
  __syncthreads();
  float* da_w = das + (wv * 2 + d) * 128;
  float* v_w = vs + (wv * 2 + d) * 64;
  const float* wTd = wT + (size_t)d * R4 * K;
  float* dWd = dW + (size_t)d * K * CHAR_DWS + j;   // + kk * CHAR_DWS + q * 32
  const int lx = j < E ? j : E - 1, lh = E + (j < Hc ? j : Hc - 1);
  const uint32_t cke = drop_colkey(seed_e, (uint32_t)(col0 + d * Hc + j)), ckl = drop_colkey(seed_l, (uint32_t)(col0 + d * Hc + j));
  const float scale = drop_scale(thresh_e) * drop_scale(thresh_l);
  float db[4] = {0.f, 0.f, 0.f, 0.f};
  const int wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
  for (int w = wave0; w < W; w += gridDim.x * 4) {
    const int row = __builtin_amdgcn_readfirstlane(rows[w]);
    if (row < 0) continue;
    int len = __builtin_amdgcn_readfirstlane(lens[w]);
    len = len < 0 ? 0 : (len > Lmax ? Lmax : len);
    const int* cw = chars + (size_t)w * Lmax;
    const bool keep = drop_keep(drop_rowkey(seed_e, (uint32_t)row), cke, thresh_e) &&
                      drop_keep(drop_rowkey(seed_l, (uint32_t)(row / n)), ckl, thresh_l);
    float dh = j < Hc ? bf2f(dout[(size_t)row * ld_out + d * Hc + j]) * (keep ? scale : 0.0f) : 0.f;
    float dc = 0.f;
    for (int t = len - 1; t >= 0; --t) {
      const int id = char_id(cw, d ? len - 1 - t : t, V);
      const float* s = ws + ((((size_t)w * 2 + d) * Lmax + t) * CHAR_SAVED) * 32 + j;
      const float ig = s[0], fg = s[32], gg = s[64], og = s[96], ct = s[128];
      const float cp = t > 0 ? s[128 - CHAR_SAVED * 32] : 0.f, hp = t > 0 ? s[160 - CHAR_SAVED * 32] : 0.f;
      const float x = j < E ? emb[(size_t)id * E + j] : 0.f;
      const float tc = tanh_f(ct);
      dc += dh * og * (1.0f - tc * tc);
      float da[4];
      da[0] = dc * gg * ig * (1.0f - ig);
      da[1] = dc * cp * fg * (1.0f - fg);
      da[2] = dc * ig * (1.0f - gg * gg);
      da[3] = dh * tc * og * (1.0f - og);
      dc *= fg;
      if (j < Hc) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          da_w[q * Hc + j] = da[q];
          db[q] += da[q];
        }
        v_w[E + j] = hp;
      }
      if (j < E) v_w[j] = x;
      CHAR_WAVE_SYNC();
      if (j < Hc) {   // dW[q Hc + j][kk] += da_q[j] v[kk]
        for (int kk = 0; kk < K; ++kk) {
          const float v = v_w[kk];
#pragma unroll
          for (int q = 0; q < 4; ++q) atomicAdd(dWd + kk * CHAR_DWS + q * 32, da[q] * v);
        }
      }
      float ax = 0.f, ah = 0.f;   // lane k: dx[k] and dh_{t-1}[k] = sum_r da[r] W[r][k | E + k]
      for (int r4 = 0; r4 < R4; r4 += 4) {
        const float4 av = *reinterpret_cast<const float4*>(da_w + r4);
        const float a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* wr = wTd + (size_t)(r4 + u) * K;
          ax += a4[u] * wr[lx];
          ah += a4[u] * wr[lh];
        }
      }
      dh = j < Hc ? ah : 0.f;
      if (j < E) atomicAdd(d_emb + (size_t)id * E + j, ax);
      CHAR_WAVE_SYNC();   // before the next step rewrites the rows
    }
  }
  if (j < Hc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) atomicAdd(dB + d * 128 + q * 32 + j, db[q]);
  }
  __syncthreads();
  for (int i = tid; i < 2 * R4 * K; i += 256) {
    const int kk = i % K, r = i / K, dd = r / R4, rr = r % R4;
    const float v = dW[((size_t)dd * K + kk) * CHAR_DWS + (rr / Hc) * 32 + rr % Hc];
    if (kk < E)
      atomicAdd(d_wih + (size_t)r * E + kk, v);
    else
      atomicAdd(d_whh + (size_t)r * Hc + (kk - E), v);
  }
  for (int r = tid; r < 2 * R4; r += 256) {
    const int dd = r / R4, rr = r % R4;
    const float v = dB[dd * 128 + (rr / Hc) * 32 + rr % Hc];
    atomicAdd(d_bias_ih + r, v);
    atomicAdd(d_bias_hh + r, v);
  }
}

static bool char_shape_ok(int W, int Lmax, int V, int E, int Hc, int ld_out, int col0, int n) {
  return W >= 0 && Lmax >= 1 && V >= 1 && E >= 1 && E <= CHAR_MAXD && Hc >= 1 && Hc <= CHAR_MAXD && ld_out >= 2 * Hc && ld_out % 8 == 0 &&
         col0 >= 0 && col0 % 8 == 0 && n >= 1;
}

extern "C" {

// bytes of the workspace kbner_char_lstm_fwd fills for kbner_char_lstm_bwd (0 for arguments outside the limits)
size_t kbner_char_lstm_ws_bytes(int W, int Lmax, int Hc) {
  if (W < 0 || Lmax < 1 || Hc < 1 || Hc > CHAR_MAXD) return 0;
  return (size_t)W * 2 * Lmax * CHAR_SAVED * 32 * sizeof(float);
}

int kbner_char_lstm_fwd(const float* emb, const float* wih, const float* whh, const float* bias_ih, const float* bias_hh,
                        const int* chars, const int* lens, const int* rows, bf16_t* out, int ld_out, int col0, float* ws, int W, int Lmax,
                        int V, int E, int Hc, int n, uint32_t seed_e, uint32_t thresh_e, uint32_t seed_l, uint32_t thresh_l, void* stream) {
  KBNER_CHECK_ARG(char_shape_ok(W, Lmax, V, E, Hc, ld_out, col0, n) && (long long)col0 + 2 * Hc <= (long long)ld_out);
  KBNER_CHECK_ARG(((uintptr_t)out & 15) == 0);
  if (W == 0) return KBNER_OK;
  KBNER_CHECK_ARG(emb != nullptr && wih != nullptr && whh != nullptr && bias_ih != nullptr && bias_hh != nullptr && chars != nullptr &&
                  lens != nullptr && rows != nullptr && out != nullptr);
  static std::atomic<unsigned long long> attr_done{0};
  const int r = kbner_set_max_lds_once(attr_done, reinterpret_cast<const void*>(char_lstm_fwd_kernel), char_fwd_lds_bytes(CHAR_MAXD, CHAR_MAXD));
  if (r) return r;
  int grid = (W + 3) / 4;
  const int cus = kbner_cu_count();
  if (grid > cus) grid = cus;
  hipLaunchKernelGGL(char_lstm_fwd_kernel, dim3(grid), dim3(256), char_fwd_lds_bytes(E, Hc), (hipStream_t)stream, emb, wih, whh, bias_ih,
                     bias_hh, chars, lens, rows, out, ld_out, col0, ws, W, Lmax, V, E, Hc, n, seed_e, thresh_e, seed_l, thresh_l);
  KBNER_LAUNCH_RET();
}

int kbner_char_lstm_bwd(const bf16_t* dout, int ld_out, int col0, const float* emb, const float* wih, const float* whh, const int* chars,
                        const int* lens, const int* rows, const float* ws, float* d_emb, float* d_wih, float* d_whh, float* d_bias_ih,
                        float* d_bias_hh, int W, int Lmax, int V, int E, int Hc, int n, uint32_t seed_e, uint32_t thresh_e,
                        uint32_t seed_l, uint32_t thresh_l, void* stream) {
  KBNER_CHECK_ARG(char_shape_ok(W, Lmax, V, E, Hc, ld_out, col0, n));
  if (W == 0) return KBNER_OK;
  KBNER_CHECK_ARG(dout != nullptr && emb != nullptr && wih != nullptr && whh != nullptr && chars != nullptr && lens != nullptr &&
                  rows != nullptr && ws != nullptr && d_emb != nullptr && d_wih != nullptr && d_whh != nullptr && d_bias_ih != nullptr &&
                  d_bias_hh != nullptr);
  static std::atomic<unsigned long long> attr_done{0};
  const int r = kbner_set_max_lds_once(attr_done, reinterpret_cast<const void*>(char_lstm_bwd_kernel), char_bwd_lds_bytes(CHAR_MAXD, CHAR_MAXD));
  if (r) return r;
  int grid = (W + 3) / 4;
  if (grid > 128) grid = 128;
  hipLaunchKernelGGL(char_lstm_bwd_kernel, dim3(grid), dim3(256), char_bwd_lds_bytes(E, Hc), (hipStream_t)stream, dout, ld_out, col0, emb,
                     wih, whh, chars, lens, rows, ws, d_emb, d_wih, d_whh, d_bias_ih, d_bias_hh, W, Lmax, V, E, Hc, n, seed_e, thresh_e,
                     seed_l, thresh_l);
  KBNER_LAUNCH_RET();
}

}  // extern "C"
