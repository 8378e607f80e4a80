// Self-attention for a FEW query rows per sentence against ALL keys of the sentence (gfx950, head_dim 64, S <= 512): the last
// encoder layer of the tagger, whose output is read at the first sub-token of each kept word only.  Same math as attention.hip
// (scores q.k + mask / scale, exp2 with scale * log2 e, probabilities rounded to bf16 before P.V, lse of the undropped softmax,
// dropout keyed by the ORIGINAL query / key index of the head), different shape: nq queries x S keys per head is too little work
// to tile over queries, so one workgroup per (sentence, head) splits the KEYS over its 8 waves -- wave w owns keys
// [64 w, 64 w + 64), waves past S idle -- and the waves' partial results meet in LDS once per block of 16 queries:
//
//   kbner_attn_rows_fwd   per wave: S^T = K Q^T for its keys (K fragments stationary in registers); the waves exchange their row
//                         maxima, so the exponentials are taken against the maximum attention.hip's forward takes for the same
//                         keys (all keys, or per half where its two-part 32-row kernel would run) and are its bits; O^T partial
//                         = V^T P^T (V through LDS for the transposed read); the 8 partial (sum, O) pairs are added
//                                                                                               -> ctx_c bf16, o32 f32, lse_c
//   kbner_attn_rows_bwd   per wave: dK, dV of its keys accumulate in registers over all query blocks; the score tile of a
//                         (16 queries x 16 keys) pair is formed in BOTH orientations -- [query, key] feeds dK / dV, [key, query]
//                         feeds dQ -- because each product contracts over the other axis (16 x 16 x 16 MFMAs take a score tile
//                         as their B operand as it stands); the dQ partials of the 8 waves are summed through LDS.  Writes every
//                         row of dqkv: dK | dV of all keys, dQ at the listed rows, zeros in the Q third of the others.
//
// Both are bound by moving K and V (and dK, dV) once per head, not by issue: nothing here is tuned beyond 16-byte loads and
// MFMA for the products.  The query list q_pos i32 [B, nq] holds positions inside the sentence (unique per sentence; < 0 or >= S:
// no query -- zero output rows, no gradient).
#include "common.h"

#include "attn_common.h"

#define AR_QB 16       // queries per block
#define AR_RED_LD 68   // floats per query row of a wave's partial [16][64] tile in LDS (padded: 16-byte rows, spread over banks)

// dynamic LDS: one [AT_MAXS][64] bf16 panel | the 8 waves' partial tiles | two [16][64] bf16 query panels | per-key | per-query
#define AR_OFF_RED (AT_MAXS * 128)
#define AR_OFF_QP (AR_OFF_RED + AT_NW * AR_QB * AR_RED_LD * 4)
#define AR_OFF_KEY (AR_OFF_QP + 2 * AR_QB * 128)
#define AR_OFF_QRY (AR_OFF_KEY + 3 * AT_MAXS * 4)
#define AR_OFF_QSUM (AR_OFF_QRY + (2 * AT_NW + 4) * AR_QB * 4)   // backward: [16][64] running column sums of the dQ rows
#define AR_LDS_BYTES (AR_OFF_QSUM + AR_QB * 64 * 4)

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k((a), (b), (c), 0, 0, 0)

// rows [r0, r0 + 64) of a [*, 64] bf16 panel (row stride ld) into the swizzled LDS image, by one wave
static __device__ __forceinline__ void ar_stage64(const bf16_t* __restrict__ src, int ld, int r0, unsigned char* s, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = r0 + i * 8 + (lane >> 3), c = lane & 7;
    *reinterpret_cast<uint4*>(s + row * 128 + ((c ^ kc_swz(row)) << 4)) = *reinterpret_cast<const uint4*>(src + (size_t)row * ld + c * 8);
  }
}
// one 16-key (or 16-query) block of a panel transposed: A operand of a 16 x 16 x 16 MFMA, rows = panel columns db*16 + (lane & 15),
// k = panel rows g*4 .. g*4 + 3 of the block (the first half of attn_common.h's tr_at)
static __device__ __forceinline__ s4v tr16_at(const unsigned char* base, int off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s4v __attribute__((address_space(3)))*)(base + off));
}
// a score tile's four values of this lane (rows g*4 .. g*4 + 3) as the B operand of a 16 x 16 x 16 MFMA
static __device__ __forceinline__ s4v pack_b16(const f4v a) {
  union {
    uint32_t u[2];
    s4v v;
  } r;
  r.u[0] = pack2bf(a[0], a[1]);
  r.u[1] = pack2bf(a[2], a[3]);
  return r.v;
}
static __device__ __forceinline__ bf16x8 zero_frag() {
  const s8v z = {0, 0, 0, 0, 0, 0, 0, 0};
  return __builtin_bit_cast(bf16x8, z);
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(AT_NW * 64) void attn_rows_fwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ maskbias,
                                                                  const int* __restrict__ q_pos, bf16_t* __restrict__ ctx_c,
                                                                  float* __restrict__ o32, float* __restrict__ lse_c, int S, int H, int A,
                                                                  int nq, float scale, uint32_t drop_seed, uint32_t drop_thresh, int two_parts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sV = smem;
  float* red = reinterpret_cast<float*>(smem + AR_OFF_RED);
  float* sMask = reinterpret_cast<float*>(smem + AR_OFF_KEY);
  uint32_t* sCk = reinterpret_cast<uint32_t*>(smem + AR_OFF_KEY + AT_MAXS * 4);
  float* sM = reinterpret_cast<float*>(smem + AR_OFF_QRY);   // [wave][query]: the wave's maximum (log2 domain) and exponential sum
  float* sSum = sM + AT_NW * AR_QB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int h = blockIdx.x, b = blockIdx.y;
  const int ld = 3 * H;
  const int nact = S / 64;
  const bool active = wid < nact;
  const int nhalf = two_parts ? nact / 2 : nact;   // waves [0, nhalf) hold the first part of the key axis
  const bf16_t* base = qkv + (size_t)b * S * ld + h * AT_D;
  const uint32_t bhS = (uint32_t)((b * A + h) * S);
  const float scale2 = scale * 1.4426950408889634f;
  const float dscale = DROP ? drop_scale(drop_thresh) : 1.0f;
  const int k0 = wid * 64;
  bf16x8 kf[4][2];
  if (active) {
    ar_stage64(base + 2 * H, ld, k0, sV, lane);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      kf[kb][0] = glb_frag(base + H, ld, k0 + kb * 16, 0, lane);
      kf[kb][1] = glb_frag(base + H, ld, k0 + kb * 16, 1, lane);
    }
  }
  for (int i = tid; i < S; i += AT_NW * 64) {
    sMask[i] = maskbias[(size_t)b * S + i] * (1.0f / scale);   // added to the RAW score sums, as in attention.hip
    if (DROP) sCk[i] = drop_colkey(drop_seed, bhS + (uint32_t)i);
  }
  __syncthreads();
  const PanelBases pV = panel_bases(sV, lane);
  for (int qb = 0; qb * AR_QB < nq; ++qb) {
    // S^T tiles [key g*4 + r of the 16-key block, query li], accumulators started at mask / scale
    f4v st[4];
    int pos = -1;
    if (active) {
      const int qi = qb * AR_QB + li;
      pos = qi < nq ? q_pos[(size_t)b * nq + qi] : -1;
      if (pos >= S) pos = -1;
      bf16x8 qf0 = zero_frag(), qf1 = zero_frag();
      if (pos >= 0) {
        const bf16_t* qrow = base + (size_t)pos * ld + g * 8;
        qf0 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const s8v*>(qrow));
        qf1 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const s8v*>(qrow + 32));
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        f4v a = *reinterpret_cast<const f4v*>(sMask + k0 + kb * 16 + g * 4);
        a = MFMA(kf[kb][0], qf0, a);
        a = MFMA(kf[kb][1], qf1, a);
        mx = fmaxf(fmaxf(mx, a[0]), a[1]);
        mx = fmaxf(fmaxf(mx, a[2]), a[3]);
        st[kb] = a;
      }
      mx = group4_max(mx);
      if (g == 0) sM[wid * AR_QB + li] = mx;   // the maximum of the RAW sums over this wave's keys
    }
    __syncthreads();
    if (active) {
      // the row maximum attention.hip's forward takes for these keys -- over ALL keys, or (two_parts: where kbner_attn_fwd runs its
      // 32-row kernel, which walks the keys in two halves) over the first half for the first half's keys -- so the exponentials
      // (the same fused a * scale2 - max * scale2) and with them the bf16 probabilities that multiply V are the same bits
      float mx = sM[li];
      for (int w = 1; w < (wid < nhalf ? nhalf : nact); ++w) mx = fmaxf(mx, sM[w * AR_QB + li]);
      const float nmx = -mx * scale2;
      const uint32_t rk = DROP ? drop_rowkey(drop_seed, bhS + (uint32_t)pos) : 0u;
      float sum = 0.0f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        f4v a = st[kb];
        a[0] = __builtin_amdgcn_exp2f(a[0] * scale2 + nmx);
        a[1] = __builtin_amdgcn_exp2f(a[1] * scale2 + nmx);
        a[2] = __builtin_amdgcn_exp2f(a[2] * scale2 + nmx);
        a[3] = __builtin_amdgcn_exp2f(a[3] * scale2 + nmx);
        if (DROP) {
          sum += (a[0] + a[1]) + (a[2] + a[3]);   // normaliser of the UNdropped softmax
          a = drop_zero4(a, rk, sCk + k0 + kb * 16 + g * 4, drop_thresh);
        }
        st[kb] = a;
      }
      if (DROP) sum = group4_sum(sum);
      // O^T partial [d = db*16 + g*4 + r, query li] from the unnormalised bf16 exponentials; without dropout the row sums are
      // those of exactly the bf16 probabilities that multiply V (one MFMA against an all-ones fragment), as in attention.hip
      f4v o[4], osum = (f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = (f4v){0.f, 0.f, 0.f, 0.f};
      const s8v ones_s = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
      const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_s);
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        const bf16x8 pb = pack_b(st[2 * kc], st[2 * kc + 1]);
        if (!DROP) osum = MFMA(ones, pb, osum);
#pragma unroll
        for (int db = 0; db < 4; ++db) o[db] = MFMA(tr_at(pV.tr[db], (wid * 2 + kc) * 4096), pb, o[db]);
      }
      if (!DROP) sum = osum[0];
#pragma unroll
      for (int db = 0; db < 4; ++db) *reinterpret_cast<f4v*>(red + (wid * AR_QB + li) * AR_RED_LD + db * 16 + g * 4) = o[db];
      if (g == 0) sSum[wid * AR_QB + li] = sum;
    }
    __syncthreads();
    if (tid < AR_QB * 8) {   // one thread per (query, 8 columns): the waves' partial sums added, normalised, stored
      const int q = tid >> 3, c = tid & 7;
      const int qi = qb * AR_QB + q;
      if (qi < nq) {
        const int pos = q_pos[(size_t)b * nq + qi];
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float m0 = sM[q], tot = 0.0f;
        for (int w = 1; w < nhalf; ++w) m0 = fmaxf(m0, sM[w * AR_QB + q]);
        float m2 = m0;
        for (int w = nhalf; w < nact; ++w) m2 = fmaxf(m2, sM[w * AR_QB + q]);
        for (int w = 0; w < nact; ++w) {
          if (w == nhalf) {   // the online-softmax step of the two-part forward: the first part to the new reference
            const float alpha = __builtin_amdgcn_exp2f((m0 - m2) * scale2);
            tot *= alpha;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] *= alpha;
          }
          tot += sSum[w * AR_QB + q];
          const float* p = red + (w * AR_QB + q) * AR_RED_LD + c * 8;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += p[j];
        }
        m2 *= scale2;   // log2-domain maximum, what the stored lse needs
        const bool none = pos < 0 || pos >= S;
        const float inv = none ? 0.0f : dscale / tot;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= inv;
        const size_t row = (size_t)b * nq + qi;
        *reinterpret_cast<uint4*>(ctx_c + row * H + h * AT_D + c * 8) = pack8bf(v);
        float* orow = o32 + row * H + h * AT_D + c * 8;
        *reinterpret_cast<float4*>(orow) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(orow + 4) = make_float4(v[4], v[5], v[6], v[7]);
        if (c == 0) lse_c[((size_t)b * A + h) * nq + qi] = none ? 0.0f : (m2 + __log2f(tot)) * 0.6931471805599453f;
      }
    }
    __syncthreads();   // the partial tiles are rewritten by the next block
  }
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
// column sums of this wave's [d = db*16 + g*4 + r][key li] accumulators over li, then over the waves: one atomic per column
static __device__ __forceinline__ void ar_flush_colsum(const f4v (&acc)[4], float* red, float* __restrict__ out, int wid, int lane, int tid) {
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = acc[db][r];
      x += __shfl_xor(x, 1, 64);
      x += __shfl_xor(x, 2, 64);
      x += __shfl_xor(x, 4, 64);
      x += __shfl_xor(x, 8, 64);
      if ((lane & 15) == 0) red[wid * 64 + db * 16 + (lane >> 4) * 4 + r] = x;
    }
  __syncthreads();
  if (tid < 64) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < AT_NW; ++w) t += red[w * 64 + tid];
    atomicAdd(out + tid, t);
  }
  __syncthreads();
}

template <bool DROP>
__global__ __launch_bounds__(AT_NW * 64) void attn_rows_bwd_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ q_pos,
                                                                  const bf16_t* __restrict__ dctx_c, const float* __restrict__ o32,
                                                                  const float* __restrict__ lse_c, const float* __restrict__ maskbias,
                                                                  bf16_t* __restrict__ dqkv, float* __restrict__ dbias, int S, int H, int A,
                                                                  int nq, float scale, uint32_t drop_seed, uint32_t drop_thresh, int fused) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sK = smem;
  float* red = reinterpret_cast<float*>(smem + AR_OFF_RED);
  unsigned char* sQ = smem + AR_OFF_QP;
  unsigned char* sO = sQ + AR_QB * 128;
  float* sMask = reinterpret_cast<float*>(smem + AR_OFF_KEY);
  uint32_t* sCk = reinterpret_cast<uint32_t*>(smem + AR_OFF_KEY + AT_MAXS * 4);
  int* sListed = reinterpret_cast<int*>(smem + AR_OFF_KEY + 2 * AT_MAXS * 4);
  float* sL = reinterpret_cast<float*>(smem + AR_OFF_QRY);   // per query of the block: the lse term (see prob), -(1-p) D, dropout row key, row
  float* sD = sL + AR_QB;
  uint32_t* sRk = reinterpret_cast<uint32_t*>(sD + AR_QB);
  int* sPos = reinterpret_cast<int*>(sRk + AR_QB);
  float* sQsum = reinterpret_cast<float*>(smem + AR_OFF_QSUM);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int h = blockIdx.x, b = blockIdx.y;
  const int ld = 3 * H;
  const int nact = S / 64;
  const bool active = wid < nact;
  const bf16_t* base = qkv + (size_t)b * S * ld + h * AT_D;
  bf16_t* dbase = dqkv + (size_t)b * S * ld + h * AT_D;
  const uint32_t bhS = (uint32_t)((b * A + h) * S);
  const float scale2 = scale * 1.4426950408889634f;
  const float dscale = DROP ? drop_scale(drop_thresh) : 1.0f;
  const float oscale = scale * dscale;   // dS carries (1-p): the 1 / (1-p) of dropout leaves through the final scales
  const int k0 = wid * 64;
  if (active) ar_stage64(base + H, ld, k0, sK, lane);
  for (int i = tid; i < S; i += AT_NW * 64) {
    sMask[i] = maskbias[(size_t)b * S + i] * (fused ? 1.0f / scale : 1.4426950408889634f);
    if (DROP) sCk[i] = drop_colkey(drop_seed, bhS + (uint32_t)i);
    sListed[i] = 0;
  }
  for (int i = tid; i < AR_QB * 64; i += AT_NW * 64) sQsum[i] = 0.0f;
  __syncthreads();
  for (int i = tid; i < nq; i += AT_NW * 64) {
    const int pos = q_pos[(size_t)b * nq + i];
    if (pos >= 0 && pos < S) sListed[pos] = 1;
  }
  __syncthreads();
  // the Q third of every row that is no listed query: exact zeros
  for (int i = tid; i < S * 8; i += AT_NW * 64) {
    const int row = i >> 3, c = i & 7;
    if (!sListed[row]) *reinterpret_cast<uint4*>(dbase + (size_t)row * ld + c * 8) = make_uint4(0, 0, 0, 0);
  }
  const PanelBases pK = panel_bases(sK, lane), pQ = panel_bases(sQ, lane), pO = panel_bases(sO, lane);
  // P from a score sum, the key's mask term and the query's lse term -- in the arithmetic of the kbner_attn_bwd kernels that
  // would run this shape, so that both paths round the same probabilities: the 32-row kernels (fused) start the score
  // accumulators at -lse / scale, add mask / scale and take exp2(scale2 * sum); the 16-row ones take exp2(scale2 * s + mask * log2 e
  // - lse * log2 e).  sMask and sL hold the terms in the form of the arithmetic chosen.
  auto prob = [&](float sc, float mk, float l) {
    return fused ? __builtin_amdgcn_exp2f((sc + mk) * scale2) : __builtin_amdgcn_exp2f(sc * scale2 + mk - l);
  };
  const f4v zero4 = (f4v){0.f, 0.f, 0.f, 0.f};
  // dK and dV of a wave's 64 keys are 128 accumulator registers together: they are taken in TWO passes over the query blocks
  // (dV first, then dK with dQ), each re-forming the score tiles it needs -- a few MFMAs per block -- so one set of 64 is live
  f4v acc[4][4];
  f4v bs[4];
  // stage Q and dO of block qb's queries (zero rows for "none"), D = rowdot(dO, O) from the fp32 O
  auto stage_block = [&](int qb) {
    __syncthreads();   // the previous block's panels and partial tiles are dead
    if (tid < AR_QB * 8) {
      const int q = tid >> 3, c = tid & 7;
      const int qi = qb * AR_QB + q;
      int pos = qi < nq ? q_pos[(size_t)b * nq + qi] : -1;
      if (pos >= S) pos = -1;
      uint4 qv = make_uint4(0, 0, 0, 0), dov = make_uint4(0, 0, 0, 0);
      float dpart = 0.0f;
      if (pos >= 0) {
        const size_t row = (size_t)b * nq + qi;
        qv = *reinterpret_cast<const uint4*>(base + (size_t)pos * ld + c * 8);
        dov = *reinterpret_cast<const uint4*>(dctx_c + row * H + h * AT_D + c * 8);
        const float* orow = o32 + row * H + h * AT_D + c * 8;
        const float4 oa = *reinterpret_cast<const float4*>(orow), ob = *reinterpret_cast<const float4*>(orow + 4);
        float dof[8];
        unpack8bf(dov, dof);
        // D from O as kbner_attn_bwd sees it -- bf16(O) plus the e5m2 byte of its rounding residual (common.h pack2bf_res8) -- so
        // that this path and the full one take the same correction, not a better one here: the two must train alike
        const float ov[8] = {oa.x, oa.y, oa.z, oa.w, ob.x, ob.y, ob.z, ob.w};
        float dmain = 0.0f, dres = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t rb = 0u;
          const f2v o16 = unpack2bf(pack2bf_res8(ov[2 * j], ov[2 * j + 1], rb, false));
          const f2v r8 = __builtin_amdgcn_cvt_pk_f32_bf8((int)rb, false);
          dmain += dof[2 * j] * o16[0] + dof[2 * j + 1] * o16[1];
          dres += dof[2 * j] * r8[0] + dof[2 * j + 1] * r8[1];
        }
        dpart = dmain + dres * (1.0f / KBNER_RES8_SCALE);
      }
      *reinterpret_cast<uint4*>(sQ + q * 128 + ((c ^ kc_swz(q)) << 4)) = qv;
      *reinterpret_cast<uint4*>(sO + q * 128 + ((c ^ kc_swz(q)) << 4)) = dov;
      dpart += __shfl_xor(dpart, 1, 64);
      dpart += __shfl_xor(dpart, 2, 64);
      dpart += __shfl_xor(dpart, 4, 64);
      if (c == 0) {
        sPos[q] = pos;
        const float lse_q = pos >= 0 ? lse_c[((size_t)b * A + h) * nq + qi] : 0.0f;
        sL[q] = fused ? -lse_q / scale : lse_q * 1.4426950408889634f;
        sD[q] = -dpart * (1.0f / dscale);   // the dP accumulators start at -(1-p) D (= -D without dropout)
        sRk[q] = DROP ? drop_rowkey(drop_seed, bhS + (uint32_t)pos) : 0u;
      }
    }
    __syncthreads();
  };
  auto zero_acc = [&]() {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int db = 0; db < 4; ++db) acc[kb][db] = zero4;
#pragma unroll
    for (int db = 0; db < 4; ++db) bs[db] = zero4;
  };
  // this wave's accumulators (dK^T / dV^T fragments: lane holds key li, columns db*16 + g*4 .. + 3) * sc to column block `third`
  // of dqkv, their column sums to the bias gradient
  auto store_acc = [&](int third, float sc) {
    if (active) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        bf16_t* row = dbase + (size_t)(k0 + kb * 16 + li) * ld + third * H;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          AT_STORE_SCALED(acc[kb], sc, row, db)
          bs[db] += acc[kb][db] * sc;
        }
      }
    }
    __syncthreads();   // (the partial-tile area doubles as the column sums' scratch)
    if (dbias != nullptr) ar_flush_colsum(bs, red, dbias + third * H + h * AT_D, wid, lane, tid);
  };

  // ---- pass 1: dV = (mask * P / (1-p))^T dO, score tiles [query g*4 + r, key li]
  zero_acc();
  for (int qb = 0; qb * AR_QB < nq; ++qb) {
    stage_block(qb);
    if (active) {
      const bf16x8 qa0 = kc_at(pQ.kc[0], 0), qa1 = kc_at(pQ.kc[1], 0);
      const f4v l_q = *reinterpret_cast<const f4v*>(sL + g * 4);
      uint32_t rk_q[4] = {0u, 0u, 0u, 0u};
      if (DROP) load_keys4(sRk + g * 4, rk_q);
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const int kk = k0 + kb * 16;
        const int co = (kk >> 4) * 2048;
        f4v s;
        AT_MFMA2(s, qa0, qa1, kc_at(pK.kc[0], co), kc_at(pK.kc[1], co), fused ? l_q : zero4);
        const float mk = sMask[kk + li];
        const uint32_t ck = DROP ? sCk[kk + li] : 0u;
        f4v pr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = prob(s[r], mk, l_q[r]);
          pr[r] = (!DROP || drop_keep(rk_q[r], ck, drop_thresh)) ? e : 0.0f;
        }
        const s4v pb = pack_b16(pr);
#pragma unroll
        for (int db = 0; db < 4; ++db) acc[kb][db] = MFMA16(tr16_at(pO.tr[db], 0), pb, acc[kb][db]);
      }
    }
  }
  store_acc(2, dscale);

  // ---- pass 2: dK = dS^T Q from the [query, key] tiles, dQ = dS K from the [key, query] tiles; dS = P * (mask * dP - (1-p) D)
  zero_acc();
  for (int qb = 0; qb * AR_QB < nq; ++qb) {
    stage_block(qb);
    if (active) {
      const bf16x8 qa0 = kc_at(pQ.kc[0], 0), qa1 = kc_at(pQ.kc[1], 0);
      const bf16x8 da0 = kc_at(pO.kc[0], 0), da1 = kc_at(pO.kc[1], 0);
      // [key, query] orientation: this lane's query is li ; [query, key] orientation: its queries are g*4 + r
      const float l_t = sL[li], d_t = sD[li];
      const uint32_t rk_t = sRk[li];
      const f4v l_q = *reinterpret_cast<const f4v*>(sL + g * 4), d_q = *reinterpret_cast<const f4v*>(sD + g * 4);
      uint32_t rk_q[4] = {0u, 0u, 0u, 0u};
      if (DROP) load_keys4(sRk + g * 4, rk_q);
      const f4v tinit = (f4v){d_t, d_t, d_t, d_t}, linit = (f4v){l_t, l_t, l_t, l_t};
      f4v dq[4];
#pragma unroll
      for (int db = 0; db < 4; ++db) dq[db] = zero4;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const int kk = k0 + kb * 16;
        const int co = (kk >> 4) * 2048;
        const bf16x8 kf0 = kc_at(pK.kc[0], co), kf1 = kc_at(pK.kc[1], co);
        const bf16x8 vf0 = glb_frag(base + 2 * H, ld, kk, 0, lane), vf1 = glb_frag(base + 2 * H, ld, kk, 1, lane);
        // ---- [key g*4 + r, query li]: dS^T -> dQ
        {
          f4v s, p;
          AT_MFMA2(s, kf0, kf1, qa0, qa1, fused ? linit : zero4);
          AT_MFMA2(p, vf0, vf1, da0, da1, tinit);
          const f4v mk = *reinterpret_cast<const f4v*>(sMask + kk + g * 4);
          uint32_t ck[4] = {0u, 0u, 0u, 0u};
          if (DROP) load_keys4(sCk + kk + g * 4, ck);
          f4v ds;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = prob(s[r], mk[r], l_t);
            float dp = p[r];
            if (DROP) dp = drop_keep(rk_t, ck[r], drop_thresh) ? dp : d_t;
            ds[r] = e * dp;
          }
          const s4v dsb = pack_b16(ds);
#pragma unroll
          for (int db = 0; db < 4; ++db) dq[db] = MFMA16(tr16_at(pK.tr[db], co), dsb, dq[db]);
        }
        // ---- [query g*4 + r, key li]: dS -> dK
        {
          f4v s, p;
          AT_MFMA2(s, qa0, qa1, kf0, kf1, fused ? l_q : zero4);
          AT_MFMA2(p, da0, da1, vf0, vf1, d_q);
          const float mk = sMask[kk + li];
          const uint32_t ck = DROP ? sCk[kk + li] : 0u;
          f4v ds;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = prob(s[r], mk, l_q[r]);
            float dp = p[r];
            if (DROP) dp = drop_keep(rk_q[r], ck, drop_thresh) ? dp : d_q[r];
            ds[r] = e * dp;
          }
          const s4v dsb = pack_b16(ds);
#pragma unroll
          for (int db = 0; db < 4; ++db) acc[kb][db] = MFMA16(tr16_at(pQ.tr[db], 0), dsb, acc[kb][db]);
        }
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) *reinterpret_cast<f4v*>(red + (wid * AR_QB + li) * AR_RED_LD + db * 16 + g * 4) = dq[db];
    }
    __syncthreads();
    if (tid < AR_QB * 8) {   // dQ of the block: the waves' partials summed, scaled, stored at the queries' own rows
      const int q = tid >> 3, c = tid & 7;
      const int pos = sPos[q];
      if (pos >= 0) {
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int w = 0; w < nact; ++w) {
          const float* p = red + (w * AR_QB + q) * AR_RED_LD + c * 8;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += p[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v[j] *= oscale;
          sQsum[q * 64 + c * 8 + j] += v[j];   // (this thread's own slot, block after block)
        }
        *reinterpret_cast<uint4*>(dbase + (size_t)pos * ld + c * 8) = pack8bf(v);
      }
    }
  }
  store_acc(1, oscale);
  if (dbias != nullptr && tid < 64) {   // (store_acc ends behind a barrier: every sQsum slot is final)
    float t = 0.0f;
#pragma unroll
    for (int q = 0; q < AR_QB; ++q) t += sQsum[q * 64 + tid];
    atomicAdd(dbias + h * AT_D + tid, t);
  }
}

template <auto KERNEL, typename... Args>
static int launch_rows(dim3 grid, hipStream_t stream, Args... args) {
  static std::atomic<unsigned long long> attr_done{0};   // per kernel, one bit per device (common.h)
  const int r = kbner_set_max_lds_once(attr_done, reinterpret_cast<const void*>(KERNEL), AR_LDS_BYTES);
  if (r) return r;
  hipLaunchKernelGGL(KERNEL, grid, dim3(AT_NW * 64), AR_LDS_BYTES, stream, args...);
  KBNER_LAUNCH_RET();
}

// csrc/attention.hip's pick_rpw (static there, and that file stays as it is): the row tile kbner_attn_fwd gives a workgroup
static inline int full_rows_per_workgroup(int B, int S, int A) {
  int rpw = 512;
  while (rpw > 128 && (rpw / 2 >= S || (long)B * A * ((S + rpw - 1) / rpw) < 512)) rpw /= 2;
  return rpw;
}

extern "C" {

// qkv bf16 [>= B*S, 3H] ; maskbias f32 [B, S] ; q_pos i32 [B, nq] ; ctx_c bf16 [B*nq, H] ; o32 f32 [B*nq, H] ; lse_c f32 [B, A, nq]
// constraints: H = A * 64, S % 64 == 0, 64 <= S <= 512, nq >= 1 (include/kbner.h)
int kbner_attn_rows_fwd(const bf16_t* qkv, const float* maskbias, const int* q_pos, bf16_t* ctx_c, float* o32, float* lse_c, int B, int S,
                        int H, int A, int nq, uint32_t drop_seed, uint32_t drop_thresh, void* stream) {
  KBNER_CHECK_ARG(B > 0 && A > 0 && H == A * AT_D && S % 64 == 0 && S >= 64 && S <= AT_MAXS && nq >= 1 && B <= 65535);
  KBNER_CHECK_ARG(qkv != nullptr && maskbias != nullptr && q_pos != nullptr && ctx_c != nullptr && o32 != nullptr && lse_c != nullptr);
  const dim3 grid(A, B);
  hipStream_t st = (hipStream_t)stream;
  if (drop_thresh)
    return launch_rows<attn_rows_fwd_kernel<true>>(grid, st, qkv, maskbias, q_pos, ctx_c, o32, lse_c, S, H, A, nq, 0.125f, drop_seed, drop_thresh, 0);
  // where kbner_attn_fwd would run its 32-row kernel (csrc/attention.hip launch_attn_fwd: no dropout, S % 64 == 0, S >= 192, a row
  // tile of whole 32-row passes) the keys go in two halves there; followed here when a half is whole waves (S % 128 == 0)
  const int two_parts = (S >= 192 && S % 128 == 0 && full_rows_per_workgroup(B, S, A) % 256 == 0) ? 1 : 0;
  return launch_rows<attn_rows_fwd_kernel<false>>(grid, st, qkv, maskbias, q_pos, ctx_c, o32, lse_c, S, H, A, nq, 0.125f, drop_seed, drop_thresh,
                                                  two_parts);
}

// dctx_c bf16 [B*nq, H] (dO at the listed queries) ; o32, lse_c: what kbner_attn_rows_fwd wrote ; dqkv bf16 [>= B*S, 3H]: rows
// [0, B*S) are written, all of them ; dbias_qkv f32 [3H] (nullable): += column sums of dqkv
int kbner_attn_rows_bwd(const bf16_t* qkv, const int* q_pos, const bf16_t* dctx_c, const float* o32, const float* lse_c,
                        const float* maskbias, bf16_t* dqkv, int B, int S, int H, int A, int nq, uint32_t drop_seed, uint32_t drop_thresh,
                        float* dbias_qkv, void* stream) {
  KBNER_CHECK_ARG(B > 0 && A > 0 && H == A * AT_D && S % 64 == 0 && S >= 64 && S <= AT_MAXS && nq >= 1 && B <= 65535);
  KBNER_CHECK_ARG(qkv != nullptr && q_pos != nullptr && dctx_c != nullptr && o32 != nullptr && lse_c != nullptr && maskbias != nullptr &&
                  dqkv != nullptr);
  const dim3 grid(A, B);
  hipStream_t st = (hipStream_t)stream;
  // (csrc/attention.hip launch_attn_bwd: the 32-row kernels whenever the row tile gives each wave whole 32-row passes)
  const int fused = full_rows_per_workgroup(B, S, A) % 256 == 0 ? 1 : 0;
  if (drop_thresh)
    return launch_rows<attn_rows_bwd_kernel<true>>(grid, st, qkv, q_pos, dctx_c, o32, lse_c, maskbias, dqkv, dbias_qkv, S, H, A, nq, 0.125f,
                                                   drop_seed, drop_thresh, fused);
  return launch_rows<attn_rows_bwd_kernel<false>>(grid, st, qkv, q_pos, dctx_c, o32, lse_c, maskbias, dqkv, dbias_qkv, S, H, A, nq, 0.125f,
                                                  drop_seed, drop_thresh, fused);
}

}  // extern "C"
