// LSTM recurrence for gfx950 (training): the BiLSTM of the stacked tagger (`use_rnn: true`,
// flair/models/sequence_tagger_model.py:324-357,969-994 -> torch.nn.LSTM, trained by autograd in the reference) on frozen features.
// Two entry points next to csrc/lstm.hip, whose kernels stay as they are:
//   kbner_lstm_seq_train  the forward recurrence of kbner_lstm_seq that also keeps, per consumed gx row, what the backward pass
//                         needs: the post-activation gates, c_t and the h_{t-1} row it multiplied;
//   kbner_lstm_seq_bwd    back-propagation through time: one launch per time step from the last step to the first;
//   kbner_lstm_seq_bwd_init  the same walk for a recurrence started from a given state: c_prev of step 0 is c_0, and one more launch
//                         of the recurrent product alone produces the gradient of h_0.
//
// TRAINING CONTRACT of the row tables (gxi / outi i32 [steps, ndir, B]): prefix-active -- every (direction, sequence) is active
// (gxi >= 0) for steps 0 .. len - 1 and finished (-1) after -- and no (direction, gx row) is consumed twice: the saved state and
// dgx are kept per gx row.  kbner.stack.step_tables produces this form; the host wrapper checks it before upload, the library
// cannot (the tables live in device memory).  The forward starts from whatever h[0] and c hold on entry; kbner_lstm_seq_bwd takes
// them to be 0 (no gradient flows into an initial state), kbner_lstm_seq_bwd_init takes c_0 and returns d h_0 and d c_0.
//
// Backward step s for an active (d, b), with r = gxi[s], nx = gxi[s + 1] (-1 past the end or when finished), pv = gxi[s - 1]:
//   dh  = dout[outi[s]] (0 where outi < 0) + (nx >= 0 ? dgx[nx, d-block] . Whh_d : 0)          (sum over the 4Hp gate columns)
//   t   = tanh(c[r]) ;  c_prev = pv >= 0 ? c[pv] : c_0   (c_0 = 0 without an initial state)
//   dc  = dc_carry + dh o (1 - t^2)
//   di  = dc g i (1 - i) ;  df = dc c_prev f (1 - f) ;  dg = dc i (1 - g^2) ;  do = dh t o (1 - o)
//   dc_carry = dc f ;  dgx[r, d-block] = (di, df, dg, do)   (bf16)
// The matrix part mirrors the forward step: a workgroup of 4 waves owns 16 hidden units x all sequences of its batch chunk (NT
// tiles of 16), ONE 16x16 accumulator per tile (the forward has four, one per gate), K = 4Hp split over the waves in 64-wide
// slices, partial sums meet in LDS and wave `nt` finishes tile nt.  It reads WhhT bf16 [ndir, Hp, 4Hp] (the host transposes the
// bf16 shadow once per optimizer step), so both MFMA operands are k-contiguous 16-byte fragments; a step streams Whh once, as
// the forward step does.  Finished sequences touch nothing, rows of dgx no step consumes are left as they are (the caller
// zero-fills them: the weight-gradient GEMMs read every row), every element is written by exactly one lane: no atomics.
#include "common.h"
#include "lstm_act.h"

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// lstm_seq_step_kernel (csrc/lstm.hip) with three stores added: same K split, same LDS reduction, same cell update, so h, c and
// out are the inference kernel's bit for bit.
//   gates bf16 [rows_gx, ndir * 4Hp] ; cs f32 [rows_gx, ndir * Hp] ; hprev bf16 [rows_gx, ndir * Hp] : direction d's columns of row gxi
template <int NT>
__global__ __launch_bounds__(256) void lstm_seq_train_step_kernel(const bf16_t* __restrict__ gx, int ld_gx, const int* __restrict__ gxi,
                                                                 const bf16_t* __restrict__ whh, const bf16_t* __restrict__ h_in,
                                                                 bf16_t* __restrict__ h_out, float* __restrict__ c,
                                                                 bf16_t* __restrict__ out, int ldo, const int* __restrict__ out_col,
                                                                 const int* __restrict__ outi, int B, int Hp, int ndir,
                                                                 bf16_t* __restrict__ gates, float* __restrict__ cs,
                                                                 bf16_t* __restrict__ hprev) {
  __shared__ f4v red[4 * 4 * NT * 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.x * 16, d = blockIdx.y, b0 = blockIdx.z * (16 * NT);
  const bf16_t* wrow = whh + ((size_t)d * 4 * Hp + j0 + li) * Hp + g * 8;   // + q * Hp * Hp for gate q
  const size_t gstride = (size_t)Hp * Hp;
  const bf16_t* hrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int b = b0 + nt * 16 + li;
    hrow[nt] = h_in + ((size_t)d * B + (b < B ? b : B - 1)) * Hp + g * 8;
  }
  f4v acc[4][NT];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[q][nt] = (f4v){0.f, 0.f, 0.f, 0.f};
  s8v wf[2][4], hf[2][NT];
  auto load_slice = [&](int kk, s8v (&wv)[2][4], s8v (&hv)[2][NT]) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) hv[half][nt] = *reinterpret_cast<const s8v*>(hrow[nt] + kk + half * 32);
#pragma unroll
      for (int q = 0; q < 4; ++q) wv[half][q] = *reinterpret_cast<const s8v*>(wrow + q * gstride + kk + half * 32);
    }
  };
  int kk = w * 64;
  if (kk < Hp) load_slice(kk, wf, hf);
  for (; kk < Hp; kk += 256) {
    s8v wn[2][4], hn[2][NT];
    load_slice(kk + 256 < Hp ? kk + 256 : kk, wn, hn);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)   // D[unit g*4+r][sequence li of tile nt]
          acc[q][nt] = MFMA16(__builtin_bit_cast(bf16x8, wf[half][q]), __builtin_bit_cast(bf16x8, hf[half][nt]), acc[q][nt]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int q = 0; q < 4; ++q) wf[half][q] = wn[half][q];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) hf[half][nt] = hn[half][nt];
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) red[((w * 4 + q) * NT + nt) * 64 + lane] = acc[q][nt];
  __syncthreads();
  if (w >= NT) return;
  const int nt = w;
  const int b = b0 + nt * 16 + li;
  if (b >= B) return;
  const int row = gxi[d * B + b];
  const size_t sidx = ((size_t)d * B + b) * Hp + j0 + g * 4;
  if (row < 0) {   // finished sequence: carry the state
    *reinterpret_cast<uint2*>(h_out + sidx) = *reinterpret_cast<const uint2*>(h_in + sidx);
    return;
  }
  const bf16_t* gp = gx + (size_t)row * ld_gx + (size_t)d * 4 * Hp + j0 + g * 4;
  float pre[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f4v sum = red[((0 * 4 + q) * NT + nt) * 64 + lane];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) {
      const f4v p = red[((ww * 4 + q) * NT + nt) * 64 + lane];
      sum[0] += p[0];
      sum[1] += p[1];
      sum[2] += p[2];
      sum[3] += p[3];
    }
    const uint2 u = *reinterpret_cast<const uint2*>(gp + q * Hp);
    const f2v a = unpack2bf(u.x), bq = unpack2bf(u.y);
    pre[q][0] = sum[0] + a[0];
    pre[q][1] = sum[1] + a[1];
    pre[q][2] = sum[2] + bq[0];
    pre[q][3] = sum[3] + bq[1];
  }
  float4 cv = *reinterpret_cast<const float4*>(c + sidx);
  float cc[4] = {cv.x, cv.y, cv.z, cv.w}, hh[4];
  float act[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ig = sigmoid_f(pre[0][r]), fg = sigmoid_f(pre[1][r]), gg = tanh_f(pre[2][r]), og = sigmoid_f(pre[3][r]);
    cc[r] = fg * cc[r] + ig * gg;
    hh[r] = og * tanh_f(cc[r]);
    act[0][r] = ig;
    act[1][r] = fg;
    act[2][r] = gg;
    act[3][r] = og;
  }
  *reinterpret_cast<float4*>(c + sidx) = make_float4(cc[0], cc[1], cc[2], cc[3]);
  uint2 ho;
  ho.x = pack2bf(hh[0], hh[1]);
  ho.y = pack2bf(hh[2], hh[3]);
  *reinterpret_cast<uint2*>(h_out + sidx) = ho;
  const int orow = outi[d * B + b];
  if (orow >= 0) *reinterpret_cast<uint2*>(out + (size_t)orow * ldo + out_col[d] + j0 + g * 4) = ho;
  // what the backward pass reads
  bf16_t* sg = gates + (size_t)row * ndir * 4 * Hp + (size_t)d * 4 * Hp + j0 + g * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint2 u;
    u.x = pack2bf(act[q][0], act[q][1]);
    u.y = pack2bf(act[q][2], act[q][3]);
    *reinterpret_cast<uint2*>(sg + q * Hp) = u;
  }
  const size_t srow = (size_t)row * ndir * Hp + (size_t)d * Hp + j0 + g * 4;
  *reinterpret_cast<float4*>(cs + srow) = make_float4(cc[0], cc[1], cc[2], cc[3]);
  *reinterpret_cast<uint2*>(hprev + srow) = *reinterpret_cast<const uint2*>(h_in + sidx);
}

template <int NT>
static void lstm_seq_train_launch(const bf16_t* gx, int ld_gx, const int* gxi, const bf16_t* whh, const bf16_t* h_in, bf16_t* h_out,
                                  float* c, bf16_t* out, int ldo, const int* out_col, const int* outi, int B, int Hp, int ndir,
                                  bf16_t* gates, float* cs, bf16_t* hprev, hipStream_t stream) {
  hipLaunchKernelGGL(lstm_seq_train_step_kernel<NT>, dim3(Hp / 16, ndir, (B + 16 * NT - 1) / (16 * NT)), dim3(256), 0, stream, gx,
                     ld_gx, gxi, whh, h_in, h_out, c, out, ldo, out_col, outi, B, Hp, ndir, gates, cs, hprev);
}

// ---------------------------------------------------------------------------------------------------------------------------
// One backward time step.  grid (Hp / 16, ndir, ceil(B / (16 NT))); block 256.
//   dout  bf16 [rows_out, ldo] : gradient of `out`, direction d at column out_col[d]
//   gxi / gxi_next / gxi_prev / outi i32 [ndir, B] : this step's tables and its neighbours' (null at either end)
//   whht  bf16 [ndir, Hp, 4Hp] ; gates / cs as the forward saved them ; dc_carry f32 [ndir, B, Hp] in place
//   dgx   bf16 [rows_gx, ld_dgx] : row nx read (written by the previous launch), row r written
//   c0    f32 [ndir, B, Hp] or null : c_prev where gxi_prev gives none (the launch of step 0 alone passes it)
// H0 = true is the launch AFTER step 0: gxi_next = gxi = the tables of step 0, the same product dgx[gxi[0], d-block] . Whh_d and
// reduction, and the f32 sum goes to dh0 f32 [ndir, B, Hp] for every active (d, b); no gate arithmetic, nothing else is written.
template <int NT, bool H0>
__global__ __launch_bounds__(256) void lstm_seq_bwd_step_kernel(const bf16_t* __restrict__ dout, int ldo, const int* __restrict__ out_col,
                                                               const int* __restrict__ outi, const int* __restrict__ gxi,
                                                               const int* __restrict__ gxi_next, const int* __restrict__ gxi_prev,
                                                               const bf16_t* __restrict__ whht, const bf16_t* __restrict__ gates,
                                                               const float* __restrict__ cs, float* __restrict__ dc_carry,
                                                               bf16_t* dgx, int ld_dgx, int B, int Hp, int ndir,
                                                               const float* __restrict__ c0, float* __restrict__ dh0) {
  __shared__ f4v red[4 * NT * 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.x * 16, d = blockIdx.y, b0 = blockIdx.z * (16 * NT);
  const int K = 4 * Hp;
  const bf16_t* wrow = whht + ((size_t)d * Hp + j0 + li) * K + g * 8;
  const bf16_t* drow[NT];   // the dgx row of the NEXT step of this lane's sequence (null: none, the recurrent term is 0)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int b = b0 + nt * 16 + li;
    const int nx = (gxi_next != nullptr && b < B) ? gxi_next[d * B + b] : -1;
    drow[nt] = nx >= 0 ? dgx + (size_t)nx * ld_dgx + (size_t)d * K + g * 8 : nullptr;
  }
  f4v acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = (f4v){0.f, 0.f, 0.f, 0.f};
  s8v wf[2], df[2][NT];
  auto load_slice = [&](int kk, s8v (&wv)[2], s8v (&dv)[2][NT]) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        dv[half][nt] = drow[nt] != nullptr ? *reinterpret_cast<const s8v*>(drow[nt] + kk + half * 32) : (s8v){0, 0, 0, 0, 0, 0, 0, 0};
      wv[half] = *reinterpret_cast<const s8v*>(wrow + kk + half * 32);
    }
  };
  int kk = w * 64;   // K = 4Hp >= 256: every wave owns at least one slice
  load_slice(kk, wf, df);
  for (; kk < K; kk += 256) {
    s8v wn[2], dn[2][NT];
    load_slice(kk + 256 < K ? kk + 256 : kk, wn, dn);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)   // D[unit g*4+r][sequence li of tile nt]
        acc[nt] = MFMA16(__builtin_bit_cast(bf16x8, wf[half]), __builtin_bit_cast(bf16x8, df[half][nt]), acc[nt]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      wf[half] = wn[half];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) df[half][nt] = dn[half][nt];
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) red[(w * NT + nt) * 64 + lane] = acc[nt];
  __syncthreads();
  if (w >= NT) return;
  const int nt = w;
  const int b = b0 + nt * 16 + li;
  if (b >= B) return;
  const int row = gxi[d * B + b];
  if (row < 0) return;   // finished sequence: touches nothing
  f4v dh = red[(0 * NT + nt) * 64 + lane];
#pragma unroll
  for (int ww = 1; ww < 4; ++ww) {
    const f4v p = red[(ww * NT + nt) * 64 + lane];
    dh[0] += p[0];
    dh[1] += p[1];
    dh[2] += p[2];
    dh[3] += p[3];
  }
  const size_t sidx = ((size_t)d * B + b) * Hp + j0 + g * 4;
  if constexpr (H0) {
    *reinterpret_cast<float4*>(dh0 + sidx) = make_float4(dh[0], dh[1], dh[2], dh[3]);
    return;
  }
  const int orow = outi[d * B + b];
  if (orow >= 0) {
    const uint2 u = *reinterpret_cast<const uint2*>(dout + (size_t)orow * ldo + out_col[d] + j0 + g * 4);
    const f2v a = unpack2bf(u.x), bq = unpack2bf(u.y);
    dh[0] += a[0];
    dh[1] += a[1];
    dh[2] += bq[0];
    dh[3] += bq[1];
  }
  const bf16_t* sg = gates + (size_t)row * ndir * K + (size_t)d * K + j0 + g * 4;
  float act[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint2 u = *reinterpret_cast<const uint2*>(sg + q * Hp);
    const f2v a = unpack2bf(u.x), bq = unpack2bf(u.y);
    act[q][0] = a[0];
    act[q][1] = a[1];
    act[q][2] = bq[0];
    act[q][3] = bq[1];
  }
  const size_t coff = (size_t)d * Hp + j0 + g * 4;
  const float4 cv = *reinterpret_cast<const float4*>(cs + (size_t)row * ndir * Hp + coff);
  const int pv = gxi_prev != nullptr ? gxi_prev[d * B + b] : -1;
  const float4 cpv = pv >= 0           ? *reinterpret_cast<const float4*>(cs + (size_t)pv * ndir * Hp + coff)
                     : c0 != nullptr ? *reinterpret_cast<const float4*>(c0 + sidx)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 carry = *reinterpret_cast<const float4*>(dc_carry + sidx);
  const float cc[4] = {cv.x, cv.y, cv.z, cv.w}, cp[4] = {cpv.x, cpv.y, cpv.z, cpv.w};
  float dcn[4] = {carry.x, carry.y, carry.z, carry.w}, dg4[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ig = act[0][r], fg = act[1][r], gg = act[2][r], og = act[3][r];
    const float t = tanh_f(cc[r]);
    const float dc = dcn[r] + dh[r] * og * (1.0f - t * t);
    dg4[0][r] = dc * gg * ig * (1.0f - ig);
    dg4[1][r] = dc * cp[r] * fg * (1.0f - fg);
    dg4[2][r] = dc * ig * (1.0f - gg * gg);
    dg4[3][r] = dh[r] * t * og * (1.0f - og);
    dcn[r] = dc * fg;
  }
  *reinterpret_cast<float4*>(dc_carry + sidx) = make_float4(dcn[0], dcn[1], dcn[2], dcn[3]);
  bf16_t* dp = dgx + (size_t)row * ld_dgx + (size_t)d * K + j0 + g * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint2 u;
    u.x = pack2bf(dg4[q][0], dg4[q][1]);
    u.y = pack2bf(dg4[q][2], dg4[q][3]);
    *reinterpret_cast<uint2*>(dp + q * Hp) = u;
  }
}

template <int NT, bool H0>
static void lstm_seq_bwd_launch(const bf16_t* dout, int ldo, const int* out_col, const int* outi, const int* gxi, const int* gxi_next,
                                const int* gxi_prev, const bf16_t* whht, const bf16_t* gates, const float* cs, float* dc_carry,
                                bf16_t* dgx, int ld_dgx, int B, int Hp, int ndir, const float* c0, float* dh0, hipStream_t stream) {
  hipLaunchKernelGGL((lstm_seq_bwd_step_kernel<NT, H0>), dim3(Hp / 16, ndir, (B + 16 * NT - 1) / (16 * NT)), dim3(256), 0, stream, dout,
                     ldo, out_col, outi, gxi, gxi_next, gxi_prev, whht, gates, cs, dc_carry, dgx, ld_dgx, B, Hp, ndir, c0, dh0);
}

template <bool H0>
static void lstm_seq_bwd_dispatch(const bf16_t* dout, int ldo, const int* out_col, const int* oi, const int* gi, const int* gn,
                                  const int* gp, const bf16_t* whht, const bf16_t* gates, const float* cs, float* dc_carry, bf16_t* dgx,
                                  int ld_dgx, int B, int Hp, int ndir, const float* c0, float* dh0, hipStream_t st) {
  if (B <= 16)
    lstm_seq_bwd_launch<1, H0>(dout, ldo, out_col, oi, gi, gn, gp, whht, gates, cs, dc_carry, dgx, ld_dgx, B, Hp, ndir, c0, dh0, st);
  else if (B <= 32)
    lstm_seq_bwd_launch<2, H0>(dout, ldo, out_col, oi, gi, gn, gp, whht, gates, cs, dc_carry, dgx, ld_dgx, B, Hp, ndir, c0, dh0, st);
  else if (B <= 48)
    lstm_seq_bwd_launch<3, H0>(dout, ldo, out_col, oi, gi, gn, gp, whht, gates, cs, dc_carry, dgx, ld_dgx, B, Hp, ndir, c0, dh0, st);
  else
    lstm_seq_bwd_launch<4, H0>(dout, ldo, out_col, oi, gi, gn, gp, whht, gates, cs, dc_carry, dgx, ld_dgx, B, Hp, ndir, c0, dh0, st);
}

// the walk of kbner_lstm_seq_bwd and kbner_lstm_seq_bwd_init: c0 reaches the launch of step 0 alone, dh0 adds one launch after it
static int lstm_seq_bwd_run(const bf16_t* dout, int ldo, const int* out_col, const int* outi, const int* gxi, const bf16_t* whht,
                            const bf16_t* gates, const float* cs, const float* c0, float* dc_carry, bf16_t* dgx, int ld_dgx, float* dh0,
                            int steps, int B, int Hp, int ndir, void* stream) {
  KBNER_CHECK_ARG(dout != nullptr && out_col != nullptr && outi != nullptr && gxi != nullptr && whht != nullptr && gates != nullptr &&
                  cs != nullptr && dc_carry != nullptr && dgx != nullptr);
  KBNER_CHECK_ARG(steps >= 0 && B > 0 && ndir > 0 && Hp > 0 && Hp % 64 == 0 && ldo % 4 == 0 && ld_dgx % 8 == 0 &&
                  (long long)ld_dgx >= (long long)ndir * 4 * Hp);
  const int per = ndir * B;
  hipStream_t st = (hipStream_t)stream;
  for (int s = steps - 1; s >= 0; --s) {
    const int* gi = gxi + (size_t)s * per;
    const int* gn = s + 1 < steps ? gi + per : nullptr;
    const int* gp = s > 0 ? gi - per : nullptr;
    const int* oi = outi + (size_t)s * per;
    lstm_seq_bwd_dispatch<false>(dout, ldo, out_col, oi, gi, gn, gp, whht, gates, cs, dc_carry, dgx, ld_dgx, B, Hp, ndir,
                                 s == 0 ? c0 : nullptr, nullptr, st);
  }
  if (steps > 0 && dh0 != nullptr)
    lstm_seq_bwd_dispatch<true>(dout, ldo, out_col, outi, gxi, gxi, nullptr, whht, gates, cs, dc_carry, dgx, ld_dgx, B, Hp, ndir, nullptr,
                                dh0, st);
  KBNER_LAUNCH_RET();
}

extern "C" {

// kbner_lstm_seq that also saves what kbner_lstm_seq_bwd reads.  Arguments and constraints of kbner_lstm_seq, the training contract
// of the row tables (top of this file), and gates bf16 [rows_gx, ndir * 4Hp], cs f32 [rows_gx, ndir * Hp], hprev bf16
// [rows_gx, ndir * Hp]: for an active (d, b) with r = gxi[s, d, b], direction d's columns of row r receive the post-activation
// gates (i | f | g | o), c_t and the h_{t-1} row the step multiplied.  Rows no step consumes are left as they are.
int kbner_lstm_seq_train(const bf16_t* gx, int ld_gx, const int* gxi, const bf16_t* whh, bf16_t* h, float* c, bf16_t* out, int ldo,
                         const int* out_col, const int* outi, int steps, int B, int Hp, int ndir, bf16_t* gates, float* cs,
                         bf16_t* hprev, void* stream) {
  KBNER_CHECK_ARG(gx != nullptr && gxi != nullptr && whh != nullptr && h != nullptr && c != nullptr && out != nullptr &&
                  out_col != nullptr && outi != nullptr && gates != nullptr && cs != nullptr && hprev != nullptr);
  KBNER_CHECK_ARG(steps >= 0 && B > 0 && ndir > 0 && Hp > 0 && Hp % 64 == 0 && ld_gx % 4 == 0 && ldo % 4 == 0);
  const size_t hs = (size_t)ndir * B * Hp;
  const int per = ndir * B;
  hipStream_t st = (hipStream_t)stream;
  for (int s = 0; s < steps; ++s) {
    const bf16_t* h_in = h + (size_t)(s & 1) * hs;
    bf16_t* h_out = h + (size_t)((s + 1) & 1) * hs;
    const int* gi = gxi + (size_t)s * per;
    const int* oi = outi + (size_t)s * per;
    if (B <= 16)
      lstm_seq_train_launch<1>(gx, ld_gx, gi, whh, h_in, h_out, c, out, ldo, out_col, oi, B, Hp, ndir, gates, cs, hprev, st);
    else if (B <= 32)
      lstm_seq_train_launch<2>(gx, ld_gx, gi, whh, h_in, h_out, c, out, ldo, out_col, oi, B, Hp, ndir, gates, cs, hprev, st);
    else if (B <= 48)
      lstm_seq_train_launch<3>(gx, ld_gx, gi, whh, h_in, h_out, c, out, ldo, out_col, oi, B, Hp, ndir, gates, cs, hprev, st);
    else
      lstm_seq_train_launch<4>(gx, ld_gx, gi, whh, h_in, h_out, c, out, ldo, out_col, oi, B, Hp, ndir, gates, cs, hprev, st);
  }
  KBNER_LAUNCH_RET();
}

// Back-propagation through the recurrence kbner_lstm_seq_train ran: `steps` launches, step steps - 1 first, enqueued back to back.
//   dout bf16 [rows_out, ldo], out_col, outi, gxi: the gradient of `out` and the forward's tables
//   whht bf16 [ndir, Hp, 4Hp]: Whh of every direction transposed ;  gates / cs: what the forward saved
//   dc_carry f32 [ndir, B, Hp]: zero on entry (or the gradient of the final c), the gradient of c_0 on return
//   dgx bf16 [rows_gx, ld_dgx]: receives the gradient of gx at every consumed (row, direction block); other rows untouched
// Constraints: Hp % 64 == 0, ldo % 4 == 0, ld_dgx % 8 == 0, ld_dgx >= ndir * 4Hp, out_col[d] % 4 == 0.
int kbner_lstm_seq_bwd(const bf16_t* dout, int ldo, const int* out_col, const int* outi, const int* gxi, const bf16_t* whht,
                       const bf16_t* gates, const float* cs, float* dc_carry, bf16_t* dgx, int ld_dgx, int steps, int B, int Hp,
                       int ndir, void* stream) {
  return lstm_seq_bwd_run(dout, ldo, out_col, outi, gxi, whht, gates, cs, nullptr, dc_carry, dgx, ld_dgx, nullptr, steps, B, Hp, ndir,
                          stream);
}

// kbner_lstm_seq_bwd for a recurrence that started from a state (h_0, c_0) instead of zeros.
//   c0  f32 [ndir, B, Hp] or null: the c the forward started from; c_prev of step 0 (null: 0)
//   dh0 f32 [ndir, B, Hp] or null: receives, after step 0, dgx[gxi[0, d, b], d-block] . Whh_d -- the gradient of h_0 -- for every
//       (d, b) with gxi[0, d, b] >= 0; other entries are untouched
// dc_carry on return is the gradient of c_0.  With c0 and dh0 null: the launches and results of kbner_lstm_seq_bwd.
int kbner_lstm_seq_bwd_init(const bf16_t* dout, int ldo, const int* out_col, const int* outi, const int* gxi, const bf16_t* whht,
                            const bf16_t* gates, const float* cs, const float* c0, float* dc_carry, bf16_t* dgx, int ld_dgx, float* dh0,
                            int steps, int B, int Hp, int ndir, void* stream) {
  return lstm_seq_bwd_run(dout, ldo, out_col, outi, gxi, whht, gates, cs, c0, dc_carry, dgx, ld_dgx, dh0, steps, B, Hp, ndir, stream);
}

}  // extern "C"
