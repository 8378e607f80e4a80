// Shared pieces of the 256-column-tile bf16 MFMA GEMM kernels (gemm256.hip; the lab kernels of tools/experiments/): problem
// descriptors, LDS-DMA issue helpers, LDS image swizzles and fragment reads, the XCD-aware tile walk.  gfx950 only.
// Each piece exists once; tools/isa_diff.py holds a change here to the letter of every kernel's device assembly, which is why a few
// pieces are macros or are called piece by piece where a function would do: hipcc's instruction order follows the statement order.
#pragma once
#include "common.h"
#include "gemm_epi.h"

#define G2_MAXP 16
#ifndef KBNER_GEMM_VARIANT_DEFAULT
#define KBNER_GEMM_VARIANT_DEFAULT 3
#endif

struct GemmProblem {
  const bf16_t* A;
  const bf16_t* B;
  bf16_t* C;
  float* C32;
  const float* bias;
  const bf16_t* addend;
  const bf16_t* aux;
  bf16_t* out2;
  float* colsum;
  int M, N, K;
  int lda, ldb, ldc, ldc32, ldadd, ldaux, ldout2;
  int epi;
  float alpha;
  int tile_begin;
  uint32_t drop_seed;
  uint32_t drop_thresh;
  int pad_;
};

struct GroupArgs {
  int nprob;
  int total_tiles;
  int ncu;
  int pad_;
  int* sched;  // dynamic tile scheduling (DYN kernels): 8 per-XCD counters, zeroed by the caller before the launch
  int tile_begin[G2_MAXP];  // compact copy of p[i].tile_begin: one s_load_dwordx16 picks the problem
  GemmProblem p[G2_MAXP];
};

#define T2 256
#define BK2 64
#define TILE2_BYTES 32768
#define STAGE2_BYTES 65536
#define G2_LDS_BYTES (2 * STAGE2_BYTES + 8 * 4096)  // two operand stages + two 2-KiB epilogue transpose buffers per wave

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_cvoid;

// LDS-DMA issued from inline asm so the compiler does not see it: with a compiler-visible
// global_load_lds in flight hipcc (ROCm 7.2) degrades every ds_read wait in the loop to lgkmcnt(0)
// (mixed pending LGKM event types), which serialises the fragment stream behind full LDS latency.
// The DMA's completion is ordered by hand: s_waitcnt vmcnt(0) + barrier before the stage is read.
// Address form: wave-uniform 64-bit base in SGPRs + per-lane 32-bit byte offset.  The per-lane part is
// loop-invariant, so only 8 VGPRs (not 8 x 64-bit pointers) stay live across the MFMA loop.
// A wave's 2 or 4 consecutive 1-KiB pieces under ONE M0 write: the instruction's immediate offset advances BOTH the LDS and the
// global address by j KiB, so the j-th per-lane offset is passed as voff_j - j * 1024 (what stage_voff returns; never negative: a
// piece step is >= 1 KiB of source bytes for every image, ld >= 64).  Saves three of the four (s_mov m0 / s_nop) sequences per
// operand tile.  dst: the wave-uniform LDS byte address of piece 0.
// (m0 is declared clobbered instead of being saved and restored: nothing else in these kernels keeps a value in it)
static __device__ __forceinline__ void glds16_quad(const void* sbase, unsigned v0, unsigned v1, unsigned v2, unsigned v3, unsigned dst) {
  asm volatile(
      "s_mov_b32 m0, %5\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %4\n\t"
      "global_load_lds_dwordx4 %1, %4 offset:1024\n\t"
      "global_load_lds_dwordx4 %2, %4 offset:2048\n\t"
      "global_load_lds_dwordx4 %3, %4 offset:3072"
      :
      : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(sbase), "s"(dst)
      : "memory", "m0");
}
// IMM0: the first piece spells its zero immediate out.  Same encoding; the two-stage loop's half-height A tile was written without
// it and the ring kernels with it, and the device assembly of both is held to the letter (tools/isa_diff.py).
#define GLDS16_PAIR_ASM(I0, I1)                                                                                             \
  asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2" I0 "\n\tglobal_load_lds_dwordx4 %1, %2" I1 \
               :                                                                                                            \
               : "v"(v0), "v"(v1), "s"(sbase), "s"(dst)                                                                     \
               : "memory", "m0")
template <bool IMM0 = true>
static __device__ __forceinline__ void glds16_pair(const void* sbase, unsigned v0, unsigned v1, unsigned dst) {
  if constexpr (IMM0) GLDS16_PAIR_ASM(" offset:0", " offset:0x400");
  else GLDS16_PAIR_ASM("", " offset:1024");
}
#undef GLDS16_PAIR_ASM
// piece J of the four, with its own M0 write (two scalar instructions: free between two MFMAs)
template <int J>
static __device__ __forceinline__ void glds16_piece(const void* sbase, unsigned voff, unsigned dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3"
               :
               : "v"(voff), "s"(sbase), "s"(dst), "n"(J * 1024)
               : "memory", "m0");
}
static __device__ __forceinline__ int kc_swz(int row) { return (row >> 1) & 7; }
static __device__ __forceinline__ int ks_swz(int krow) { return (krow & 3) | ((krow >> 1) & 4); }
// B operand, KC image: a fragment's 16 lanes read rows {8a + 4h + c : a,c in 0..3} of a 32-row block (the column
// permutation below), so the conflict-free chunk swizzle keys on row bits 4,3 and 1
static __device__ __forceinline__ int kcb_swz(int row) { return (((row >> 3) & 3) << 1) | ((row >> 1) & 1); }

// Output-column permutation: MFMA fragment ni (0..3) of a wave's 64 columns takes operand row j (= lane & 15) from
// column (ni>>1)*32 + (j>>2)*8 + (ni&1)*4 + (j&3).  With the operand-swapped MFMA a lane then owns 8 CONTIGUOUS
// output columns per fragment pair (g*8 .. g*8+7 of each 32-column block): every epilogue access is 16 bytes
// (dwordx4) instead of 8 -- the row-per-lane store tail is issue-bound, halving the instruction count halves it.

// the per-lane source byte offset of 1-KiB piece q of an operand tile: 8 rows x 128 B of a row-major (KC) image, 2 k rows x 512 B
// of a k-strided one, chunk-swizzled
template <bool KS, bool ISB>
static __device__ __forceinline__ unsigned piece_voff(int q, int ld, int lane) {
  if (!KS) {
    const int row = q * 8 + (lane >> 3);
    const int pos = lane & 7;
    return (unsigned)(row * ld + ((pos ^ (ISB ? kcb_swz(row) : kc_swz(row))) << 3)) * 2u;
  } else {
    const int kr = q * 2 + (lane >> 5);
    const int pos = lane & 31;
    return (unsigned)(kr * ld + ((pos ^ (ks_swz(kr) << 1)) << 3)) * 2u;
  }
}
// ... of a wave's NP consecutive pieces of a tile of NP * 64 rows (NP * 8 wave-instructions x 1 KiB: 32 KiB for a 256-row tile);
// piece j's offset already carries the - j KiB of its instruction's immediate offset, see glds16_quad
template <bool KS, bool ISB, int NP>
static __device__ __forceinline__ void stage_voff(int ld, int wid, int lane, unsigned (&voff)[NP]) {
#pragma unroll
  for (int j = 0; j < NP; ++j) voff[j] = piece_voff<KS, ISB>(wid * NP + j, ld, lane) - (unsigned)j * 1024u;
}

template <bool KS, bool ISB, int ROWS = 256>
static __device__ __forceinline__ void stage256(const bf16_t* __restrict__ P, int ld, int row0, int k0, unsigned char* s, int wid,
                                                int lane) {
  static_assert(ROWS == 256 || (ROWS == 128 && !KS), "half-height tiles exist for the row-major (KC) A image only");
  // uniform tile origin in SGPRs
  const bf16_t* sbase = KS ? P + (size_t)k0 * ld + row0 : P + (size_t)row0 * ld + k0;
  // (the - j KiB at the issue, not through stage_voff: that gives the same instructions in another order)
  unsigned voff[ROWS / 64];
#pragma unroll
  for (int j = 0; j < ROWS / 64; ++j) voff[j] = piece_voff<KS, ISB>(wid * (ROWS / 64) + j, ld, lane);
  // this wave's pieces are consecutive in the image
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_void*)(s + wid * (ROWS / 64) * 1024));
  if constexpr (ROWS == 256) glds16_quad(sbase, voff[0], voff[1] - 1024u, voff[2] - 2048u, voff[3] - 3072u, dst);
  else glds16_pair<false>(sbase, voff[0], voff[1] - 1024u, dst);
}

// the two transposed 8-byte reads of a k-strided fragment: k rows r and r + 4 of the image, 4 x 512 B apart
typedef s4v __attribute__((address_space(3))) lds_s4v;
static __device__ __forceinline__ bf16x8 tr_pair(lds_s4v* p_lo, lds_s4v* p_hi) {
  const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p_lo);
#if defined(RF_EXP_HALFTR)     /* timing only (wrong operands): one transposed read per fragment instead of two */
  const s4v hi = lo;
#else
  const s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p_hi);
#endif
  s8v v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf16x8, v);
}
static __device__ __forceinline__ bf16x8 tr_pair(const unsigned char* a) { return tr_pair((lds_s4v*)(a), (lds_s4v*)(a + 4 * 512)); }
static __device__ __forceinline__ bf16x8 tr_pair(unsigned addr) {   // an LDS byte address
  return tr_pair((lds_s4v*)(size_t)addr, (lds_s4v*)(size_t)(addr + 4u * 512u));
}

template <bool KS>
static __device__ __forceinline__ bf16x8 frag256(const unsigned char* s, int r0, int ks, int lane) {
  if (!KS) {
    const int row = r0 + (lane & 15);
    const int c = ks * 4 + (lane >> 4);
    const s8v v = *reinterpret_cast<const s8v*>(s + row * 128 + ((c ^ kc_swz(row)) << 4));
    return __builtin_bit_cast(bf16x8, v);
  } else {
    const int p = lane & 15;
    const int r = ks * 32 + (lane >> 4) * 8 + (p >> 2);
    return tr_pair(s + r * 512 + ((((r0 >> 4) ^ ks_swz(r))) << 5) + ((p & 3) << 3));
  }
}

// B-operand fragment ni of the wave whose columns start at c0 (see the permutation note above)
template <bool KS>
static __device__ __forceinline__ bf16x8 fragB256(const unsigned char* s, int c0, int ni, int ks, int lane) {
  if (!KS) {
    const int j = lane & 15;
    const int row = c0 + (ni >> 1) * 32 + (j >> 2) * 8 + (ni & 1) * 4 + (j & 3);
    const int c = ks * 4 + (lane >> 4);
    const s8v v = *reinterpret_cast<const s8v*>(s + row * 128 + ((c ^ kcb_swz(row)) << 4));
    return __builtin_bit_cast(bf16x8, v);
  } else {
    const int p = lane & 15;
    const int r = ks * 32 + (lane >> 4) * 8 + (p >> 2);
    const int col = c0 + (ni >> 1) * 32 + (p & 3) * 8 + (ni & 1) * 4;  // this lane's 4-column piece
    return tr_pair(s + r * 512 + ((((col >> 4) ^ ks_swz(r))) << 5) + ((col & 15) << 1));
  }
}

// linear id -> (problem, tile origin), in two halves so that a kernel may pick a tile ONCE and hand the record on.
// pick_problem: the XCD-aware bijective remap (block b runs on XCD b % 8; persistent ids keep id % 8): each XCD's private L2 sees
// a contiguous run of tiles, n fastest, so neighbours share the A panel; then which problem the remapped id falls into, with
// static indices only (a runtime-indexed kernarg array would go to scratch) and no memory access.
static __device__ __forceinline__ void pick_problem(const GroupArgs& ga, int id, int total, int& pi, int& wg) {
  const int xcd = id & 7;
  const int q8 = total >> 3, r8 = total & 7;
  wg = ((xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
  pi = 0;
#pragma unroll
  for (int i = 1; i < G2_MAXP; ++i)
    if (wg >= ga.tile_begin[i]) pi = i;  // unused slots hold INT_MAX
}
// the descriptor itself is read from the kernarg segment with a RUNTIME index (scalar loads); selecting it
// from by-value kernargs makes hipcc preload all 16 descriptors into ~500 SGPRs and spill them
static __device__ __forceinline__ const GemmProblem* problem_ptr(int pi) {
  return &((const GroupArgs*)__builtin_amdgcn_kernarg_segment_ptr())->p[pi];
}
// a wave-uniform pointer that the compiler computed with vector instructions (64-bit multiply-add), back in scalar registers:
// the "s" operands of the LDS-DMA inline asm are not legalised by hipcc
static __device__ __forceinline__ const bf16_t* uniform_ptr(const bf16_t* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const bf16_t*)(((unsigned long long)hi << 32) | lo);
}
// Grouped (8 tile-rows at a time, column-major inside the group) ordering: the ~32 tiles an XCD works on concurrently
// then form an 8 x 4 patch that shares 8 A panels and 4 B panels through that XCD's L2, instead of a 1 x 32 strip that
// shares one A panel and streams 32 different B panels from MALL/HBM (measured: the strip order is fabric-bound).
template <int TM = 256>
static __device__ __forceinline__ void tile_origin(int tile, int M, int N, int& m0, int& n0) {
  const int tiles_n = N / T2, tiles_m = M / TM;
  const int group = 8 * tiles_n;
  const int first_m = (tile / group) * 8;
  const int gm = min(tiles_m - first_m, 8);
  const int r = tile % group;
  m0 = (first_m + r % gm) * TM;
  n0 = (r / gm) * T2;
}
template <int TM = 256>
static __device__ __forceinline__ void pick_tile(const GroupArgs& ga, int id, int total, GemmProblem& g, int& m0, int& n0) {
  int pi, wg;
  pick_problem(ga, id, total, pi, wg);
  g = *problem_ptr(pi);
  tile_origin<TM>(wg - g.tile_begin, g.M, g.N, m0, n0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Round 4: the ring main loop (gemm256f_kernel).  LDS = 3 A slots + 2 B slots of 32 KiB (one K = 64 operand tile each).
#define PP_B_BASE (3 * TILE2_BYTES)
#define PP_LDS_BYTES (5 * TILE2_BYTES)

static __device__ __forceinline__ void pp_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}

// The ring kernels' (gemm256f_kernel, gemm128i_kernel) fragment read addresses, the fragment maps of frag256 / fragB256.  Macros, not
// functions: as functions they give the same instructions in another order (tools/isa_diff.py).
// Lane bases: this lane's address of row block 0, k half 0 -- A in the slot at LDS byte address lds0 for a wave of A_ROWS rows, B in
// the slot at b_base.
#define RING_LANE_BASES(A_KS, B_KS, A_ROWS, b_base, lane)                                                        \
  {                                                                                                              \
    if (!A_KS) {                                                                                                 \
      const int row = wm * A_ROWS + (lane & 15);                                                                 \
      laneA = lds0 + row * 128 + ((((lane >> 4)) ^ kc_swz(row)) << 4);                                           \
    } else { /* k-strided image: k row r, 32-byte block (row block ^ swizzle): the row block mi enters by XOR, see ring_frag_a */ \
      const int p = lane & 15;                                                                                   \
      const int r = (lane >> 4) * 8 + (p >> 2);                                                                  \
      laneA = lds0 + r * 512 + ((p & 3) << 3) + wm * (A_ROWS * 2) + (ks_swz(r) << 5);                            \
    }                                                                                                            \
    if (!B_KS) {                                                                                                 \
      const int j = lane & 15;                                                                                   \
      const int row = wn * 64 + (j >> 2) * 8 + (j & 3);                                                          \
      laneB = b_base + row * 128 + ((((lane >> 4)) ^ kcb_swz(row)) << 4);                                        \
    } else {                                                                                                     \
      const int p = lane & 15;                                                                                   \
      const int r = (lane >> 4) * 8 + (p >> 2);                                                                  \
      laneB = b_base + r * 512 + (((wn * 4 + ((p & 3) >> 1)) ^ ks_swz(r)) << 5) + (((p & 3) & 1) << 4);          \
    }                                                                                                            \
  }
// The address registers of a K step, from the lane bases and the offsets of the slots being consumed.  Row-major (KC) images: ONE
// address register per operand and k half for the whole step -- the row block (A: mi * 2 KiB, B: (ni >> 1) * 4 KiB + (ni & 1) *
// 512 B) is the ds_read's immediate offset and k half 1 is k half 0 with bit 6 flipped (the chunk swizzles only look at row bits the
// row block does not touch) -- made opaque so that hipcc keeps this form (left alone it hoists eight per-row-block registers out of
// the loop and adds the slot offset to each: two VALU instructions per read, each of which takes the matrix pipe's issue port)
#define RING_STEP_BASES(A_KS)                                    \
  {                                                              \
    pa0 = laneA + sa_off;                                        \
    asm volatile("" : "+v"(pa0));                                \
    if (!A_KS) {                                                 \
      pa1 = pa0 ^ 64u;                                           \
      asm volatile("" : "+v"(pa1));                              \
    }                                                            \
    pb0 = laneB + sb_off;                                        \
    asm volatile("" : "+v"(pb0));                                \
    pb1 = pb0 ^ 64u;                                             \
    asm volatile("" : "+v"(pb1));                                \
  }

// A fragment (k half ks, row block mi) and B fragment (k half ks, column fragment ni) from those registers
typedef const s8v __attribute__((address_space(3))) lds_s8v;
template <bool KS>
static __device__ __forceinline__ bf16x8 ring_frag_a(unsigned pa0, unsigned pa1, int ks, int mi) {
  if constexpr (!KS) {
    const s8v v = *reinterpret_cast<lds_s8v*>((size_t)((ks ? pa1 : pa0) + (unsigned)mi * 2048u));
    return __builtin_bit_cast(bf16x8, v);
  } else {
    // (block ^ swizzle) << 5 with block = 8 wm + mi: the low three bits of the block are mi, so the row block is an XOR on
    // address bits 5-7 (one VALU instruction per fragment; the k half is an immediate: 32 k rows x 512 B)
#if defined(RF_EXP_NOXOR)      /* timing only (wrong operands): what do the 16 address XORs of a TN K step cost? */
    return tr_pair(pa0 + (unsigned)mi * 32u + (unsigned)ks * 16384u);
#else
    return tr_pair((pa0 ^ ((unsigned)mi << 5)) + (unsigned)ks * 16384u);
#endif
  }
}
template <bool KS>
static __device__ __forceinline__ bf16x8 ring_frag_b(unsigned pb0, unsigned pb1, int ks, int ni) {
  if constexpr (!KS) {
    const s8v v = *reinterpret_cast<lds_s8v*>((size_t)((ks ? pb1 : pb0) + (unsigned)((ni >> 1) * 4096 + (ni & 1) * 512)));
    return __builtin_bit_cast(bf16x8, v);
  } else {
    // column block (4 wn + 2 (ni >> 1) + ...) ^ swizzle: ni >> 1 flips address bit 6 (pb1), ni & 1 adds 8 bytes
    return tr_pair(((ni >> 1) ? pb1 : pb0) + (unsigned)ks * 16384u + (unsigned)(ni & 1) * 8u);
  }
}
