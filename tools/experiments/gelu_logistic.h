// Round 4 experiment, rejected: gelu / gelu' through ONE logistic per element instead of the erf series of kb-ner_amd/csrc/common.h
// (gelu2 / gelu_both2, which stay):
//     Phi(x) ~= s(x) = 1 / (1 + exp(-(x (p0 + p1 x^2 + p2 x^4))))        gelu = x s,   gelu' = s + x s (1 - s) (p0 + 3 p1 x^2 + 5 p2 x^4)
// p fitted (minimax) to |gelu error| <= 3.8e-5 and |gelu' error| <= 9.3e-5 in fp32, 11 packed fp32 operations + 2 v_exp + 2 v_rcp per
// element PAIR instead of 17 + 4.  Measured on one box, alternating processes: 945.1 / 945.1 sentences/s against 945.0 / 943.0 with
// the erf series -- 4 of the ~30 vector instructions per element pair of an epilogue that is one of nine GEMMs: 0.3 %
// of the step, inside the noise.  No measurable speed for a 250 times larger error: rejected.
// x^2 is clamped at 36: beyond |x| = 6 the fit's polynomial is not monotone, s is 0 / 1 to 1e-9 there.
// Lab builds only (README.md here): force-included in front of a GEMM source with -DKBNER_GELU_LOGISTIC, it sends that source's
// gelu2 / gelu_both2 calls to the logistic forms.
#pragma once
#include "common.h"

#define KBNER_GELU_P0 1.59484492f
#define KBNER_GELU_P1 7.40112029e-02f
#define KBNER_GELU_P2 -6.97126291e-04f
static __device__ __forceinline__ void gelu_logistic2(f2v x, f2v& sg, f2v& x2c) {
  const f2v x2 = x * x;
  x2c = (f2v){fminf(x2[0], 36.0f), fminf(x2[1], 36.0f)};
  // -log2(e) folded into the coefficients: e = 2^(x * t) = exp(-u)
  f2v t = x2c * splat2(-1.4426950408889634f * KBNER_GELU_P2) + splat2(-1.4426950408889634f * KBNER_GELU_P1);
  t = t * x2c + splat2(-1.4426950408889634f * KBNER_GELU_P0);
  const f2v a = x * t;
  const f2v d = (f2v){__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])} + splat2(1.0f);
  sg = (f2v){__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}
static __device__ __forceinline__ f2v gelu2_logistic(f2v x) {
  f2v sg, x2c;
  gelu_logistic2(x, sg, x2c);
  return x * sg;
}
static __device__ __forceinline__ void gelu_both2_logistic(f2v x, f2v& y, f2v& dy) {
  f2v sg, x2c;
  gelu_logistic2(x, sg, x2c);
  y = x * sg;
  f2v du = x2c * splat2(5.0f * KBNER_GELU_P2) + splat2(3.0f * KBNER_GELU_P1);
  du = du * x2c + splat2(KBNER_GELU_P0);
  const f2v w = sg - sg * sg;
  dy = (x * w) * du + sg;
}
#ifdef KBNER_GELU_LOGISTIC
#define gelu2 gelu2_logistic
#define gelu_both2 gelu_both2_logistic
#endif
