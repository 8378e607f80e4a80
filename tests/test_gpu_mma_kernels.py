"""GPU: element-wise and exact parity tests of the kernels that carry the flops -- the bf16 MFMA GEMM and its epilogues
(csrc/gemm.hip, csrc/gemm256.hip), the fused self-attention (csrc/attention.hip), kbner_ln_fwd / kbner_ln_bwd
(csrc/layernorm.hip) -- and of the dropout mask, through the C ABI against the float64 references of tests/mmaref.py (which
tests/test_mmaref_cpu.py proves against torch.autograd).  tests/selftest.py reduces an output tensor to one relative L2
number; one zeroed 16 x 16 block of a 16384 x 4096 product, a dropped K step of one tile, a bias read one column off or a
query row that misses a key chunk moves that number by less than its threshold.  Here every element is compared.

Two kinds of case, as in tests/test_gpu_row_kernels.py.  EXACT: integer-valued inputs whose every float32 intermediate is an
integer (or half-integer) below 2^24 (mmaref.GEMM_EXACT, bound asserted on the CPU), one-hot / uniform attention, +-1
LayerNorm rows: the assertion is EQUALITY with the float64 reference (bf16 outputs: with its bf16 rounding, bit for bit).
REAL: Gaussian inputs against float64 under rowref.tolerance: 8 x the worst error of the same formula evaluated in float32
with the kernels' documented rounding points (mmaref docstring), floor 2 * 2^-24 * sum|terms|, plus one bf16 ulp for bf16
outputs; attention is asserted per query row with the row's own scale.  No dropout case takes its reference from
kbner_dropout_mask: the mask comes from mmaref.dropout_keep, the integer restatement of the contract in include/kbner.h.
Every output buffer has NaN guard rows behind it and, where a leading dimension allows, NaN guard columns beside it.

Every real-valued check prints kernel error, float32-evaluation error, their ratio (of which the rule allows 8) and the
largest share of its tolerance any element used (run with -s).  Worst figures per kernel of the MI355X run that accompanied
this module (196 cases, all passing, 54 s on its own): `ratio` = kernel error / float32-evaluation error; `share` = the
largest fraction of its tolerance any element used.  For bf16 outputs the ratio says nothing where the error IS the bf16
rounding of the output (share just below 1: half a bf16 ulp is 2^-8 relative at the bottom of a binade); for attention the
float32 evaluation models the bf16 probabilities, so the shares show how little of 8 x that error the kernels use.

    kernel (output)                 ratio   share      kernel (output)                 ratio   share
    gemm128 (C32)                   0.24    0.03       attention ctx                   -       0.18
    gemm128 (bf16 / out2)           -       0.994      attention ctx, dropout          -       0.18
    gemm256 (C32)                   1.03    0.13       attention dq                    -       0.29
    gemm256 (bf16 / out2)           -       0.996      attention dk                    -       0.20
    gemm256 colsum                  0.19    0.02       attention dv                    -       0.19
    gemm256 grouped x16 (C32)       1.05    0.13       attention dq / dk / dv, dropout -       0.21
    gemm256 split-K slab            0.91    0.11       attention lse                   1.35    0.17
    splitk_finish (bf16)            -       0.994      attention dbias                 1.01    0.13
    ln_fwd (mean)                   1.60    0.13       ln_bwd (dgamma)                 1.46    0.18
    ln_fwd (rstd)                   1.00    0.12       ln_bwd (dbeta)                  1.59    0.12
    ln_fwd (y, bf16)                -       0.994      ln_bwd (dbias)                  1.37    0.17
    ln_bwd (dh / dhm, bf16)         -       0.994      ln_bwd deferred (all three)     0.89    0.07

No kernel needed more than 1.6 of the factor 8.  Every exact case is bit-equal, the S = 192 / 384 / 448 instantiations and the
workgroup tiles larger than a head included; kbner_ln_fwd's variance of a +-1 row is exactly 1.  One observation, not a
defect: the forward's fused exponent leaves e = 1 + delta at a row's largest score, and with dropout the forward normalises
by the float32 sum of e while P.V takes bf16(e), so in the one-hot case O = 2 V / (1 + 3e-6) before its bf16 rounding; with
ctx_lo the residual byte hands that to D and dQ / dK are 3.9e-4 / 1.4e-3 instead of 0 there.  mmaref.attn_eval32 models both
(fused exponent, residual byte), so the case stands under the same 8 x rule; everywhere else dQ = dK = 0 exactly.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import mmaref
import rowref
from mmaref import D, NN, NT, TN, bf16_rne

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
WORST = {}
EPI_BIAS, EPI_GELU, EPI_ADD, EPI_DGELU, EPI_ATOMIC32, EPI_RMW32, EPI_COLSUM, EPI_DROP = 1, 2, 4, 8, 16, 32, 64, 128
EPI_STORE32, EPI_COLSUM_WS, EPI_GELU_FWD = 256, 512, 1024
C32_EPIS = EPI_ATOMIC32 | EPI_RMW32 | EPI_STORE32


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    yield _ops
    print("\n[mmak] worst per kernel (error ratio kernel / float32 evaluation, largest share of the tolerance used):")
    for k in sorted(WORST):
        print("[mmak]   %-34s ratio %8.3f   share %6.3f" % (k, WORST[k][0], WORST[k][1]))


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def dev_bf16(a):
    """float64 array of bf16 values -> device bf16 tensor"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF16).to(DEV)


def dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def round_bf16(a):
    return bf16_rne(a)


def parent(a, dtype, pad_cols=0, extra_rows=0):
    """device buffer [rows + extra_rows, cols + pad_cols] of NaN holding `a` in its top-left corner: the kernel is given the
    buffer's width as the leading dimension, so the NaN columns / rows are guards (an input that is read there poisons the
    output, an output that is written there shows)"""
    a = np.asarray(a)
    full = torch.full((a.shape[0] + extra_rows, a.shape[1] + pad_cols), NAN, dtype=dtype, device=DEV)
    full[:a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)
    return full


def out_parent(M, N, dtype, pad_cols=0, extra_rows=3):
    return torch.full((M + extra_rows, N + pad_cols), NAN, dtype=dtype, device=DEV)


def guards_untouched(full, M, N):
    g = torch.isnan(full)
    return bool(g[M:].all()) and bool(g[:M, N:].all())


def check_exact(got, ref64, what=""):
    """integer-valued case: the float32 output EQUALS the float64 reference"""
    ref64 = np.asarray(ref64, np.float64)
    ref = ref64.astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), ref64), "the reference is not a float32 value"
    g = got.detach().float().cpu().numpy().reshape(ref.shape)
    bad = np.argwhere(g != ref)
    assert bad.shape[0] == 0, "%s: %d elements differ, first at %s: got %r expected %r" % (
        what, bad.shape[0], tuple(bad[0]), g[tuple(bad[0])], ref[tuple(bad[0])])


def check_exact_bf16(got, ref64, what=""):
    """the bf16 output EQUALS bf16_rne(reference) bit for bit (the reference is a float32 value)"""
    ref64 = np.asarray(ref64, np.float64)
    assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64), "the reference is not a float32 value"
    assert got.dtype == BF16
    check_exact(got, round_bf16(ref64), what)


def check_real(kernel, case, got, ref64, err32, sum_abs, bf16_out=False, got_is_numpy=False):
    """rowref.tolerance with the float32 evaluation's worst error given (it may come from a sample of rows / heads)"""
    ref64 = np.asarray(ref64, np.float64)
    g = (np.asarray(got, np.float64) if got_is_numpy else host(got)).reshape(ref64.shape)
    assert np.isfinite(g).all(), "%s %s: non-finite output" % (kernel, case)
    tol = np.maximum(8.0 * err32, 2.0 * rowref.F32_EPS * np.asarray(sum_abs, np.float64))
    if bf16_out:
        tol = tol + rowref.BF16_ULP * np.abs(ref64)
    diff = np.abs(g - ref64)
    kerr = float(diff.max()) if diff.size else 0.0
    share = float((diff / np.maximum(tol, 1e-300)).max()) if diff.size else 0.0
    ratio = kerr / err32 if err32 > 0 else (0.0 if kerr == 0 else float("inf"))
    print("[mmak] %s %s: kernel_err %.3e  f32_eval_err %.3e  ratio %.3f  tolerance_share %.3f%s"
          % (kernel, case, kerr, err32, ratio, share, "  (bf16 output)" if bf16_out else ""))
    w = WORST.setdefault(kernel, [0.0, 0.0])
    if not bf16_out and math.isfinite(ratio):
        w[0] = max(w[0], ratio)
    w[1] = max(w[1], share)
    if share > 1.0:
        i = np.unravel_index(int(np.argmax(diff / np.maximum(tol, 1e-300))), diff.shape)
        raise AssertionError("%s %s: element %s got %r expected %r, tolerance share %.3f" % (kernel, case, i, g[i], ref64[i], share))


# ====================================================================== dropout mask: the documented hash, bit for bit
@pytest.mark.parametrize("Z,M,N,seed,thresh", [
    (1, 256, 384, 12345, mmaref.dropout_thresh(0.1)), (3, 512, 512, 12345, mmaref.dropout_thresh(0.1)),
    (4, 64, 192, 0x80000001, mmaref.dropout_thresh(0.5)), (2, 300, 8, 0xFFFFFFF0, mmaref.dropout_thresh(0.1)),   # top bit set, wrap
    (5, 1, 1024, 7, mmaref.dropout_thresh(0.5)), (1, 1024, 1024, 0xDEADBEEF, 1), (2, 17, 40, 0, mmaref.dropout_thresh(0.75))])
def test_dropout_mask_is_the_documented_hash(ops, Z, M, N, seed, thresh):
    full = torch.full((Z * M + 3, N), NAN, dtype=F32, device=DEV)
    from kbner import lib as L
    L.call("kbner_dropout_mask", L.ptr(full), Z, M, N, seed, thresh, L.stream_ptr())
    torch.cuda.synchronize()
    ref = mmaref.dropout_mult(Z, M, N, seed, thresh).reshape(Z * M, N)
    assert np.array_equal(full[:Z * M].cpu().numpy().view(np.int32), ref.view(np.int32))
    assert bool(torch.isnan(full[Z * M:]).all())


# ====================================================================== GEMM
def _gemm_inputs(rng, kind, layout, M, N, K, epi, drop_p, seed, colsum=False):
    """-> dict of float64 host arrays in MEMORY layout (bf16 operands already rounded) + the dropout multiplier"""
    if kind == "exact":
        g = mmaref.GEMM_COLSUM_EXACT if colsum else mmaref.GEMM_EXACT
        assert K <= g["K"] and (not colsum or M <= g["M"])
        a, b = mmaref.ints(rng, g["ab"], (M, K)), mmaref.ints(rng, g["ab"], (N, K))
        bias = mmaref.ints(rng, mmaref.GEMM_EXACT["bias"], N)
        add = mmaref.ints(rng, mmaref.GEMM_EXACT["addend"], (M, N))
        aux = mmaref.ints(rng, g["aux"], (M, N))
    else:
        a, b = round_bf16(rng.standard_normal((M, K)) * 0.5), round_bf16(rng.standard_normal((N, K)) * 0.5)
        bias = rng.standard_normal(N).astype(np.float32).astype(np.float64)
        add, aux = round_bf16(rng.standard_normal((M, N))), round_bf16(rng.standard_normal((M, N)))
    d = {"A": np.ascontiguousarray(a.T) if layout == TN else a, "B": b if layout == NT else np.ascontiguousarray(b.T),
         "bias": bias if epi & EPI_BIAS else None, "addend": add if epi & EPI_ADD else None, "aux": aux if epi & EPI_DGELU else None,
         "mask": None, "drop": (0, 0)}
    if drop_p:
        th = mmaref.dropout_thresh(drop_p)
        d["drop"] = (seed, th)
        d["mask"] = mmaref.dropout_mult(1, M, N, seed, th)[0]
    return d


def _run_gemm(ops, route, kind, layout, M, N, K, epi, alpha=1.0, pad=0, drop_p=0.0, splitk=1, tag=""):
    """one GEMM through `route` ("g128": kbner_gemm_bf16; "grp": kbner_gemm_bf16_grouped, static walk; "dyn":
    kbner_gemm_bf16_grouped_dyn), every operand in a parent `pad` columns wider than the matrix, checked against mmaref"""
    from kbner import lib as L
    seed = 1000003 * layout + M + 7 * N + 13 * K + epi
    rng = np.random.default_rng(seed)
    colsum = bool(epi & EPI_COLSUM)
    d = _gemm_inputs(rng, kind, layout, M, N, K, epi, drop_p, 0x80000000 | seed, colsum)
    Ad, Bd = parent(d["A"], BF16, pad), parent(d["B"], BF16, pad)
    kw = {}
    if d["bias"] is not None:
        kw["bias"] = dev_f32(d["bias"])
    if d["addend"] is not None:
        kw["addend"] = parent(d["addend"], BF16, pad)
    if d["aux"] is not None:
        kw["aux"] = parent(d["aux"], BF16, pad)
    out2 = None
    if epi & EPI_GELU:
        out2 = kw["out2"] = out_parent(M, N, BF16, pad)
    pre32 = None
    if epi & C32_EPIS:
        pre32 = mmaref.ints(rng, mmaref.GEMM_EXACT["preload"], (M, N)) if kind == "exact" else rng.standard_normal((M, N)).astype(np.float32).astype(np.float64)
        C = kw["C32"] = parent(pre32, F32, pad and 4, 3)
    else:
        C = kw["C"] = out_parent(M, N, BF16, pad)
    cs = cs0 = None
    if colsum:
        if epi & EPI_COLSUM_WS:
            cs = torch.full((2 * (M // ops.gemm_tile_rows(layout, M, N)) + 1, N), NAN, dtype=F32, device=DEV)
        else:
            cs0 = mmaref.ints(rng, 8, N)
            cs = torch.cat([dev_f32(cs0), torch.full((8,), NAN, device=DEV)])
        kw["colsum"] = cs
    if route == "g128":
        assert not colsum
        ops.gemm(layout, Ad, Bd, M, N, K, epi=epi, splitk=splitk, alpha=alpha, lda=Ad.shape[1], ldb=Bd.shape[1], drop=d["drop"], **kw)
    else:
        p = ops.make_problem(Ad, Bd, M, N, K, epi=epi, alpha=alpha, drop=d["drop"], **kw)
        if route == "grp":
            arr = (L.GemmProblem * 1)(p)
            L.call("kbner_gemm_bf16_grouped", layout, 1, ctypes.cast(arr, ctypes.c_void_p), L.stream_ptr())
        else:
            sched = torch.zeros(8, dtype=I32, device=DEV)
            arr = (L.GemmProblem * 1)(p)
            L.call("kbner_gemm_bf16_grouped_dyn", layout, 1, ctypes.cast(arr, ctypes.c_void_p), L.ptr(sched), L.stream_ptr())
    torch.cuda.synchronize()
    case = "%s %s L%d %dx%dx%d epi=%d alpha=%g pad=%d p=%g sk=%d %s" % (route, kind, layout, M, N, K, epi, alpha, pad, drop_p, splitk, tag)
    assert guards_untouched(C, M, N), case
    got = C[:M, :N]
    if epi & C32_EPIS:          # alpha * acc only (the 32-bit outputs bypass the rest of the epilogue), onto the preload
        fl = 0
        base = 0.0 if epi & EPI_STORE32 else pre32
    else:
        fl = epi & (EPI_BIAS | EPI_GELU | EPI_ADD | EPI_DGELU | EPI_GELU_FWD)
        base = 0.0
    args = (layout, d["A"], d["B"], fl, d["bias"], d["addend"], d["aux"], alpha, None if epi & C32_EPIS else d["mask"])
    ref, dref = mmaref.gemm_ref(*args)
    ref = ref + base
    kname = "gemm128" if route == "g128" else "gemm256"
    if kind == "exact":
        if epi & C32_EPIS:
            check_exact(got, ref, case)
        else:
            check_exact_bf16(got, ref, case)
        if colsum:
            want = host(got).sum(0)                                  # EQUAL the column sums of the bf16 output
            assert np.array_equal(want, ref.sum(0))                  # (which the generator keeps bf16-exact)
            if epi & EPI_COLSUM_WS:
                rows = cs.shape[0] - 1
                assert bool(torch.isnan(cs[rows:]).all()) and bool(torch.isfinite(cs[:rows]).all())
                check_exact(cs[:rows].sum(0), want, case + " colsum_ws")
            else:
                assert bool(torch.isnan(cs[N:]).all())
                check_exact(cs[:N], want + cs0, case + " colsum")
        return
    rows = None
    if M * N * K > 2 ** 27:       # a large output: the float32 evaluation runs on a sample of rows (mmaref.gemm_eval32)
        rows = np.unique(np.concatenate([np.linspace(0, M - 1, 96).astype(np.int64), np.arange(M - 16, M)]))
    ev, dev_ = mmaref.gemm_eval32(*args, rows=rows)
    sl = slice(None) if rows is None else rows
    ev = ev.astype(np.float64) + (base if np.isscalar(base) else base[sl])
    sa = mmaref.gemm_sum_abs(*args) + (0.0 if np.isscalar(base) else np.abs(base))
    if fl & (EPI_GELU | EPI_GELU_FWD):
        sa = sa * 1.2             # |gelu'| <= 1.13, |gelu''| <= 1: an error of the pre-activation passes through at most like that
    check_real(kname + (" (C32)" if epi & C32_EPIS else " (bf16)"), case, got, ref, float(np.abs(ev - ref[sl]).max()), sa,
               bf16_out=not (epi & C32_EPIS))
    if out2 is not None:
        assert guards_untouched(out2, M, N), case
        check_real(kname + " (out2 gelu', bf16)", case, out2[:M, :N], dref, float(np.abs(dev_.astype(np.float64) - dref[sl]).max()), sa, bf16_out=True)
    if colsum and not (epi & EPI_COLSUM_WS):
        want = ref.sum(0) + cs0                                      # the kernel sums the float32 values it rounds for the store
        check_real("gemm256 colsum", case, cs[:N], want, float(np.abs(rowref.seq_sum32(np.float32(ev), 0) + np.float32(cs0) - want).max()),
                   sa.sum(0) + np.abs(cs0))


# (route, layout, M, N, K, epi, alpha, pad, dropout p, split-K).  Which launcher route each one reaches, and why:
GEMM_CASES = [
    # kbner_gemm_bf16, the 128 x 128 kernel: one tile; a 128-multiple that is not a 256-multiple; all layouts; ld > width
    ("g128", NT, 128, 128, 64, 0, 1.0, 0, 0.0, 1), ("g128", NT, 384, 128, 192, EPI_BIAS | EPI_ADD, 0.5, 8, 0.0, 1),
    ("g128", NN, 128, 384, 320, EPI_DGELU, -2.0, 24, 0.0, 1), ("g128", NN, 256, 256, 128, EPI_ADD, 1.0, 8, 0.0, 1),
    ("g128", NT, 256, 384, 4096, EPI_BIAS | EPI_ADD | EPI_DROP, -2.0, 8, 0.75, 1), ("g128", NT, 128, 256, 64, EPI_BIAS | EPI_DROP, 1.0, 0, 0.5, 1),
    ("g128", TN, 128, 128, 64, EPI_ATOMIC32, 1.0, 0, 0.0, 1), ("g128", TN, 256, 384, 512, EPI_ATOMIC32, 0.5, 8, 0.0, 4),
    ("g128", TN, 384, 256, 4096, EPI_ATOMIC32, -2.0, 8, 0.0, 8), ("g128", NT, 128, 128, 128, EPI_BIAS, 0.5, 16, 0.0, 1),
    # kbner_gemm_bf16_grouped, one problem: NT / NN with few tiles -> 128-row tiles (2 * tiles <= CUs; kbner_gemm_tile_rows
    # is printed), TN always 256-row tiles; every K of the ring phases (64, 128, 192, 320) and the longest exact K
    ("grp", NT, 256, 256, 64, 0, 1.0, 0, 0.0, 1), ("grp", NT, 512, 768, 320, EPI_BIAS | EPI_ADD, 0.5, 8, 0.0, 1),
    ("grp", NT, 512, 256, 128, EPI_BIAS, -2.0, 24, 0.0, 1), ("grp", NN, 256, 256, 64, 0, 1.0, 8, 0.0, 1),
    ("grp", NN, 512, 768, 320, EPI_DGELU, 0.5, 8, 0.0, 1), ("grp", NN, 768, 256, 192, EPI_ADD, 1.0, 8, 0.0, 1),
    ("grp", TN, 256, 256, 64, EPI_RMW32, 1.0, 0, 0.0, 1), ("grp", TN, 512, 768, 4096, EPI_RMW32, -2.0, 8, 0.0, 1),
    ("grp", TN, 256, 512, 320, EPI_ATOMIC32, 0.5, 8, 0.0, 1), ("grp", TN, 512, 256, 192, EPI_STORE32, 1.0, 8, 0.0, 1),
    ("grp", NT, 768, 512, 4096, EPI_BIAS | EPI_ADD | EPI_DROP, 1.0, 8, 0.5, 1), ("grp", NT, 256, 512, 192, EPI_BIAS | EPI_ADD | EPI_DROP, 0.5, 0, 0.75, 1),
    ("grp", NN, 768, 512, 128, EPI_DGELU | EPI_COLSUM, 1.0, 8, 0.0, 1), ("grp", NN, 768, 512, 64, EPI_DGELU | EPI_COLSUM | EPI_COLSUM_WS, 1.0, 0, 0.0, 1),
    # more tiles than CUs (320 tiles; asserted in test_case_lists_reach_the_routes_their_comments_name): 256-row tiles, persistent
    # walk, several tiles per workgroup
    ("grp", NT, 4096, 5120, 128, EPI_BIAS | EPI_ADD, 0.5, 8, 0.0, 1), ("grp", NN, 5120, 4096, 64, EPI_DGELU, -2.0, 8, 0.0, 1),
    ("grp", TN, 4096, 5120, 192, EPI_RMW32, 1.0, 8, 0.0, 1), ("grp", NN, 8192, 4096, 64, EPI_DGELU | EPI_COLSUM | EPI_COLSUM_WS, 1.0, 8, 0.0, 1),
    ("grp", NT, 4096, 5120, 320, EPI_BIAS | EPI_ADD | EPI_DROP, 1.0, 8, 0.5, 1),
    # kbner_gemm_bf16_grouped_dyn with a zeroed sched: the tile draw of the two-stage loop (K < 1024), one workgroup per
    # tile on the ring kernel (K >= 1024)
    ("dyn", NT, 512, 768, 320, EPI_BIAS | EPI_ADD, 0.5, 8, 0.0, 1), ("dyn", TN, 4096, 5120, 128, EPI_RMW32, 1.0, 8, 0.0, 1),
    ("dyn", NN, 768, 512, 1024, EPI_DGELU, -2.0, 8, 0.0, 1), ("dyn", NT, 4096, 2560, 64, EPI_BIAS, 1.0, 0, 0.0, 1),
]


@pytest.mark.parametrize("route,layout,M,N,K,epi,alpha,pad,drop_p,sk,variant",
                         [c + (v,) for v in (1, 0) for c in GEMM_CASES if v == 1 or c[0] != "g128"])
def test_gemm_exact(ops, route, layout, M, N, K, epi, alpha, pad, drop_p, sk, variant):
    """variant 1: the ring kernels (default); 0: the two-stage loop.  The 128 x 128 kernel has no variants: it runs once."""
    prev = ops.gemm_variant(variant)
    try:
        tag = "v%d" % variant + (" tile_rows=%d" % ops.gemm_tile_rows(layout, M, N) if route == "grp" else "")
        _run_gemm(ops, route, "exact", layout, M, N, K, epi, alpha, pad, drop_p, sk, tag)
    finally:
        ops.gemm_variant(prev)


# REAL-VALUED: one shape per route above with the epilogues that are not integer-valued (GELU, GELU', GELU_FWD) added, and
# the two largest shapes of tests/test_gpu_kernels.py test_gemm
GEMM_REAL_CASES = [
    ("g128", NT, 384, 128, 192, EPI_BIAS | EPI_GELU, 1.0, 8, 0.0, 1), ("g128", NT, 128, 384, 64, EPI_BIAS | EPI_GELU_FWD, 1.0, 8, 0.0, 1),
    ("g128", NN, 128, 384, 320, EPI_DGELU, 0.5, 24, 0.0, 1), ("g128", TN, 256, 384, 512, EPI_ATOMIC32, 1.0, 8, 0.0, 4),
    ("g128", NT, 256, 384, 1024, EPI_BIAS | EPI_ADD | EPI_DROP, 1.0, 8, 0.1, 1),
    ("grp", NT, 512, 256, 128, EPI_BIAS | EPI_GELU, 1.0, 8, 0.0, 1), ("grp", NT, 512, 256, 128, EPI_BIAS | EPI_GELU_FWD, 1.0, 8, 0.0, 1),
    ("grp", NN, 512, 768, 320, EPI_DGELU, 1.0, 8, 0.0, 1), ("grp", TN, 512, 768, 1024, EPI_RMW32, 1.0, 8, 0.0, 1),
    ("grp", TN, 512, 256, 192, EPI_STORE32, 0.5, 8, 0.0, 1), ("grp", NT, 768, 512, 1024, EPI_BIAS | EPI_ADD | EPI_DROP, 1.0, 8, 0.1, 1),
    ("grp", NN, 768, 512, 256, EPI_DGELU | EPI_COLSUM, 1.0, 8, 0.0, 1),
    ("grp", NT, 4096, 5120, 128, EPI_BIAS | EPI_GELU, 1.0, 8, 0.0, 1), ("grp", NT, 4096, 5120, 128, EPI_BIAS | EPI_GELU_FWD, 1.0, 0, 0.0, 1),
    ("grp", NN, 4096, 5120, 128, EPI_DGELU, 1.0, 8, 0.0, 1), ("grp", TN, 5120, 4096, 128, EPI_RMW32, 1.0, 8, 0.0, 1),
    ("dyn", NT, 512, 768, 320, EPI_BIAS | EPI_GELU, 1.0, 8, 0.0, 1), ("dyn", NN, 768, 512, 1024, EPI_DGELU, 1.0, 8, 0.0, 1),
    ("grp", NT, 16384, 4096, 64, 0, 1.0, 0, 0.0, 1), ("grp", NT, 8192, 2560, 192, EPI_BIAS | EPI_ADD, 1.0, 0, 0.0, 1),
]


@pytest.mark.parametrize("route,layout,M,N,K,epi,alpha,pad,drop_p,sk", GEMM_REAL_CASES)
def test_gemm_real(ops, route, layout, M, N, K, epi, alpha, pad, drop_p, sk):
    _run_gemm(ops, route, "real", layout, M, N, K, epi, alpha, pad, drop_p, sk)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("route,layout,M,N,K,epi,alpha,pad,drop_p,sk", [c for c in GEMM_REAL_CASES if c[0] == "grp" and c[2] * c[3] < 2 ** 26])
def test_gemm_real_two_stage_loop(ops, route, layout, M, N, K, epi, alpha, pad, drop_p, sk):
    """the grouped real-valued cases again on kbner_gemm_set_variant(0), the two-stage loop (the default is the ring loop)"""
    prev = ops.gemm_variant(0)
    try:
        _run_gemm(ops, route, "real", layout, M, N, K, epi, alpha, pad, drop_p, sk, "v0")
    finally:
        ops.gemm_variant(prev)
    torch.cuda.empty_cache()


def test_case_lists_reach_the_routes_their_comments_name(ops):
    """the launchers choose by the device's CU count: on a part where a case list no longer reaches a route its comment names
    (128-row grouped tiles, the persistent walk, the attention tile heights) this fails instead of silently testing less"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for cases in (GEMM_CASES, GEMM_REAL_CASES):
        grp = [c for c in cases if c[0] == "grp"]
        rows = {(c[1], ops.gemm_tile_rows(c[1], c[2], c[3])) for c in grp}
        assert {(NT, 128), (NN, 128), (NT, 256), (NN, 256), (TN, 256)} <= rows and (TN, 128) not in rows, rows
        for c in grp:                                   # kbner_gemm_tile_rows itself: 128 iff NT / NN and 2 * tiles <= CUs
            tiles = (c[2] // 256) * (c[3] // 256)
            assert ops.gemm_tile_rows(c[1], c[2], c[3]) == (128 if c[1] != TN and 2 * tiles <= ncu else 256), c
        for layout in (NT, NN, TN):                     # persistent walk: more 256-row tiles than CUs
            assert any(c[1] == layout and (c[2] // 256) * (c[3] // 256) > ncu for c in grp), layout
        assert any(c[0] == "dyn" and c[4] >= 1024 for c in cases) and any(c[0] == "dyn" and c[4] < 1024 for c in cases)
    for cases in (mmaref.ONEHOT_CASES, ATTN_REAL_CASES):
        routes = {(mmaref.pick_rpw(B, S, A), mmaref.pick_rpw(B, S, A) == S and B * A >= 2 * ncu) for B, S, A, *_ in cases}
        assert {(128, False), (256, True), (512, True), (256, False)} <= routes, routes
        assert any(mmaref.pick_rpw(B, S, A) == 512 and S < 512 for B, S, A, *_ in cases)      # a tile larger than the head
        assert any(mmaref.pick_rpw(B, S, A) == 256 and S < 256 for B, S, A, *_ in cases)
        assert any(p and mmaref.pick_rpw(B, S, A) >= 256 for B, S, A, _r, _s, p in cases)     # dropout on the 32-row backward kernels


def test_gemm_exact_long_k_sync_variants(ops):
    """kbner_gemm_set_variant 3 and 7 (XCD meetings of the ring kernel) on a K >= 16384 TN launch with two tiles per CU: A, B of
    {-1, 0, 1} keep |acc| <= 16384, so the result must EQUAL the reference in every variant"""
    K, M, N = 16384, 4096, 8192                     # 16 x 32 = 512 tiles
    rng = np.random.default_rng(5)
    # A[k, :] = s[k] * x_(k mod 2): two interleaved rank-one halves, so the float64 reference is two outer products instead of
    # a 1.1-TFLOP product on the host; B is unstructured.  A dropped or doubled K step, row or column still changes C.
    s_, x_ = rng.integers(-1, 2, size=K).astype(np.float64), rng.integers(-1, 2, size=(2, M)).astype(np.float64)
    a = torch.from_numpy((s_[:, None] * x_[np.arange(K) % 2]).astype(np.float32))
    bn = rng.integers(-1, 2, size=(K, N)).astype(np.float32)
    b = torch.from_numpy(bn)
    ref = 3.0 + sum(np.outer(x_[j], (s_[j::2, None] * bn[j::2].astype(np.float64)).sum(0)) for j in (0, 1))
    ad, bd = a.to(BF16).to(DEV), b.to(BF16).to(DEV)
    prev = ops.gemm_variant()
    try:
        for v in (0, 1, 3, 7):
            ops.gemm_variant(v)
            c = torch.full((M + 2, N), NAN, dtype=F32, device=DEV)
            c[:M] = 3.0
            ops.gemm_grouped(TN, [ops.make_problem(ad, bd, M, N, K, C32=c, epi=EPI_RMW32)])
            torch.cuda.synchronize()
            assert bool(torch.isnan(c[M:]).all())
            check_exact(c[:M], ref, "variant %d" % v)
    finally:
        ops.gemm_variant(prev)


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_gemm_grouped_16_problems(ops, kind):
    """one grouped NT launch of 16 problems of different shapes, K, alpha, leading dimensions and epilogues"""
    rng = np.random.default_rng(16)
    epis = [0, EPI_BIAS, EPI_BIAS | EPI_ADD, EPI_ADD, EPI_BIAS | EPI_ADD | EPI_DROP, EPI_STORE32, EPI_RMW32, EPI_ATOMIC32]
    if kind == "real":
        epis += [EPI_BIAS | EPI_GELU, EPI_BIAS | EPI_GELU_FWD]
    probs, keep = [], []
    for i in range(16):
        M, N, K = (256, 512, 768)[i % 3], (256, 512)[(i // 3) % 2], (64, 128, 192, 320)[i % 4]
        epi, alpha, pad = epis[i % len(epis)], (1.0, 0.5, -2.0)[i % 3], (0, 8, 24)[i % 3]
        d = _gemm_inputs(rng, kind, NT, M, N, K, epi, (0.5 if kind == "exact" else 0.1) if epi & EPI_DROP else 0.0, 0x90000000 + i)
        kw = {}
        if d["bias"] is not None:
            kw["bias"] = dev_f32(d["bias"])
        if d["addend"] is not None:
            kw["addend"] = parent(d["addend"], BF16, pad)
        out2 = None
        if epi & EPI_GELU:
            out2 = kw["out2"] = out_parent(M, N, BF16, pad)
        pre32 = None
        if epi & C32_EPIS:
            pre32 = mmaref.ints(rng, 8, (M, N))
            C = kw["C32"] = parent(pre32, F32, pad and 4, 3)
        else:
            C = kw["C"] = out_parent(M, N, BF16, pad)
        Ad, Bd = parent(d["A"], BF16, pad), parent(d["B"], BF16, pad)
        probs.append(ops.make_problem(Ad, Bd, M, N, K, epi=epi, alpha=alpha, drop=d["drop"], **kw))
        keep.append((d, Ad, Bd, kw, C, out2, pre32, M, N, K, epi, alpha))
    assert ops.gemm_grouped(NT, probs) is False
    torch.cuda.synchronize()
    for i, (d, _a, _b, _kw, C, out2, pre32, M, N, K, epi, alpha) in enumerate(keep):
        case = "problem %d %dx%dx%d epi=%d alpha=%g" % (i, M, N, K, epi, alpha)
        assert guards_untouched(C, M, N), case
        c32 = bool(epi & C32_EPIS)
        fl = 0 if c32 else epi & (EPI_BIAS | EPI_GELU | EPI_ADD | EPI_GELU_FWD)
        args = (NT, d["A"], d["B"], fl, d["bias"], d["addend"], None, alpha, None if c32 else d["mask"])
        ref, dref = mmaref.gemm_ref(*args)
        base = 0.0 if not c32 or epi & EPI_STORE32 else pre32
        ref = ref + base
        if kind == "exact":
            (check_exact if c32 else check_exact_bf16)(C[:M, :N], ref, case)
            continue
        ev, dev_ = mmaref.gemm_eval32(*args)
        sa = (mmaref.gemm_sum_abs(*args) + np.abs(base)) * 1.2
        check_real("gemm256 grouped x16" + (" (C32)" if c32 else " (bf16)"), case, C[:M, :N], ref, float(np.abs(ev + base - ref).max()), sa, bf16_out=not c32)
        if out2 is not None:
            assert guards_untouched(out2, M, N)
            check_real("gemm256 grouped x16 (out2, bf16)", case, out2[:M, :N], dref, float(np.abs(dev_ - dref).max()), sa, bf16_out=True)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("layout,M,N,K,splits,drop_p,pad", [(NT, 512, 256, 1024, 4, 0.0, 8), (NN, 256, 512, 512, 2, 0.0, 8),
                                                             (NT, 256, 256, 4096, 4, 0.5, 8), (NN, 512, 512, 256, 2, 0.75, 0)])
def test_gemm_splitk(ops, kind, layout, M, N, K, splits, drop_p, pad):
    """gemm_splitk: the K slices (a_off / b_off into parents that keep their leading dimensions) as STORE32 slabs of one grouped
    launch -- each slab checked on its own -- and kbner_splitk_finish's fold bf16(dropout(sum + bias) + addend)"""
    if kind == "real" and drop_p:
        drop_p = 0.1
    seed = 77 + M + K + splits
    rng = np.random.default_rng(seed)
    d = _gemm_inputs(rng, kind, layout, M, N, K, EPI_BIAS | EPI_ADD, drop_p, 0xA0000000 + seed)
    Ad, Bd = parent(d["A"], BF16, pad), parent(d["B"], BF16, pad)
    ws = torch.full((splits + 1, M, N), NAN, dtype=F32, device=DEV)
    C = out_parent(M, N, BF16, pad)
    ops.gemm_splitk(layout, Ad, Bd, M, N, K, splits, ws, C, bias=dev_f32(d["bias"]), addend=parent(d["addend"], BF16, pad), drop=d["drop"])
    torch.cuda.synchronize()
    case = "L%d %dx%dx%d splits=%d p=%g" % (layout, M, N, K, splits, drop_p)
    assert guards_untouched(C, M, N) and bool(torch.isnan(ws[splits]).all()), case
    Ks = K // splits
    args = (layout, d["A"], d["B"], EPI_BIAS | EPI_ADD, d["bias"], d["addend"], None, 1.0, d["mask"])
    ref, _ = mmaref.gemm_ref(*args)
    slabs = []
    for s in range(splits):
        As = d["A"][:, s * Ks:(s + 1) * Ks]
        Bs = d["B"][:, s * Ks:(s + 1) * Ks] if layout == NT else d["B"][s * Ks:(s + 1) * Ks]
        sref, _ = mmaref.gemm_ref(layout, As, Bs)
        if kind == "exact":
            check_exact(ws[s], sref, case + " slab %d" % s)
        else:
            ev, _ = mmaref.gemm_eval32(layout, As, Bs)
            check_real("gemm256 split-K slab", case + " slab %d" % s, ws[s], sref, float(np.abs(ev - sref).max()), mmaref.gemm_sum_abs(layout, As, Bs))
            slabs.append(ev)
    if kind == "exact":
        check_exact_bf16(C[:M, :N], ref, case + " finish")
    else:
        ev = sum(slabs[1:], slabs[0]) + np.float32(d["bias"])[None, :]
        if d["mask"] is not None:
            ev = ev * d["mask"]
        ev = ev + np.float32(d["addend"])
        check_real("splitk_finish (bf16)", case, C[:M, :N], ref, float(np.abs(ev - ref).max()), mmaref.gemm_sum_abs(*args), bf16_out=True)


# ====================================================================== attention
def _run_attention(ops, qkv64, dctx64, mb, B, S, A, residual, drop):
    """forward + backward through the C ABI, every output in a buffer with NaN guard rows -> host arrays"""
    H = A * D
    qd, dd, mbd = dev_bf16(qkv64), dev_bf16(dctx64), dev_f32(mb)
    ctx = torch.full((B * S + 3, H), NAN, dtype=BF16, device=DEV)
    lse = torch.full((B * A * S + 64,), NAN, dtype=F32, device=DEV)
    dqkv = torch.full((B * S + 3, 3 * H), NAN, dtype=BF16, device=DEV)
    dws = torch.zeros(B * A * S + 64, dtype=F32, device=DEV)
    dbias = torch.zeros(3 * H, dtype=F32, device=DEV)
    ctx_lo = torch.zeros(B * S * H, dtype=torch.uint8, device=DEV) if residual else None
    ops.attn_fwd(qd, mbd, ctx, lse, B, S, H, A, drop=drop, ctx_lo=ctx_lo)
    ops.attn_bwd(qd, ctx, dd, mbd, lse, dws, dqkv, B, S, H, A, drop=drop, dbias=dbias, ctx_lo=ctx_lo)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx[B * S:]).all()) and bool(torch.isnan(lse[B * A * S:]).all()) and bool(torch.isnan(dqkv[B * S:]).all())
    assert bool(torch.isfinite(ctx[:B * S]).all()) and bool(torch.isfinite(dqkv[:B * S]).all()) and bool(torch.isfinite(lse[:B * A * S]).all())
    g = host(dqkv[:B * S])
    return {"ctx": host(ctx[:B * S]), "lse": host(lse[:B * A * S]).reshape(B, A, S), "dq": g[:, :H], "dk": g[:, H:2 * H], "dv": g[:, 2 * H:],
            "dbias": host(dbias)}


def _route(B, S, A):
    rpw = mmaref.pick_rpw(B, S, A)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return "rpw=%d %s" % (rpw, "persistent" if rpw == S and B * A >= 2 * ncu else "grid")


@pytest.mark.parametrize("case", mmaref.ONEHOT_CASES, ids=str)
def test_attention_exact_onehot(ops, case):
    """every query selects exactly one key with probability 1 (mmaref.onehot_case): ctx[i] EQUALS V[pi(i)], lse EQUALS 504,
    dV[j] EQUALS the sum of dO over pi(i) = j, the V third of dbias likewise; dQ = dK = 0 up to the D - dP rounding.  With
    dropout 0.5 a kept probability is exactly 2 and a dropped one 0, according to mmaref.dropout_keep."""
    B, S, A, ragged, residual, p = case
    H = A * D
    qkv, dctx, mb, pi = mmaref.onehot_inputs(case)
    keep, scale, drop = None, 1.0, (0, 0)
    if p:
        drop = (99, mmaref.dropout_thresh(p))
        keep, scale = mmaref.dropout_keep(B * A, S, S, *drop).reshape(B, A, S, S), float(mmaref.dropout_scale(drop[1]))
    ctx, dv = mmaref.onehot_expected(qkv, dctx, pi, B, S, A, keep, scale)
    assert np.array_equal(bf16_rne(dv), dv) and np.array_equal(bf16_rne(ctx), ctx)        # preconditions of the equalities
    r = _run_attention(ops, qkv, dctx, mb, B, S, A, residual, drop)
    print("[mmak] attention one-hot %s: %s" % (case, _route(B, S, A)))
    bad = np.argwhere((r["ctx"] != ctx).any(1))
    assert bad.size == 0, "ctx: %d rows differ, first (batch entry, query) = %s" % (bad.shape[0], divmod(int(bad[0, 0]), S))
    assert (r["lse"] == 504.0).all(), "lse: %d entries differ from 504" % int((r["lse"] != 504.0).sum())
    bad = np.argwhere((r["dv"] != dv).any(1))
    assert bad.size == 0, "dv: %d rows differ, first (batch entry, key) = %s" % (bad.shape[0], divmod(int(bad[0, 0]), S))
    assert np.array_equal(r["dbias"][2 * H:], dv.sum(0))
    # dQ, dK, dbias(Q | K) under the rule of the real-valued cases, unchanged: the reference is 0 (dS = P (dP - D) with P one-hot
    # and dP, D the same integer sum), the tolerance 8 x the error of the float32 evaluation with the kernels' rounding points,
    # floor 2 * 2^-24 * sum|terms| with sum|terms| of dS = |dP| + |D| <= 2 * 64 * |V| * |dO| / (1-p), times |k| / 8 / (1-p) (dK:
    # times the queries that select the key).  The evaluation is exactly 0 except with dropout AND the residual: the fused forward
    # exponent leaves e = 1 + delta at the selected key, the dropout path normalises by the float32 sum of e while P.V takes
    # bf16(e), and the residual byte hands O = 2 V / (1 + delta) to D (mmaref.attn_eval32).
    lst = mmaref.n_real_list(S)
    entries = list(range(min(B, len(lst)))) + ([B - 1] if B > len(lst) else [])
    ev = mmaref.attn_eval32(qkv, mb, B, S, A, dctx, keep=keep, thresh=drop[1], entries=entries, residual=residual)
    e32_q, e32_k = float(np.abs(ev["dq"]).max()), float(np.abs(ev["dk"]).max())
    e32_b = max(float(np.abs(ev[n].astype(np.float64).sum((0, 2))).max()) for n in ("dq", "dk")) * B / len(entries)
    terms = 2 * 64 * mmaref.ATTN_EXACT["v"] * mmaref.ATTN_EXACT["do"] * scale
    floor = 2 * rowref.F32_EPS * terms * scale
    per_key = max(int(np.bincount(pi[b, a], minlength=S).max()) for b in range(B) for a in range(A))
    tol_q, tol_k, tol_b = max(8 * e32_q, floor), max(8 * e32_k, floor * per_key), max(8 * e32_b, floor * B * S)
    print("[mmak] attention one-hot %s: max|dq| %.3e (f32 eval %.3e, bound %.3e)  max|dk| %.3e (f32 eval %.3e, bound %.3e)"
          % (case, np.abs(r["dq"]).max(), e32_q, tol_q, np.abs(r["dk"]).max(), e32_k, tol_k))
    assert np.abs(r["dq"]).max() <= tol_q and np.abs(r["dk"]).max() <= tol_k
    assert np.abs(r["dbias"][:2 * H]).max() <= tol_b


@pytest.mark.parametrize("B,S,A,n_real,residual", [(2, 64, 2, 1, False), (3, 128, 2, 16, True), (2, 192, 1, 64, False), (2, 320, 2, 32, True),
                                                   (2, 512, 2, 512, False), (64, 256, 8, 64, False), (64, 512, 8, 256, True), (64, 384, 8, 128, False)])
def test_attention_exact_uniform(ops, B, S, A, n_real, residual):
    """Q = 0 and a power of two of real keys: every real key has probability 1 / n_real exactly, so ctx[i] EQUALS bf16(mean of
    the real V rows) for integer V, and lse is log(n_real) to one float32 ulp"""
    H = A * D
    rng = np.random.default_rng(B + S + n_real)
    qkv = np.zeros((B * S, 3 * H))
    qkv[:, H:] = mmaref.ints(rng, 4, (B * S, 2 * H))
    mb = np.zeros((B, S), np.float32)
    mb[:, n_real:] = -10000.0
    r = _run_attention(ops, qkv, mmaref.ints(rng, 1, (B * S, H)), mb, B, S, A, residual, (0, 0))
    v = qkv[:, 2 * H:].reshape(B, S, H)
    mean = v[:, :n_real].sum(1) / n_real                       # an integer / 2^k: a float32 value
    want = np.repeat(bf16_rne(mean)[:, None, :], S, axis=1).reshape(B * S, H)
    assert np.array_equal(r["ctx"], want), _route(B, S, A)
    ref = np.float32(math.log(n_real))
    assert (np.abs(r["lse"] - float(ref)) <= float(np.spacing(ref))).all()


# (B, S, A, ragged, residual, dropout p): the S sweep on 128-row tiles (16-row kernels dq / dkv), the 256- and 512-row routes
# (32-row kernels fwd32 / dq2 / dkv2; persistent at (64, 256, 8) and (64, 512, 8), grid at (32, 512, 8); tiles larger than the
# head at S = 192 / 384), dropout 0.1 on both backward families, residual on and off
ATTN_REAL_CASES = (
    [(13, S, 2, True, (S // 64) % 2 == 0, 0.0) for S in range(64, 513, 64)]
    + [(13, 192, 2, True, False, 0.1), (13, 512, 1, True, True, 0.1), (64, 256, 8, True, True, 0.1)]
    + [(64, 256, 8, True, False, 0.0), (64, 512, 8, True, True, 0.0), (32, 512, 8, True, False, 0.0), (64, 192, 8, True, True, 0.0),
       (64, 384, 8, True, False, 0.0)]
)


@pytest.mark.parametrize("case", ATTN_REAL_CASES, ids=str)
def test_attention_real(ops, case):
    """Gaussian qkv, asserted PER QUERY ROW (and head): a row's error, relative to the row's own largest reference value, is at
    most 8 x the worst such error of the float32 evaluation with the kernels' rounding points (evaluated on a sample of batch
    entries that covers every n_real), plus one bf16 ulp per element; lse per element"""
    B, S, A, ragged, residual, p = case
    H = A * D
    rng = np.random.default_rng(B * 1009 + S + A + int(p * 100))
    qkv, dctx = round_bf16(rng.standard_normal((B * S, 3 * H))), round_bf16(rng.standard_normal((B * S, H)))
    mb = np.zeros((B, S), np.float32)
    lst = mmaref.n_real_list(S)
    if ragged:
        for b in range(B):
            mb[b, lst[b % len(lst)]:] = -10000.0
    keep, pmask, drop = None, None, (0, 0)
    if p:
        drop = (424242, mmaref.dropout_thresh(p))
        keep = mmaref.dropout_keep(B * A, S, S, *drop).reshape(B, A, S, S)
        pmask = keep.astype(np.float32) * mmaref.dropout_scale(drop[1])
    ref = mmaref.attn_ref(qkv, mb, B, S, A, dctx, pmask)
    entries = list(range(min(B, len(lst)))) + ([B - 1] if B > len(lst) else [])
    ev = mmaref.attn_eval32(qkv, mb, B, S, A, dctx, keep=keep, thresh=drop[1], entries=entries, residual=residual)
    r = _run_attention(ops, qkv, dctx, mb, B, S, A, residual, drop)
    cs = "%s %s" % (case, _route(B, S, A))
    for name in ("ctx", "dq", "dk", "dv"):
        rh = mmaref._heads(ref[name], B, S, A)                       # [B, A, S, 64]
        scale = np.abs(rh).max(-1, keepdims=True)                    # the row's own scale
        scale[scale == 0.0] = 1.0                                    # (dK / dV rows of masked keys are exactly 0)
        e32 = float((np.abs(ev[name].astype(np.float64) - rh[entries]).max(-1, keepdims=True) / scale[entries]).max())
        check_real("attention %s (bf16)%s" % (name, " dropout" if p else ""), cs, mmaref._heads(r[name], B, S, A) / scale, rh / scale, e32,
                   1.0, bf16_out=True, got_is_numpy=True)
    e32 = float(np.abs(ev["lse"].astype(np.float64) - ref["lse"][entries]).max())
    check_real("attention lse", cs, r["lse"], ref["lse"], e32, np.abs(ref["lse"]) + 8.0, got_is_numpy=True)
    bsum = np.concatenate([ref[n].sum(0) for n in ("dq", "dk", "dv")])
    esum = np.concatenate([mmaref._rows(np.ascontiguousarray(ev[n].astype(np.float64)), len(entries), S, A).sum(0) for n in ("dq", "dk", "dv")])
    rsum = np.concatenate([ref[n].reshape(B, S, H)[entries].sum((0, 1)) for n in ("dq", "dk", "dv")])
    sabs = np.concatenate([np.abs(ref[n]).sum(0) for n in ("dq", "dk", "dv")])
    check_real("attention dbias", cs, r["dbias"], bsum, float(np.abs(esum - rsum).max()) * B / len(entries), sabs, got_is_numpy=True)


# ====================================================================== LayerNorm
def _run_ln(ops, h64, gamma, beta, eps, dy64=None, drop=(0, 0), deferred=0):
    M, H = h64.shape
    hd = parent(h64, BF16, 0, 3)[:M]
    gd, bd = dev_f32(gamma), dev_f32(beta)
    y = out_parent(M, H, BF16)
    st = torch.full((2, M + 5), NAN, dtype=F32, device=DEV)
    ops.ln_fwd(hd, gd, bd, eps, y[:M], st[0], st[1])
    torch.cuda.synchronize()
    assert guards_untouched(y, M, H) and bool(torch.isnan(st[:, M:]).all())
    out = {"y": y[:M], "mean": st[0, :M], "rstd": st[1, :M]}
    if dy64 is None:
        return out
    dyd = parent(dy64, BF16, 0, 3)[:M]
    dh, dhm = out_parent(M, H, BF16), (out_parent(M, H, BF16) if drop[1] else None)
    n = max(deferred, 1)
    acc = torch.full((n, 3, H + 8), NAN, dtype=F32, device=DEV)
    pre = np.arange(3 * H).reshape(3, H) % 5 - 2.0
    acc[:, :, :H] = dev_f32(pre)
    mean, rstd = st[0, :M].contiguous(), st[1, :M].contiguous()
    if not deferred:
        ops.ln_bwd(dyd, hd, mean, rstd, gd, dh[:M], acc[0, 0], acc[0, 1], acc[0, 2], dhm=None if dhm is None else dhm[:M], drop=drop)
    else:
        nb = ops.ln_bwd_blocks(M)
        wss = [torch.full((nb * 3 * H + 16,), NAN, dtype=F32, device=DEV) for _ in range(n)]
        for w in wss:
            ops.ln_bwd(dyd, hd, mean, rstd, gd, dh[:M], None, None, None, dhm=None if dhm is None else dhm[:M], drop=drop, defer_ws=w)
        ops.ln_colreduce_batched([(w, acc[i, 0], acc[i, 1], acc[i, 2], nb) for i, w in enumerate(wss)], H)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(w[nb * 3 * H:]).all()) for w in wss)
    torch.cuda.synchronize()
    assert guards_untouched(dh, M, H) and (dhm is None or guards_untouched(dhm, M, H)) and bool(torch.isnan(acc[:, :, H:]).all())
    out.update(dh=dh[:M], dhm=None if dhm is None else dhm[:M], acc=acc[:, :, :H], pre=pre)
    return out


@pytest.mark.parametrize("M,H", [(1, 8), (3, 64), (5, 504), (300, 512), (4, 520), (8192, 768), (3, 1016), (1, 1024), (4100, 1024)])
def test_layernorm_exact_forward(ops, M, H):
    """rows of -1 / +1 in equal numbers, integer gamma and beta, eps = 0: mean == 0, rstd == 1, y == gamma x + beta EXACTLY"""
    h, gamma, beta = mmaref.ln_exact_case(np.random.default_rng(M + H), M, H)
    r = _run_ln(ops, h, gamma, beta, 0.0)
    assert bool((r["mean"] == 0).all()), "mean"
    assert bool((r["rstd"] == 1).all()), "rstd is not exactly 1: %r" % r["rstd"][r["rstd"] != 1][:4].tolist()
    check_exact_bf16(r["y"], h * gamma + beta, "y")


# H: one 16-byte chunk per lane up to 512, two beyond; 504 / 520 / 1016 leave lanes without a chunk.  M: 1, 3, the block's row
# count (4: one row per wave) - 1 and + 1, 300 (not a multiple of 4), 8192 and 4100 (more than LN_BWD_MAXBLOCKS x 4 = 4096 rows:
# the grid is capped at 1024 blocks and a wave walks several rows).  kind: Gaussian rows; "const": rows 0 and M - 1 constant
# (rstd = 1 / sqrt(eps)); "offset": rows around 1000 (a one-pass variance E[x^2] - mean^2 loses them in float32)
LN_CASES = ([(300, H, "gauss", 0.0, 0) for H in (8, 64, 504, 512, 520, 768, 1016, 1024)]
            + [(M, H, "gauss", 0.0, 0) for M in (1, 3, 5, 8192, 4100) for H in (768, 1024)]
            + [(1, 8, "gauss", 0.0, 0), (3, 504, "gauss", 0.0, 0), (4100, 8, "gauss", 0.0, 0), (5, 520, "const", 0.0, 0), (300, 1024, "const", 0.0, 0),
               (300, 768, "offset", 0.0, 0), (5, 1024, "offset", 0.0, 0), (301, 512, "offset", 0.0, 0),
               (300, 768, "gauss", 0.1, 0), (4100, 1024, "gauss", 0.1, 0), (5, 504, "gauss", 0.5, 0),
               (37, 768, "gauss", 0.0, 1), (300, 1024, "gauss", 0.1, 1), (37, 768, "gauss", 0.0, 64), (4100, 512, "gauss", 0.0, 1)])


@pytest.mark.parametrize("M,H,kind,drop_p,deferred", LN_CASES)
def test_layernorm_real(ops, M, H, kind, drop_p, deferred):
    rng = np.random.default_rng(M * 31 + H + deferred)
    eps = 1e-5
    h = rng.standard_normal((M, H)) * 2 + 0.3
    if kind == "offset":
        h = 1000.0 + 8.0 * rng.standard_normal((M, H))          # (bf16 spacing at 1000 is 4: the spread survives the rounding)
    h = round_bf16(h)
    if kind == "const":
        h[0] = h[0, 0]
        h[M - 1] = -3.25
    dy = round_bf16(rng.standard_normal((M, H)))
    gamma = (rng.standard_normal(H) * 0.2 + 1).astype(np.float32).astype(np.float64)
    beta = (rng.standard_normal(H) * 0.1).astype(np.float32).astype(np.float64)
    drop, mult = (0, 0), None
    if drop_p:
        drop = (0x80000063, mmaref.dropout_thresh(drop_p))
        mult = mmaref.dropout_mult(1, M, H, *drop)[0]
    ref = mmaref.ln_ref(h, gamma, beta, eps, dy, mult)
    ev = mmaref.ln_eval32(h, gamma, beta, eps, dy, mult)
    r = _run_ln(ops, h, gamma, beta, eps, dy, drop, deferred)
    cs = "M=%d H=%d %s p=%g deferred=%d" % (M, H, kind, drop_p, deferred)
    e = lambda k: float(np.abs(ev[k].astype(np.float64) - ref[k]).max())  # noqa: E731
    if kind == "const":
        assert abs(float(r["rstd"][0]) - 1 / math.sqrt(eps)) <= 2 * float(np.spacing(np.float32(1 / math.sqrt(eps))))
    xh = (h - ref["mean"][:, None]) * ref["rstd"][:, None]
    check_real("ln_fwd (mean)", cs, r["mean"], ref["mean"], e("mean"), np.abs(h).mean(1))
    check_real("ln_fwd (rstd)", cs, r["rstd"], ref["rstd"], e("rstd"), ref["rstd"])
    check_real("ln_fwd (y, bf16)", cs, r["y"], ref["y"], e("y"), (np.abs(h) + np.abs(ref["mean"])[:, None]) * ref["rstd"][:, None] * np.abs(gamma) + np.abs(beta), bf16_out=True)
    # (the kernel's backward pass starts from the float32 mean / rstd its forward stored, both checked above; the references
    # recompute their own statistics from h)
    g = np.abs(dy * gamma)
    sa_dh = ref["rstd"][:, None] * (g + g.mean(1)[:, None] + np.abs(xh) * (g * np.abs(xh)).mean(1)[:, None])
    check_real("ln_bwd (dh, bf16)", cs, r["dh"], ref["dh"], e("dh"), sa_dh, bf16_out=True)
    if drop_p:
        check_real("ln_bwd (dhm, bf16)", cs, r["dhm"], ref["dhm"], e("dhm"), sa_dh * mult, bf16_out=True)
    for i in range(r["acc"].shape[0]):
        for j, (k, sa) in enumerate((("dgamma", np.abs(dy * xh).sum(0)), ("dbeta", np.abs(dy).sum(0)),
                                     ("dbias", (sa_dh * (1.0 if mult is None else mult)).sum(0)))):
            check_real("ln_bwd (%s)%s" % (k, " deferred" if deferred else ""), cs, r["acc"][i, j], ref[k] + r["pre"][j], e(k), sa + np.abs(r["pre"][j]))
