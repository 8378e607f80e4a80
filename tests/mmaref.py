"""TEST INFRASTRUCTURE: plain float64 references of the three kernels that carry the flops -- the bf16 MFMA GEMM with its
epilogues (csrc/gemm.hip, csrc/gemm256.hip), the fused self-attention (csrc/attention.hip) and the LayerNorm half of
csrc/layernorm.hip -- and of the counter-based dropout mask, all written from the formulas in include/kbner.h (numpy; torch
on the CPU only for erf and for the bf16 rounding, as tests/rowref.py does; no kernel structure, no import of kbner).

tests/test_mmaref_cpu.py proves these functions against torch.autograd (float64) on the CPU;
tests/test_gpu_mma_kernels.py compares the HIP kernels with them.

Also here, because both test modules need them: a float32 evaluation of every real-valued formula (it feeds
rowref.tolerance: 8 x its worst error, floor 2 * 2^-24 * sum|terms|, + one bf16 ulp for bf16 outputs) and the input
generators of the EXACT cases with the magnitude bounds they guarantee.

Where the float32 evaluations round, and the kernel lines they mirror (the evaluation models the DOCUMENTED precision):
  GEMM       products of bf16 operands accumulated over K in float32 (MFMA accumulators); the whole epilogue in float32 on the
             float32 pre-activation (gemm.hip / gemm256.hip epilogue: `acc * alpha`, `+ bias`, dropout, `+ addend`, `* aux`,
             gelu_both2 "evaluated at the fp32 pre-activation"); one bf16 rounding at the store (pack2bf).
  attention  forward (attention.hip attn_fwd_kernel): raw scores q.k in float32, maximum taken on them, e = exp2(scale2 * (s - max))
             in float32 with the product and the subtraction FUSED (one rounding), UNNORMALISED e rounded to bf16 (pack_b) before P.V, row sum = sum of those bf16 values (the ones-MFMA)
             -- with dropout the float32 e of the undropped softmax --, O = (e_bf16 . V) * (1/(1-p) / sum) -> bf16,
             lse = (max * scale2 + log2(sum)) * ln 2.
             backward (attn_bwd_dq_kernel / attn_bwd_dkv_kernel): P = exp2(s * scale2 + mask * log2e - lse * log2e) in float32,
             dP = dO.V^T in float32, D = rowdot(dO, bf16 O [+ its e5m2 residual byte, with ctx_lo]) in float32, dS = P * (keep ? dP - (1-p) D : -(1-p) D) in float32
             ROUNDED TO bf16 (pack_b(ds0, ds1)) before the dQ / dK products, the (masked) P ROUNDED TO bf16 (pack_b(pr0, pr1))
             before dV; dQ, dK scaled by scale / (1-p), dV by 1 / (1-p), then one bf16 rounding at the store.
  LayerNorm  two-pass statistics in float32 (layernorm.hip row_stats: mean, then sum (x - mean)^2), y in float32 -> bf16;
             backward in float32 from the STORED float32 mean / rstd, dh -> bf16, column sums of the float32 values.
"""
import numpy as np

from rowref import F64, _f64, bf16_round, seq_sum32

F32 = np.float32
M32 = np.uint64(0xFFFFFFFF)
LOG2E32 = F32(1.4426950408889634)
LN2_32 = F32(0.6931471805599453)


def f32(a):
    return np.asarray(a, dtype=F32)


def bf16_rne(a):
    """float64 / float32 array -> float64 values of the bf16 rounding (to nearest even) of its float32 rounding"""
    return bf16_round(np.asarray(a, dtype=F32)).astype(F64)


def _erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gelu(x):
    """erf form: x Phi(x), Phi(x) = (1 + erf(x / sqrt 2)) / 2  -> (gelu, gelu') in the dtype of x"""
    x = np.asarray(x)
    t = x.dtype.type
    cdf = t(0.5) * (t(1) + _erf(x * t(0.7071067811865476)))
    pdf = np.exp(t(-0.5) * x * x) * t(0.3989422804014327)
    return x * cdf, cdf + x * pdf


# ------------------------------------------------------------------ dropout (include/kbner.h, dropout section)
def drop_mix(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def dropout_keep(Z, M, N, seed, thresh):
    """bool [Z, M, N]: element (z, i, j), row key mix(seed + z*M + i), column key mix((seed*0x9E3779B1 + 0x7F4A7C15) ^ (z*N + j)),
    kept iff the low 32 bits of (low 24 bits of rowkey ^ colkey) * 0x9E3779 are >= thresh.  Integer arithmetic only."""
    seed = int(seed) & 0xFFFFFFFF
    rk = drop_mix((np.arange(Z * M, dtype=np.uint64) + np.uint64(seed)) & M32)
    cseed = np.uint64((seed * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF)
    ck = drop_mix(cseed ^ np.arange(Z * N, dtype=np.uint64))
    keep = np.empty((Z, M, N), bool)
    for z in range(Z):
        x = (rk[z * M:(z + 1) * M, None] ^ ck[None, z * N:(z + 1) * N]) & np.uint64(0xFFFFFF)
        keep[z] = ((x * np.uint64(0x9E3779)) & M32) >= np.uint64(thresh)
    return keep


def dropout_scale(thresh):
    """1 / (1 - p) as the kernels compute it: 2^32 / (2^32 - thresh) in float32"""
    return F32(4294967296.0) / (F32(4294967296.0) - F32(np.uint32(thresh)))


def dropout_thresh(p):
    return min(int(round(p * 4294967296.0)), 0xFFFFFFFF)


def dropout_mult(Z, M, N, seed, thresh):
    """the multiplier (0 or 1/(1-p)) as float32 [Z, M, N]"""
    return dropout_keep(Z, M, N, seed, thresh).astype(F32) * dropout_scale(thresh)


# ------------------------------------------------------------------ GEMM
NT, NN, TN = 0, 1, 2
EPI_BIAS, EPI_GELU, EPI_ADD, EPI_DGELU, EPI_DROP, EPI_GELU_FWD = 1, 2, 4, 8, 128, 1024


def _acc(layout, A, B, dot):
    """A, B in their MEMORY layouts: NT A[M,K] B[N,K]; NN A[M,K] B[K,N]; TN A[K,M] B[K,N]"""
    a = A.T if layout == TN else A
    b = B if layout == NT else B.T          # -> [N, K]
    return dot(a, b)


def gemm_ref(layout, A, B, epi=0, bias=None, addend=None, aux=None, alpha=1.0, mask=None):
    """float64, the epilogue order of include/kbner.h: alpha * acc + bias -> dropout (mask = the multiplier) -> + addend ->
    * aux -> gelu.  -> (result before the output rounding, gelu'(pre) or None)"""
    v = float(alpha) * _acc(layout, _f64(A), _f64(B), lambda a, b: a @ b.T)
    if epi & EPI_BIAS:
        v = v + _f64(bias)[None, :]
    if mask is not None:
        v = v * _f64(mask)
    if epi & EPI_ADD:
        v = v + _f64(addend)
    if epi & EPI_DGELU:
        v = v * _f64(aux)
    d = None
    if epi & EPI_GELU:
        v, d = gelu(v)
    elif epi & EPI_GELU_FWD:
        v = gelu(v)[0]
    return v, d


def gemm_sum_abs(layout, A, B, epi=0, bias=None, addend=None, aux=None, alpha=1.0, mask=None):
    """sum of |terms| of the pre-activation (the floor of the tolerance), float64"""
    v = abs(float(alpha)) * _acc(layout, np.abs(_f64(A)), np.abs(_f64(B)), lambda a, b: a @ b.T)
    if epi & EPI_BIAS:
        v = v + np.abs(_f64(bias))[None, :]
    if mask is not None:
        v = v * _f64(mask)
    if epi & EPI_ADD:
        v = v + np.abs(_f64(addend))
    if epi & EPI_DGELU:
        v = v * np.abs(_f64(aux))
    return v


def seq_dot32(a, b):
    """float32 a[R,K] . b[N,K]^T, each dot product added up sequentially over K"""
    a, b = f32(a), f32(b)
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, :, k]
    return acc


def gemm_eval32(layout, A, B, epi=0, bias=None, addend=None, aux=None, alpha=1.0, mask=None, rows=None):
    """the same in float32, accumulating over K sequentially; `rows`: only these output rows (a large output is evaluated on
    a sample of rows: the worst error over a sample is at most the worst error over all, so the tolerance only gets tighter)"""
    a = f32(A).T if layout == TN else f32(A)
    b = f32(B) if layout == NT else f32(B).T
    sl = slice(None) if rows is None else rows
    v = seq_dot32(a[sl], b) * F32(alpha)
    if epi & EPI_BIAS:
        v = v + f32(bias)[None, :]
    if mask is not None:
        v = v * f32(mask)[sl]
    if epi & EPI_ADD:
        v = v + f32(addend)[sl]
    if epi & EPI_DGELU:
        v = v * f32(aux)[sl]
    d = None
    if epi & EPI_GELU:
        v, d = gelu(v)
    elif epi & EPI_GELU_FWD:
        v = gelu(v)[0]
    return v, d


# EXACT GEMM cases: A, B integers of [-4, 4], K <= 4096, |alpha| <= 2, bias / addend integers of [-8, 8], dropout scale <= 4,
# aux of {-2..2}.  Every float32 intermediate is then an integer or a half-integer (alpha = 0.5) of magnitude at most
# gemm_exact_bound() < 2^24: exact in float32 in any summation order.
GEMM_EXACT = {"ab": 4, "K": 4096, "alpha": 2.0, "bias": 8, "drop_scale": 4.0, "addend": 8, "aux": 2, "preload": 8}
# EPI_COLSUM sums the float32 epilogue values; they equal the column sums of the bf16 OUTPUT only where every output is a
# bf16 value: A, B of [-1, 1], K <= 128, aux of {-2..2} -> |out| <= 256 (every integer up to 256 is a bf16 value), M <= 8192 rows
GEMM_COLSUM_EXACT = {"ab": 1, "K": 128, "aux": 2, "M": 8192, "preload": 8}


def gemm_exact_bound():
    g = GEMM_EXACT
    return ((g["ab"] ** 2 * g["K"] * g["alpha"] + g["bias"]) * g["drop_scale"] + g["addend"]) * g["aux"] + g["preload"]


def gemm_colsum_exact_bound():
    g = GEMM_COLSUM_EXACT
    out = g["ab"] ** 2 * g["K"] * g["aux"]
    return out, out * g["M"] + g["preload"]          # largest |output| (must be <= 256), largest |column sum|


def ints(rng, k, shape):
    return rng.integers(-k, k + 1, size=shape).astype(F64)


# ------------------------------------------------------------------ attention (head dim 64, scale 1/8)
D = 64
SCALE = 0.125


def _heads(x, B, S, A):
    """[B*S, A*64] -> [B, A, S, 64]"""
    return x.reshape(B, S, A, D).transpose(0, 2, 1, 3)


def _rows(x, B, S, A):
    """[B, A, S, 64] -> [B*S, A*64]"""
    return x.transpose(0, 2, 1, 3).reshape(B * S, A * D)


def attn_ref(qkv, maskbias, B, S, A, dctx=None, pmask=None):
    """float64 softmax attention per (batch entry, head), derived by hand.  qkv [B*S, 3H] (Q | K | V), maskbias [B, S] added to
    the scores of its KEY, pmask [B, A, S, S] (optional) multiplies the probabilities (dropout: 0 or 1/(1-p)).
      s = q k^T / 8 + maskbias ; lse = logsumexp_j s ; P = exp(s - lse) ; ctx = (P pmask) v
      dPm = dO v^T ; dP = dPm pmask ; dS = P (dP - rowsum(dP P)) ; dq = dS k / 8 ; dk = dS^T q / 8 ; dv = (P pmask)^T dO
    -> dict(ctx [B*S,H], lse [B,A,S], dq, dk, dv [B*S,H])  (the gradients only with dctx)"""
    H = A * D
    x = _f64(qkv)
    q, k, v = (_heads(x[:, i * H:(i + 1) * H], B, S, A) for i in range(3))
    mb = _f64(maskbias)
    out = {"ctx": np.empty((B, A, S, D)), "lse": np.empty((B, A, S))}
    if dctx is not None:
        do = _heads(_f64(dctx), B, S, A)
        for n in ("dq", "dk", "dv"):
            out[n] = np.empty((B, A, S, D))
    for b in range(B):                                         # one batch entry at a time: [A, S, S] temporaries
        s = q[b] @ k[b].transpose(0, 2, 1) * SCALE + mb[b][None, None, :]
        mx = s.max(-1, keepdims=True)
        e = np.exp(s - mx)
        sm = e.sum(-1, keepdims=True)
        out["lse"][b] = (mx + np.log(sm))[..., 0]
        P = e / sm
        Pm = P if pmask is None else P * _f64(pmask[b])
        out["ctx"][b] = Pm @ v[b]
        if dctx is not None:
            dP = do[b] @ v[b].transpose(0, 2, 1)
            if pmask is not None:
                dP = dP * _f64(pmask[b])
            dS = P * (dP - (dP * P).sum(-1, keepdims=True))
            out["dq"][b] = dS @ k[b] * SCALE
            out["dk"][b] = dS.transpose(0, 2, 1) @ q[b] * SCALE
            out["dv"][b] = Pm.transpose(0, 2, 1) @ do[b]
    for n in out:
        if n != "lse":
            out[n] = _rows(out[n], B, S, A)
    return out


def _bf(x):
    return bf16_round(f32(x))


def e5m2_round(x):
    """float32 -> the nearest e5m2 value (2 mantissa bits, round to nearest even, denormals of step 2^-16), clamped to +-57344:
    the residual byte of csrc/common.h pack2bf_res8"""
    x = np.clip(f32(x), F32(-57344.0), F32(57344.0)).astype(F64)
    a = np.abs(x)
    ex = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    step = np.exp2(np.maximum(ex, -14.0) - 2.0)
    return f32(np.sign(x) * np.rint(a / step) * step)


def attn_eval32(qkv, maskbias, B, S, A, dctx=None, keep=None, thresh=0, entries=None, use_exp2=True, residual=False):
    """float32 evaluation with the kernels' rounding points (module docstring).  keep: bool [B, A, S, S] (dropout) with its
    thresh; entries: the batch entries to evaluate (default all) -> the same dict as attn_ref holding [len(entries), A, S, 64]
    arrays (lse [len(entries), A, S]): compare with _heads(reference)[entries].
    The forward exponent is the FUSED a * scale2 + (-max * scale2) of attn_fwd_kernel: the product exact, the max term rounded,
    one rounding of the sum -- so the largest e of a row is 1 + delta, |delta| <= 2^-24 |max * scale2| ln 2, not 1.
    residual: D also takes the e5m2 byte of (O - bf16 O) * 2^14 the forward stores in ctx_lo (kbner_attn_bwd)."""
    H = A * D
    x = f32(qkv)
    q, k, v = (_heads(x[:, i * H:(i + 1) * H], B, S, A) for i in range(3))
    mb = f32(maskbias)
    entries = list(range(B)) if entries is None else list(entries)
    dscale = dropout_scale(thresh) if keep is not None else F32(1)
    scale = F32(SCALE)
    scale2 = scale * LOG2E32
    n = len(entries)
    out = {"ctx": np.empty((n, A, S, D), F32), "lse": np.empty((n, A, S), F32)}
    if dctx is not None:
        do = _heads(f32(dctx), B, S, A)
        for nm in ("dq", "dk", "dv"):
            out[nm] = np.empty((n, A, S, D), F32)
    for i, b in enumerate(entries):
        raw = q[b] @ k[b].transpose(0, 2, 1) + (mb[b] * (F32(1) / scale))[None, None, :]     # accumulators start at mask / scale
        mx = raw.max(-1, keepdims=True)
        if use_exp2:
            e = np.exp2(f32(raw.astype(F64) * F64(scale2) - (mx * scale2).astype(F64)))
        else:
            e = np.exp(raw * scale - mx * scale)
        kp = None if keep is None else keep[b]
        eb = _bf(e if kp is None else e * kp)
        sm = (eb if kp is None else e).sum(-1, keepdims=True, dtype=F32)
        o = (eb @ v[b]) * (dscale / sm)
        out["ctx"][i] = o
        lse = ((mx * scale2 + np.log2(sm)) * LN2_32) if use_exp2 else (mx * scale + np.log(sm))
        out["lse"][i] = lse[..., 0]
        if dctx is None:
            continue
        P = np.exp2(raw * scale2 - lse * LOG2E32) if use_exp2 else np.exp(raw * scale - lse)
        ob = _bf(o)
        Dq = (do[b] * ob).sum(-1, keepdims=True, dtype=F32)
        if residual:
            Dq = Dq + (do[b] * e5m2_round((o - ob) * F32(16384.0))).sum(-1, keepdims=True, dtype=F32) * F32(1.0 / 16384.0)
        Dq = Dq * (F32(1) / dscale)
        dP = do[b] @ v[b].transpose(0, 2, 1) - Dq
        if kp is not None:
            dP = np.where(kp, dP, -Dq)
        dSb = _bf(P * dP)
        out["dq"][i] = (dSb @ k[b]) * (scale * dscale)
        out["dk"][i] = (dSb.transpose(0, 2, 1) @ q[b]) * (scale * dscale)
        Pb = _bf(P if kp is None else P * kp)
        out["dv"][i] = (Pb.transpose(0, 2, 1) @ do[b]) * dscale
    return out


# EXACT attention, the one-hot construction: key j carries the 9-bit code of j as +-8 in dimensions 0..62 (7 copies of the 9
# bits), dimension 63 is 0; query i carries the code of pi(i).  q.k / 8 = 504 where the codes agree and at most 392 = 504 - 2*7*8
# elsewhere: exp(-112) < 2^-149 is 0 in float32, so is exp(-10000) of a masked key -> exactly one probability, equal to 1.
ONEHOT_HIT, ONEHOT_MISS = 504.0, 392.0
ATTN_EXACT = {"v": 4, "do": 1}     # V integers of [-4, 4]: bf16 values; dO of {-1, 0, 1}: dV[j] = sum of dO over pi(i) = j


def onehot_codes(idx):
    """[n] integers below 512 -> [n, 64] float64 rows of +-8 (dimension 63: 0)"""
    idx = np.asarray(idx)
    bits = ((idx[:, None] >> np.arange(9)[None, :]) & 1) * 2.0 - 1.0
    out = np.zeros((idx.shape[0], D))
    out[:, :63] = np.tile(bits, (1, 7)) * 8.0
    return out


def onehot_case(rng, B, S, A, n_real=None):
    """-> qkv [B*S, 3H], dctx [B*S, H] (float64, bf16 values), maskbias [B, S] float32, pi [B, A, S] (the key each query
    selects).  n_real: per batch entry the number of unmasked keys (None: all S, pi a permutation; else a random map onto
    [0, n_real[b]))."""
    H = A * D
    n_real = [S] * B if n_real is None else list(n_real)
    pi = np.empty((B, A, S), np.int64)
    for b in range(B):
        for a in range(A):
            pi[b, a] = rng.permutation(S) if n_real[b] == S else rng.integers(0, n_real[b], size=S)
    kcode = onehot_codes(np.arange(S))
    q = onehot_codes(pi.reshape(-1)).reshape(B, A, S, D)
    k = np.broadcast_to(kcode, (B, A, S, D))
    v = ints(rng, ATTN_EXACT["v"], (B, A, S, D))
    qkv = np.concatenate([_rows(np.ascontiguousarray(t), B, S, A) for t in (q, k, v)], axis=1)
    dctx = ints(rng, ATTN_EXACT["do"], (B * S, H))
    mb = np.zeros((B, S), F32)
    for b in range(B):
        mb[b, n_real[b]:] = -10000.0
    return qkv, dctx, mb, pi


def onehot_expected(qkv, dctx, pi, B, S, A, keep=None, scale=1.0):
    """ctx[i] = scale * keep(i, pi(i)) * V[pi(i)];  dV[j] = scale * sum of kept dO[i] over pi(i) = j  (float64, [B*S, H])"""
    H = A * D
    v = _heads(_f64(qkv)[:, 2 * H:], B, S, A)
    do = _heads(_f64(dctx), B, S, A)
    ctx = np.zeros((B, A, S, D))
    dv = np.zeros((B, A, S, D))
    for b in range(B):
        for a in range(A):
            w = np.full(S, float(scale)) if keep is None else keep[b, a, np.arange(S), pi[b, a]] * float(scale)
            ctx[b, a] = v[b, a, pi[b, a]] * w[:, None]
            np.add.at(dv[b, a], pi[b, a], do[b, a] * w[:, None])
    return _rows(ctx, B, S, A), _rows(dv, B, S, A)


# ------------------------------------------------------------------ LayerNorm
def ln_ref(h, gamma, beta, eps, dy=None, mult=None):
    """y = (h - mean) rstd gamma + beta, rstd = 1 / sqrt(var + eps) (biased variance).  Backward for the incoming dy, with
    xhat = (h - mean) rstd, g = dy gamma:  dh = rstd (g - mean_H(g) - xhat mean_H(g xhat)); dgamma = sum_rows dy xhat;
    dbeta = sum_rows dy; dhm = dh * mult (the dropout multiplier of the GEMM that fed h; None: dh); dbias = sum_rows dhm."""
    h, gamma = _f64(h), _f64(gamma)
    mean = h.mean(1)
    var = ((h - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (h - mean[:, None]) * rstd[:, None]
    out = {"y": xh * gamma + _f64(beta), "mean": mean, "rstd": rstd}
    if dy is not None:
        d = _f64(dy)
        g = d * gamma
        dh = rstd[:, None] * (g - g.mean(1)[:, None] - xh * (g * xh).mean(1)[:, None])
        dhm = dh if mult is None else dh * _f64(mult)
        out.update(dh=dh, dhm=dhm, dgamma=(d * xh).sum(0), dbeta=d.sum(0), dbias=dhm.sum(0))
    return out


def ln_eval32(h, gamma, beta, eps, dy=None, mult=None):
    """the same in sequential float32, two-pass statistics; backward from the float32 mean / rstd"""
    h, gamma, beta = f32(h), f32(gamma), f32(beta)
    H = h.shape[1]
    mean = seq_sum32(h, 1) / F32(H)
    c = h - mean[:, None]
    rstd = F32(1) / np.sqrt(seq_sum32(c * c, 1) / F32(H) + F32(eps))
    xh = c * rstd[:, None]
    out = {"y": xh * gamma + beta, "mean": mean, "rstd": rstd}
    if dy is not None:
        d = f32(dy)
        g = d * gamma
        s1 = seq_sum32(g, 1) / F32(H)
        s2 = seq_sum32(g * xh, 1) / F32(H)
        dh = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
        dhm = dh if mult is None else dh * f32(mult)
        out.update(dh=dh, dhm=dhm, dgamma=seq_sum32(d * xh, 0), dbeta=seq_sum32(d, 0), dbias=seq_sum32(dhm, 0))
    return out


def ln_exact_case(rng, M, H):
    """rows of -1 / +1 in equal numbers (H even), integer gamma of [-3, 3] and beta of [-4, 4]: with eps = 0 mean == 0,
    rstd == 1 and y == gamma x + beta, integers of magnitude <= 7"""
    h = np.ones((M, H))
    h[:, :H // 2] = -1.0
    h = rng.permuted(h, axis=1)
    return h, ints(rng, 3, H), ints(rng, 4, H)


# The one-hot cases both test modules walk (tests/test_mmaref_cpu.py asserts their preconditions, tests/test_gpu_mma_kernels.py
# runs them): (B, S, A, ragged, residual, dropout p).  Ragged: batch entry b has n_real_list(S)[b % len] real keys.
def n_real_list(S):
    return sorted({n for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, S - 1, S) if n <= S})


ONEHOT_CASES = (
    # all eight instantiations S / 64 = 1..8, small batch: 128-row workgroup tiles (16-row kernels, grid launch), every n_real
    [(13, S, 2, True, (S // 64) % 2 == 1, 0.0) for S in range(64, 513, 64)]
    + [(2, S, 2, False, (S // 64) % 2 == 0, 0.0) for S in (64, 192, 384, 448, 512)]
    # dropout 0.5 (the 16-row forward kernels with the keep tests; both backward families)
    + [(13, 128, 2, True, False, 0.5), (13, 448, 1, True, True, 0.5), (64, 256, 8, True, False, 0.5)]
    # 512 heads: 256-row tiles at S = 256 (whole heads: persistent walk on 256 CUs), 512-row tiles at S = 512 (persistent) and at
    # S = 320 / 384 / 448 (512-row tiles LARGER than the head: waves past S idle), 256-row tiles at S = 192 likewise
    + [(64, 256, 8, True, False, 0.0), (64, 512, 8, True, True, 0.0), (64, 192, 8, True, True, 0.0),
       (64, 384, 8, True, False, 0.0), (64, 448, 8, False, True, 0.0), (64, 320, 8, True, False, 0.0)]
    # 256 heads at S = 512: 256-row tiles, two workgroups per head, grid launch
    + [(32, 512, 8, True, False, 0.0)]
)


def onehot_inputs(case):
    B, S, A, ragged, _res, _p = case
    rng = np.random.default_rng(B * 100003 + S * 101 + A * 7 + int(ragged))
    nr = None
    if ragged:
        lst = n_real_list(S)
        nr = [lst[b % len(lst)] for b in range(B)]
    return onehot_case(rng, B, S, A, nr)


def pick_rpw(B, S, A):
    """rows per workgroup of the attention launchers (csrc/attention.hip pick_rpw), restated so that a case list can say
    which route it reaches"""
    rpw = 512
    while rpw > 128 and (rpw // 2 >= S or B * A * ((S + rpw - 1) // rpw) < 512):
        rpw //= 2
    return rpw
