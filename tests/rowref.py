"""TEST INFRASTRUCTURE: plain float64 references of the row / head / embedding / optimizer operations behind
csrc/rows.hip, the embedding half of csrc/layernorm.hip and the flat utilities of csrc/optim.hip, written from the
formulas in include/kbner.h (numpy only, no kernel structure: no chunks, no waves, no summation order).

tests/test_rowref_cpu.py proves these functions against torch.autograd (float64) and oracle/optim.py on the CPU;
tests/test_gpu_row_kernels.py compares the HIP kernels with them.

Also here, because both test modules need them: the integer-valued input generators of the EXACT cases (with the bound
that makes fp32 addition exact in any order) and the tolerance rule of the REAL-VALUED cases.
"""
import numpy as np

F64 = np.float64


def _f64(a):
    return np.asarray(a, dtype=F64)


# ------------------------------------------------------------------ row moves
def gather(src, idx):
    """out[r] = src[idx[r]] if idx[r] >= 0 else 0  (dtype of src kept: a pure copy)"""
    src = np.asarray(src)
    idx = np.asarray(idx)
    out = np.zeros((idx.shape[0],) + src.shape[1:], dtype=src.dtype)
    keep = idx >= 0
    out[keep] = src[idx[keep]]
    return out


def scatter(dst, rows, idx):
    """dst[idx[r]] = rows[r] for idx[r] >= 0 (unique indices); every other row of dst is returned as it was"""
    out = np.array(dst, copy=True)
    idx = np.asarray(idx)
    keep = idx >= 0
    out[idx[keep]] = np.asarray(rows)[keep]
    return out


def scatter_add(dst, rows, idx):
    """dst[idx[r]] += rows[r] for idx[r] >= 0, float64 (repeated indices add up)"""
    out = _f64(dst).copy()
    idx = np.asarray(idx)
    keep = idx >= 0
    np.add.at(out, idx[keep], _f64(rows)[keep])
    return out


# ------------------------------------------------------------------ emission head
def head_fwd(x, w, b):
    """out[r,t] = sum_h x[r,h] w[t,h] + b[t]"""
    return _f64(x) @ _f64(w).T + _f64(b)


def head_bwd(de, x, w):
    """-> dx[r,h] = sum_t de[r,t] w[t,h];  dw[t,h] = sum_r de[r,t] x[r,h];  db[t] = sum_r de[r,t]"""
    de, x, w = _f64(de), _f64(x), _f64(w)
    return de @ w, de.T @ x, de.sum(0)


def colsum(x):
    """out[n] = sum_m x[m,n]"""
    return _f64(x).sum(0)


# ------------------------------------------------------------------ embeddings + LayerNorm
def embed_ln_fwd(ids, pos_ids, word, pos, type0, gamma, beta, eps, mult=None, h0=None):
    """BertEmbeddings.forward: h0 = word[ids] + pos[pos_ids] + type0; y = LayerNorm(h0) * gamma + beta (eps inside the
    root), then the dropout multiplier `mult` (0 or 1/(1-p) per element).  -> h0, y, mean, rstd.
    `h0`: normalise THIS matrix instead of the sum (the kernel normalises what it stored: the bf16 rounding of the sum)."""
    s = _f64(word)[np.asarray(ids)] + _f64(pos)[np.asarray(pos_ids)] + _f64(type0)
    h = s if h0 is None else _f64(h0)
    mean = h.mean(1)
    var = ((h - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    y = (h - mean[:, None]) * rstd[:, None] * _f64(gamma) + _f64(beta)
    if mult is not None:
        y = y * _f64(mult)
    return s, y, mean, rstd


def embed_ln_bwd(dy, h0, mean, rstd, gamma, ids, pos_ids, n_word, n_pos, mult=None):
    """Backward of embed_ln_fwd for the incoming gradient dy of y.  With xhat = (h0 - mean) rstd, d = dy * mult,
    g = d * gamma:   dh = rstd (g - mean_H(g) - xhat mean_H(g xhat));  dgamma = sum_rows d xhat;  dbeta = sum_rows d;
    dword / dpos = scatter-add of dh by ids / pos_ids;  dtype0 = sum_rows dh;  flags[v] = 3 (KBNER_ROW_LIVE |
    KBNER_ROW_TOUCHED) for every word row an id names, else 0.
    -> dict(dh, dgamma, dbeta, dword, dpos, dtype0, flags)"""
    d = _f64(dy)
    if mult is not None:
        d = d * _f64(mult)
    xh = (_f64(h0) - _f64(mean)[:, None]) * _f64(rstd)[:, None]
    g = d * _f64(gamma)
    dh = _f64(rstd)[:, None] * (g - g.mean(1)[:, None] - xh * (g * xh).mean(1)[:, None])
    H = dh.shape[1]
    ids = np.asarray(ids)
    pos_ids = np.asarray(pos_ids)
    flags = np.zeros(n_word, np.uint8)
    flags[ids] = 3
    return {"dh": dh, "dgamma": (d * xh).sum(0), "dbeta": d.sum(0),
            "dword": scatter_add(np.zeros((n_word, H)), dh, ids), "dpos": scatter_add(np.zeros((n_pos, H)), dh, pos_ids),
            "dtype0": dh.sum(0), "flags": flags}


# ------------------------------------------------------------------ optimizer
def bf16_round(a):
    """float32 array -> the float32 values of its bfloat16 rounding (round to nearest even), through torch on the CPU"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def adamw_hf(p, g, m, v, step_size, lr_wd=0.0, b1=0.9, b2=0.999, eps=1e-6, gnorm_sq=None, max_norm=5.0, grad_scale=1.0,
             n_shadow=None):
    """One step of transformers==3.0.0 AdamW behind clip_grad_norm_ (include/kbner.h, optimiser section), float64:
         the gradient in use is g * grad_scale, its norm sqrt(gnorm_sq) * grad_scale (gnorm_sq = sum g^2 of the stored g)
         coef = max_norm / (norm + 1e-6), applied iff < 1         (gnorm_sq None: no clipping)
         m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2 ;  p -= step_size m / (sqrt(v) + eps) ;  p -= lr_wd p
    -> p, m, v (new float64 arrays) and shadow = bf16(float32(p))[:n_shadow] as float32 (None when n_shadow is None)."""
    p, g, m, v = _f64(p).copy(), _f64(g), _f64(m).copy(), _f64(v).copy()
    gs = float(grad_scale)
    if gnorm_sq is not None:
        norm = np.sqrt(float(gnorm_sq)) * grad_scale
        coef = max_norm / (norm + 1e-6)
        if coef < 1.0:
            gs *= coef
    gk = g * gs
    m = b1 * m + (1.0 - b1) * gk
    v = b2 * v + (1.0 - b2) * gk * gk
    p = p - step_size * (m / (np.sqrt(v) + eps))
    if lr_wd != 0.0:
        p = p - lr_wd * p
    shadow = None if n_shadow is None else bf16_round(p.astype(np.float32)[:n_shadow])
    return p, m, v, shadow


def sqnorm(g):
    g = _f64(g)
    return float((g * g).sum())


def wdiff_sum(a, b, w):
    """sum_i w[i] (a[i] - b[i])"""
    return float((_f64(w) * (_f64(a) - _f64(b))).sum())


# ------------------------------------------------------------------ EXACT cases: integer-valued inputs
# A case draws every factor of a term from the integers of [-k, k] and adds at most `terms` terms to a start value of at
# most `start`: every partial sum, in any order, is an integer of magnitude <= terms * prod(k) + start.  Below 2^24 each of
# them is a float32, so float32 addition is exact whatever the order (atomics included) and the result must EQUAL the
# float64 reference.  test_rowref_cpu.py asserts the bound for every entry; the GPU tests draw their inputs through
# ints(..., EXACT[name][factor]) and check their sizes against `terms`, so the table is what runs.
EXACT_LIMIT = 2 ** 24
EXACT = {
    # name: (factor ranges k, largest number of terms, largest start value)
    "head_fwd": ({"x": 4, "w": 2, "b": 8}, 8192, 8),            # sum over H <= 8192 of x w, + bias
    "head_bwd_dx": ({"de": 2, "w": 2}, 64, 0),                  # sum over T <= 64 of de w: also <= 256, bf16-exact
    "head_bwd_dw": ({"de": 2, "x": 4}, 70000, 8),               # sum over R <= 70 000 of de x into a pre-filled dw
    "head_bwd_db": ({"de": 2}, 70000, 8),
    "colsum": ({"x": 8}, 65536, 8),
    "colsum_rows": ({"ws": 64}, 1024, 8),
    "scatter_add": ({"rows": 64}, 1, 64),
    "sqnorm_block": ({"g": 3, "g2": 3}, 40000004 // 2048 + 256 * 4, 0),   # one workgroup's share of g^2 (<= n / 2048 + a stride's tail)
    "wdiff_sum": ({"w": 8, "d": 16}, 1000, 0),                  # d = a - b with a, b in [-8, 8]
}


def exact_bound(name):
    ranges, terms, start = EXACT[name]
    prod = 1
    for k in ranges.values():
        prod *= k
    return terms * prod + start


def ints(rng, k, shape):
    """integers of [-k, k], float64"""
    return rng.integers(-k, k + 1, size=shape).astype(F64)


# ------------------------------------------------------------------ REAL-VALUED cases: the tolerance rule
BF16_ULP = 2.0 ** -8     # one bf16 ulp, relative (8 significand bits)
F32_EPS = 2.0 ** -24


def tolerance(ref64, eval32, sum_abs, bf16_out=False, scale=1.0):
    """Elementwise tolerance of a kernel output against ref64:
         scale * max( 8 * max_elements |eval32 - ref64| ,  2 * 2^-24 * sum_abs )   [+ 2^-8 |ref64| for a bf16 output]
    eval32: the same formula evaluated in plain float32 numpy (sequential sums); its worst error over the output is what a
    float32 implementation of this size loses, the factor 8 covers another summation order and FMA contraction.  sum_abs
    (per element or scalar): sum of |terms| of the float64 evaluation; the floor keeps a case whose float32 evaluation
    happens to be exact from demanding bit equality."""
    ref64 = _f64(ref64)
    err32 = float(np.abs(_f64(eval32) - ref64).max()) if np.size(ref64) else 0.0
    tol = scale * np.maximum(8.0 * err32, 2.0 * F32_EPS * _f64(sum_abs)) + np.zeros_like(ref64)
    if bf16_out:
        tol = tol + BF16_ULP * np.abs(ref64)
    return tol, err32


def seq_sum32(terms, axis):
    """sequential float32 sum along `axis` (np.sum adds pairwise; a cumulative sum cannot)"""
    t = np.asarray(terms, dtype=np.float32)
    if t.shape[axis] == 0:
        return np.zeros(np.delete(t.shape, axis), np.float32)
    return np.take(np.cumsum(t, axis=axis, dtype=np.float32), -1, axis=axis)


def seq_dot32(a, b):
    """float32 a[R,K] . b[N,K]^T with each dot product added up sequentially over K (one rank-1 update per k)"""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, :, k]
    return acc
