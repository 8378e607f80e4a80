"""TEST INFRASTRUCTURE: float64 / integer reference of the tagger head's dropout on the token features -- the multiplier of
kbner_gather_rows_drop / kbner_scatter_rows_drop (include/kbner.h) and the two row moves with it applied.  numpy only, built
from the integer keep test and the float32 scale of tests/mmaref.py; no kernel structure, no import of kbner.

Rows are laid out [B, n] (R = B * n): row r belongs to sentence r // n.  Two sites, each a (seed, thresh) pair:
    element mask  m_e(r, h): element (r, h)      of site drop_e   (torch.nn.Dropout)
    locked mask   m_l(r, h): element (r // n, h) of site drop_l   (flair.nn.LockedDropout: one value per (sentence, column))
thresh == 0 disables a site (multiplier 1).  The product m_e * m_l is formed in float32, as the kernels form it.

tests/test_headdrop_cpu.py proves gather / scatter against torch.autograd; tests/test_gpu_headdrop_kernels.py and
tests/test_gpu_headdrop_e2e.py compare the HIP kernels and the engine with them."""
import numpy as np

import mmaref

F32, F64 = np.float32, np.float64
NO_DROP = (0, 0)


def keep(R, H, n, drop_e, drop_l):
    """(bool [R, H] of the element site, bool [R, H] of the locked site expanded over the n rows of each sentence)"""
    if n < 1 or R % n:
        raise ValueError("rows are [B, n]: R %% n == 0, n >= 1")
    ke = np.ones((R, H), bool) if drop_e[1] == 0 else mmaref.dropout_keep(1, R, H, drop_e[0], drop_e[1])[0]
    kl = np.ones((R // n, H), bool) if drop_l[1] == 0 else mmaref.dropout_keep(1, R // n, H, drop_l[0], drop_l[1])[0]
    return ke, np.repeat(kl, n, axis=0)


def mult(R, H, n, drop_e=NO_DROP, drop_l=NO_DROP):
    """the multiplier m_e * m_l as float32 [R, H]"""
    ke, kl = keep(R, H, n, drop_e, drop_l)
    se = F32(1.0) if drop_e[1] == 0 else mmaref.dropout_scale(drop_e[1])
    sl = F32(1.0) if drop_l[1] == 0 else mmaref.dropout_scale(drop_l[1])
    return (ke.astype(F32) * F32(se)) * (kl.astype(F32) * F32(sl))


def gather(x64, idx, n, drop_e=NO_DROP, drop_l=NO_DROP):
    """y[r] = idx[r] >= 0 ? x[idx[r]] * M[r] : 0   (float64, unrounded; x64 [rows_src, H], idx [R])"""
    x64 = np.asarray(x64, F64)
    idx = np.asarray(idx, np.int64)
    R, H = idx.size, x64.shape[1]
    M = mult(R, H, n, drop_e, drop_l).astype(F64)
    y = np.zeros((R, H), F64)
    ok = idx >= 0
    y[ok] = x64[idx[ok]] * M[ok]
    return y


def scatter(d64, idx, rows_src, n, drop_e=NO_DROP, drop_l=NO_DROP):
    """the backward of gather: dx[idx[r]] = d[r] * M[r] for idx[r] >= 0 (unique indices), zeros elsewhere; float64 [rows_src, H]"""
    d64 = np.asarray(d64, F64)
    idx = np.asarray(idx, np.int64)
    R, H = idx.size, d64.shape[1]
    M = mult(R, H, n, drop_e, drop_l).astype(F64)
    ok = idx >= 0
    assert np.unique(idx[ok]).size == int(ok.sum()), "scatter: indices must be unique"
    dx = np.zeros((rows_src, H), F64)
    dx[idx[ok]] = d64[:R][ok] * M[ok]
    return dx


def real_bound(ref64):
    """per-element bound of a bf16 result against the float64 reference: one bf16 rounding (2^-8 relative at the bottom of a
    binade) + three float32 roundings (the scale product, the two factors' quotients folded into it, the value product)"""
    a = np.abs(np.asarray(ref64, F64))
    return 2.0 ** -8 * a + 4 * 2.0 ** -24 * a
