"""TEST INFRASTRUCTURE: numpy reference of kbner_gather_rows_blocks_drop (include/kbner.h), written from its definition -- no kernel
structure, no import of kbner.  The two dropout multipliers are INPUTS (a test materialises them with kbner_dropout_mask, or draws
them itself), so the reference holds no keep test:

    out[r, c] = (r < R and c < W and idx[r] >= 0 and block_on[blk(c)]) ? bf16(store[idx[r], c] * (m_e[r, c] * m_l[r // n, c])) : 0
                                                                                                   r < R_out, c < ld_out
    blk(c): the block b with block_col[b] <= c < block_col[b + 1]; a column outside every block is 0.

store holds bf16 values (as float32); m_e float32 [R, W] or None (all 1), m_l float32 [R // n, W] or None.  The product of the two
multipliers and the product with the value are float32 operations, the result is rounded to bf16 once (round to nearest even): what
the definition says, so a kernel that follows it gives EXACTLY these values.

tests/test_feature_store_cpu.py checks this file against a per-element loop and shows that `mismatch` refuses defective
evaluations; tests/test_gpu_store_kernels.py compares the HIP kernel with it."""
import numpy as np
import torch

F32 = np.float32


def bf16_round(a):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).bfloat16().float().numpy()


def check_contract(ld_store, block_col, nblk, ld_out, R, R_out, W, n):
    """the contract of the entry point: True when the call is legal (an illegal one returns -22)"""
    cols = [int(c) for c in block_col]
    return bool(1 <= nblk <= 64 and len(cols) == nblk + 1 and all(c % 8 == 0 for c in cols) and cols[0] >= 0
                and all(b >= a for a, b in zip(cols, cols[1:])) and cols[-1] <= W <= ld_store and W % 8 == 0 and ld_store % 8 == 0
                and ld_out % 8 == 0 and W <= ld_out and n >= 1 and R >= 0 and R % n == 0 and R <= R_out)


def column_on(block_col, block_on, width):
    """bool [width]: column c lies in a block that is switched on"""
    on = np.zeros(width, bool)
    for b in range(len(block_col) - 1):
        lo, hi = int(block_col[b]), min(int(block_col[b + 1]), width)
        if hi > lo:
            on[lo:hi] = bool(block_on[b])
    return on


def gather_blocks(store, idx, block_col, block_on, ld_out, R_out, W, n, m_e=None, m_l=None):
    """-> float32 [R_out, ld_out] holding bf16 values"""
    store = np.asarray(store, F32)
    idx = np.asarray(idx, np.int64)
    R = idx.size
    assert check_contract(store.shape[1], block_col, len(block_col) - 1, ld_out, R, R_out, W, n)
    m = np.ones((R, W), F32)
    if m_e is not None:
        m = m * np.asarray(m_e, F32)[:R, :W]
    if m_l is not None:
        m = m * np.repeat(np.asarray(m_l, F32)[:R // n, :W], n, axis=0)
    out = np.zeros((R_out, ld_out), F32)
    rows = np.nonzero(idx >= 0)[0]
    cols = np.nonzero(column_on(block_col, block_on, W))[0]
    if rows.size and cols.size:
        out[np.ix_(rows, cols)] = bf16_round(store[np.ix_(idx[rows], cols)] * m[np.ix_(rows, cols)])
    return out


def mismatch(got, want):
    """compare a result with the reference, element for element and exactly (one definition, one rounding: no tolerance; +0 and -0
    are the same value) -> None when equal, else a description of the first differing element"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not bad.any():
        return None
    r, c = np.argwhere(bad)[0]
    return "%d of %d elements differ, first at [%d, %d]: %r, expected %r" % (int(bad.sum()), bad.size, r, c, float(got[r, c]),
                                                                            float(want[r, c]))
