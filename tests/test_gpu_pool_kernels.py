"""GPU: kbner_pool_rows_layers (csrc/rows.hip) through kbner.ops.pool_rows_layers against tests/poolref.py.

The case list of poolref.POOL_CASES -- R in {1, 6, 70}, H in {8, 128, 520, 1024}, k in {1, 2, 4}, the four pooling operations, with and
without the layer mean -- on Gaussian bf16 sources, with span tables that hold empty spans (first and last row), spans of 1, 2, 3 and 17
rows, a seam (non-consecutive, non-monotone rows) and a source row two words name.  Every launch writes its block at a non-zero column
of a wider matrix with three more rows, pre-filled with a sentinel: everything outside the block must keep it.  first / last /
first_last without the layer mean are copies: bit equality; the rest inside poolref.bound; the exact cases (integers, m and k powers of
two; one on bf16 ties) bit for bit.  A mean over one row equals the copy.  Malformed tables are refused on the host."""
import numpy as np
import pytest
import torch

import poolref as pr

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
EXTRA_ROWS = 3


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    return _ops


def _dev_bf16(a64):
    """float64 values that ARE bf16 numbers -> device bf16 tensor (asserted lossless)"""
    t = torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).bfloat16()
    assert np.array_equal(t.float().numpy().astype(np.float64), a64)
    return t.to(DEV)


def _run(ops, xs, sp, sr, op, lm, col=16, pad=24):
    """-> the whole output matrix as float64 [R + EXTRA_ROWS, col + W + pad]"""
    R = len(sp) - 1
    W = pr.width(op, len(xs), xs[0].shape[1], lm)
    full = torch.full((R + EXTRA_ROWS, col + W + pad), pr.SENTINEL, dtype=BF16, device=DEV)
    ops.pool_rows_layers([_dev_bf16(x) for x in xs], sp, sr, full, col, op, layer_mean=lm)
    torch.cuda.synchronize()
    return full.float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("case", pr.POOL_CASES, ids=lambda c: "R%d-H%d-k%d-%s-%s" % (c[0], c[1], c[2], c[3], "lm" if c[4] else "cat"))
def test_pool_real(ops, case):
    R, H, k, op, lm = case
    xs, sp, sr = pr.pool_inputs(R, H, k)
    full = _run(ops, xs, sp, sr, op, lm)
    pr.check_matrix(full, R, 16, xs, sp, sr, op, lm)
    m = pr.span_lengths(sp)
    W = pr.width(op, k, H, lm)
    block = full[:R, 16:16 + W]
    assert not block[m == 0].any(), "a word without a sub-token must pool to zeros"
    if op == "mean" and not lm and (m == 1).any():               # a span of one row: the mean is the copy, exactly
        assert np.array_equal(block[m == 1], pr.pool_layers(xs, sp, sr, "first", False)[m == 1])


@pytest.mark.parametrize("op,lm", pr.EXACT_CASES)
def test_pool_exact(ops, op, lm):
    xs, sp, sr = pr.exact_inputs()
    full = _run(ops, xs, sp, sr, op, lm, col=8, pad=8)
    pr.check_matrix(full, len(sp) - 1, 8, xs, sp, sr, op, lm, exact=True)


def test_pool_tie_rounds_to_nearest_even(ops):
    xs, sp, sr, want = pr.tie_inputs()
    full = _run(ops, xs, sp, sr, "mean", False, col=8, pad=8)
    pr.check_matrix(full, 1, 8, xs, sp, sr, "mean", False, exact=True)
    assert np.array_equal(full[:1, 8:16], want)


def test_pool_col_zero_and_all_empty(ops):
    """the block at column 0 of a matrix exactly W wide; a table whose spans are all empty writes zeros and reads nothing"""
    xs, sp, sr = pr.pool_inputs(6, 128, 2)
    full = torch.full((6, 256), pr.SENTINEL, dtype=BF16, device=DEV)
    ops.pool_rows_layers([_dev_bf16(x) for x in xs], sp, sr, full, 0, "last", layer_mean=False)
    torch.cuda.synchronize()
    pr.check(full.float().cpu().numpy(), xs, sp, sr, "last", False)
    full.fill_(pr.SENTINEL)
    ops.pool_rows_layers([_dev_bf16(x) for x in xs], np.zeros(7, np.int64), np.zeros(0, np.int64), full, 0, "mean", layer_mean=True)
    torch.cuda.synchronize()
    got = full.float().cpu().numpy()
    assert not got[:, :128].any() and (got[:, 128:] == pr.SENTINEL).all()


def test_pool_refusals_reach_no_kernel(ops):
    from kbner import lib as L
    xs, sp, sr = pr.pool_inputs(6, 128, 2)
    srcs = [_dev_bf16(x) for x in xs]
    full = torch.full((6, 512), pr.SENTINEL, dtype=BF16, device=DEV)
    rows_src = xs[0].shape[0]
    bad_rows = sr.copy()
    bad_rows[3] = rows_src
    neg_rows = sr.copy()
    neg_rows[0] = -1
    bad_ptr = sp.copy()
    bad_ptr[2], bad_ptr[3] = bad_ptr[3], bad_ptr[2] - 1
    for kw in (dict(span_rows=bad_rows), dict(span_rows=neg_rows), dict(span_ptr=bad_ptr), dict(span_ptr=sp[:-2]),
               dict(span_ptr=np.concatenate([sp, [sp[-1]]])), dict(col=4), dict(col=264), dict(op="max"),
               dict(srcs=[srcs[0], srcs[1][:, :64].contiguous()]), dict(srcs=[srcs[0].float()]), dict(srcs=[])):
        a = dict(srcs=srcs, span_ptr=sp, span_rows=sr, out2d=full, col=0, op="mean")
        a.update(kw)
        with pytest.raises(L.KbnerError):
            ops.pool_rows_layers(a["srcs"], a["span_ptr"], a["span_rows"], a["out2d"], a["col"], a["op"])
    torch.cuda.synchronize()
    assert (full.float() == pr.SENTINEL).all()
    # the C entry point's own argument checks: -22 and nothing launched
    import ctypes
    lib, st = L.load(), L.stream_ptr()
    ptrs = (ctypes.c_void_p * 2)(*[s.data_ptr() for s in srcs])
    spd, srd = torch.from_numpy(sp.astype(np.int32)).to(DEV), torch.from_numpy(sr.astype(np.int32)).to(DEV)

    def raw(k=2, lm=0, op=3, out=full.data_ptr(), ld=512, R=6, H=128):
        return lib.kbner_pool_rows_layers(ptrs, k, lm, op, L.ptr(spd), L.ptr(srd), ctypes.c_void_p(out), ld, R, H, st)

    assert raw() == 0
    for kw in (dict(k=0), dict(k=33), dict(op=4), dict(op=-1), dict(H=12), dict(ld=508), dict(out=full.data_ptr() + 2), dict(ld=248),
               dict(op=2, ld=504), dict(R=-1)):
        assert raw(**kw) == -22, kw
    torch.cuda.synchronize()
