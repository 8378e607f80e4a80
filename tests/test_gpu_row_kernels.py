"""GPU: direct parity tests of the row, head, embedding and optimizer kernels (csrc/rows.hip, the embedding half of
csrc/layernorm.hip, the flat utilities of csrc/optim.hip), each through the C ABI against the float64 references of
tests/rowref.py, at the shapes where their launchers change code path.

Two kinds of case.  EXACT: integer-valued inputs sized so that every partial sum stays below 2^24 (rowref.EXACT, bound
asserted in tests/test_rowref_cpu.py): float32 addition is then exact in any order, atomics included, and the assertion is
equality with the float64 reference -- one dropped, doubled or misrouted row in 70 000 shows.  REAL: Gaussian inputs
against float64 under rowref.tolerance: 8 x the worst error of the same formula in sequential float32 numpy, a floor of
2 * 2^-24 * sum|terms|, plus one bf16 ulp where the output is bf16.  Pure copies are bit-exact assertions in both kinds.

Every real-valued check prints the kernel's worst error, the float32-numpy evaluation's worst error, their ratio and the
largest share of the tolerance any element used (run with -s).  Worst figures per kernel of the MI355X run that
accompanied this module (245 cases, all passing, 22 s): `ratio` = kernel error / float32-numpy error, of which the rule
allows 8; `share` = the largest fraction of its tolerance any element used.  For the two bf16 outputs the ratio says
nothing (the error IS the bf16 rounding): their share is just below 1 because half a bf16 ulp reaches 2^-8 relative at
the bottom of a binade, which is what the rule's bf16 term grants -- nothing there is slack.

    kernel (output)               ratio   share        kernel (output)               ratio   share
    colsum                        1.62    0.13         embed_ln_bwd (dh)             0.95    0.12
    colsum_rows_f32               1.00    0.13         embed_ln_bwd (dgamma)         2.63    0.33
    colsum_rows_f32_batched       2.02    0.25         embed_ln_bwd (dbeta)          2.80    0.29
    head_fwd                      0.78    0.10         embed_ln_bwd (dtype0)         1.77    0.22
    head_bwd_dx (bf16)            -       0.995        embed_ln_bwd (dword)          1.86    0.11
    head_bwd_dw (dw)              1.00    0.13         embed_ln_bwd (dpos)           1.56    0.10
    head_bwd_dw (db)              1.23    0.15         embed_ln_fwd (mean)           1.00    0.10
    scatter_add_rows_f32          1.00    0.13         embed_ln_fwd (rstd)           1.10    0.11
    wdiff_sum                     1.00    0.13         embed_ln_fwd (y, bf16)        -       0.994
    grad_sqnorm (real-valued, bound 1e-6 relative): worst 4.6e-8

No case needed more than the factor 8; at most 2.8 of it is used (the per-wave row sums of dbeta at 10 560 rows).
"""
import math

import numpy as np
import pytest
import torch

import rowref
from rowref import EXACT, ints

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
WORST = {}   # kernel -> [worst error ratio kernel / float32 numpy, worst share of the tolerance]


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    yield _ops
    print("\n[rowk] worst per kernel (error ratio kernel / float32-numpy, largest share of the tolerance used):")
    for k in sorted(WORST):
        print("[rowk]   %-28s ratio %8.3f   share %6.3f" % (k, WORST[k][0], WORST[k][1]))


def f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def i32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def to_bf16(a):
    """numpy -> (bf16 cpu tensor, its values as float64): the reference sees exactly what the kernel reads"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16()
    return t, t.float().numpy().astype(np.float64)


def padded(t, extra=3, fill=NAN):
    """device copy of t with `extra` rows of `fill` behind it; returns (whole buffer, view of the first rows)"""
    full = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=DEV)
    full[:t.shape[0]] = t.to(DEV)
    return full, full[:t.shape[0]]


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def check_exact(got, ref64):
    """integer-valued case: the kernel's float32 / bf16 output EQUALS the float64 reference"""
    ref = torch.from_numpy(np.ascontiguousarray(ref64, dtype=np.float32))
    assert float(np.abs(ref.double().numpy() - ref64).max() if ref64.size else 0.0) == 0.0   # the reference is a float32 integer
    assert torch.equal(got.detach().float().cpu().reshape(ref.shape), ref)


def check_real(kernel, case, got, ref64, eval32, sum_abs, bf16_out=False, scale=1.0, tol=None):
    ref64 = np.asarray(ref64, np.float64)
    if tol is None:
        tol, err32 = rowref.tolerance(ref64, eval32, sum_abs, bf16_out=bf16_out, scale=scale)
    else:
        err32 = float(np.abs(np.asarray(eval32, np.float64) - ref64).max())
    g = host(got).reshape(ref64.shape)
    assert np.isfinite(g).all()
    diff = np.abs(g - ref64)
    kerr = float(diff.max()) if diff.size else 0.0
    share = float((diff / np.maximum(tol, 1e-300)).max()) if diff.size else 0.0
    ratio = kerr / err32 if err32 > 0 else (0.0 if kerr == 0 else float("inf"))
    print("[rowk] %s %s: kernel_err %.3e  f32_numpy_err %.3e  ratio %.3f  tolerance_share %.3f%s"
          % (kernel, case, kerr, err32, ratio, share, "  (bf16 output)" if bf16_out else ""))
    w = WORST.setdefault(kernel, [0.0, 0.0])
    if not bf16_out and math.isfinite(ratio):
        w[0] = max(w[0], ratio)
    w[1] = max(w[1], share)
    assert (diff <= tol).all(), "%s %s: worst error %.3e, tolerance share %.3f" % (kernel, case, kerr, share)


# ====================================================================== gather / scatter family (pure copies: bit-exact)
def _idx(rng, R, n_src, neg, unique=False):
    idx = rng.permutation(n_src)[:R] if unique else rng.integers(0, n_src, size=R)
    idx = idx.astype(np.int64)
    if neg == "all":
        idx[:] = -1
    elif neg:
        idx[rng.random(R) < 0.25] = -1
    return idx


GATHER_CASES = [(1, 8, True), (3, 504, True), (4, 512, True), (5, 520, True), (8191, 1024, True), (8192, 8, True), (8193, 520, True),
                (70000, 512, True), (70000, 1024, True), (8193, 512, "all"), (5, 1024, False)]


@pytest.mark.parametrize("R,H,neg", GATHER_CASES)
def test_gather_scatter_rows_bf16(ops, R, H, neg):
    rng = np.random.default_rng(R * 131 + H)
    n_src = R + 5
    src = rng.integers(-32768, 32768, size=(n_src, H)).astype(np.int16)          # every bit pattern: a copy must not look at values
    idx = _idx(rng, R, n_src, neg)
    sentinel = np.int16(0x7b7b)
    out = torch.full((R + 2, H), 0, dtype=torch.int16, device=DEV) + int(sentinel)
    ops.gather_rows(torch.from_numpy(src).to(DEV).view(BF16), i32dev(idx), out=out.view(BF16))
    got = out.cpu().numpy()
    assert np.array_equal(got[:R], rowref.gather(src, idx))                      # zeros for idx < 0
    assert (got[R:] == sentinel).all()                                           # nothing behind row R
    # scatter: unique indices; rows that are not indexed, and rows with idx < 0, keep the sentinel
    uidx = _idx(rng, R, n_src, neg, unique=True)
    rows = rng.integers(-32768, 32768, size=(R, H)).astype(np.int16)
    dst = np.full((n_src, H), sentinel, np.int16)
    d = torch.from_numpy(dst).to(DEV)
    ops.scatter_rows(torch.from_numpy(rows).to(DEV).view(BF16), i32dev(uidx), d.view(BF16))
    assert np.array_equal(d.cpu().numpy(), rowref.scatter(dst, rows, uidx))


@pytest.mark.parametrize("R,H,ld_src,ld_out,col", [(5, 8, 16, 24, 8), (8193, 504, 512, 840, 328), (70000, 512, 520, 520, 0),
                                                   (3, 1024, 1032, 1360, 328), (4, 520, 528, 536, 8), (8192, 8, 8, 16, 0)])
def test_gather_rows_ld(ops, R, H, ld_src, ld_out, col):
    rng = np.random.default_rng(R + H)
    n_src = R + 3
    src = rng.integers(-32768, 32768, size=(n_src, ld_src)).astype(np.int16)
    idx = _idx(rng, R, n_src, True)
    sentinel = np.int16(0x7b7b)
    out = torch.zeros((R + 2, ld_out), dtype=torch.int16, device=DEV) + int(sentinel)
    ops.gather_rows_into(torch.from_numpy(src).to(DEV).view(BF16), i32dev(idx), out.view(BF16), col, H)
    got = out.cpu().numpy()
    assert np.array_equal(got[:R, col:col + H], rowref.gather(src[:, :H], idx))
    keep = np.ones(got.shape, bool)
    keep[:R, col:col + H] = False
    assert (got[keep] == sentinel).all()                                         # other columns and the rows behind R


@pytest.mark.parametrize("R,W", [(1, 29), (5, 64), (8193, 29), (70000, 64), (70000, 29), (8193, 64)])
def test_gather_rows_f32(ops, R, W):
    rng = np.random.default_rng(R + W)
    n_src = R + 3
    src = rng.integers(-2 ** 31, 2 ** 31, size=(n_src, W)).astype(np.int32)
    for neg in (True, "all"):
        idx = _idx(rng, R, n_src, neg)
        got = ops.gather_rows_f32(torch.from_numpy(src).to(DEV).view(F32), i32dev(idx))
        assert np.array_equal(got.view(I32).cpu().numpy(), rowref.gather(src, idx))


@pytest.mark.parametrize("R,W", [(1, 4), (5, 28), (8193, 1024), (70000, 28), (8192, 4), (3, 1024)])
def test_scatter_rows_f32(ops, R, W):
    rng = np.random.default_rng(R + W)
    n_dst = R + 7
    rows = rng.integers(-2 ** 31, 2 ** 31, size=(R, W)).astype(np.int32)
    for neg in (True, "all"):
        idx = _idx(rng, R, n_dst, neg, unique=True)
        dst = np.full((n_dst, W), 0x7b7b7b7b, np.int32)
        d = torch.from_numpy(dst).to(DEV)
        ops.scatter_rows_f32(torch.from_numpy(rows).to(DEV).view(F32), i32dev(idx), d.view(F32))
        assert np.array_equal(d.cpu().numpy(), rowref.scatter(dst, rows, idx))


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("R,W", [(1, 29), (5, 64), (8193, 29), (70000, 64), (70000, 29), (4, 64)])
def test_scatter_add_rows_f32(ops, R, W, kind):
    rng = np.random.default_rng(R + W)
    n_dst = R + 7
    idx = _idx(rng, R, n_dst, True, unique=True)                                 # unique by contract: a plain read-modify-write
    if kind == "exact":
        k, terms, start = EXACT["scatter_add"]
        rows, dst = ints(rng, k["rows"], (R, W)), ints(rng, start, (n_dst, W))
    else:
        rows, dst = rng.standard_normal((R, W)), rng.standard_normal((n_dst, W))
    rows, dst = rows.astype(np.float32), dst.astype(np.float32)
    d = f32dev(dst)
    ops.scatter_add_rows_f32(f32dev(rows), i32dev(idx), d)
    ref = rowref.scatter_add(dst, rows, idx)
    if kind == "exact":
        check_exact(d, ref)
    else:
        ev = dst.copy()
        ev[idx[idx >= 0]] += rows[idx >= 0]
        check_real("scatter_add_rows_f32", "R=%d W=%d" % (R, W), d, ref, ev, rowref.scatter_add(np.abs(dst), np.abs(rows), idx))
    untouched = np.ones(n_dst, bool)
    untouched[idx[idx >= 0]] = False
    assert np.array_equal(bits(d).numpy()[untouched], dst.view(np.int32)[untouched])


# ====================================================================== emission head
HEAD_FWD_CASES = [(1, 128, 29), (64, 768, 29), (511, 1024, 1), (512, 128, 21), (513, 768, 32), (512, 1024, 64), (513, 1024, 64),
                  (8193, 1024, 33), (70000, 128, 29),                               # rt kernel up to 512 rows, row kernel beyond
                  (64, 1032, 29), (513, 2048, 33), (1030, 8192, 21), (8193, 1032, 64), (1, 8192, 1)]   # wide kernel (H > 1024)


def _head_inputs(rng, kind, R, H, T):
    if kind == "exact":
        k = EXACT["head_fwd"][0]
        assert H <= EXACT["head_fwd"][1]
        x, w, b = ints(rng, k["x"], (R, H)), ints(rng, k["w"], (T, H)), ints(rng, k["b"], (T,))
    else:
        x, w, b = rng.standard_normal((R, H)), 0.05 * rng.standard_normal((T, H)), 0.1 * rng.standard_normal(T)
    xb, x64 = to_bf16(x)
    return xb, x64, w.astype(np.float32), b.astype(np.float32)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("R,H,T", HEAD_FWD_CASES)
def test_head_fwd(ops, R, H, T, kind):
    rng = np.random.default_rng(R * 7 + H + T)
    xb, x64, w, b = _head_inputs(rng, kind, R, H, T)
    full, x = padded(xb)                                                         # NaN rows behind R: a kernel that reads them shows
    out = ops.head_fwd(x, f32dev(w), f32dev(b))
    assert out.shape == (R, T) and bool(torch.isfinite(out).all())
    ref = rowref.head_fwd(x64, w, b)
    if kind == "exact":
        check_exact(out, ref)
    else:
        ev = rowref.seq_dot32(x64, w) + b
        check_real("head_fwd", "R=%d H=%d T=%d" % (R, H, T), out, ref, ev, np.abs(x64) @ np.abs(w.astype(np.float64)).T + np.abs(b))
    del full, x, out
    torch.cuda.empty_cache()


def test_head_fwd_rt_kernel_same_bits_as_row_kernel(ops):
    """csrc/rows.hip: head_fwd_rt_kernel (R <= 512) computes `the same bits` as head_fwd_kernel (R > 512)"""
    rng = np.random.default_rng(1)
    for H, T in ((768, 29), (1024, 64), (128, 1)):
        xb, _, w, b = _head_inputs(rng, "real", 600, H, T)
        x = xb.to(DEV)
        wd, bd = f32dev(w), f32dev(b)
        rows = ops.head_fwd(x, wd, bd)                                           # 600 rows: the row kernel
        rt = ops.head_fwd(x[:512].contiguous(), wd, bd)                          # 512 rows: the (row, tag) kernel
        assert torch.equal(rows[:512], rt)


def test_head_zero_rows_touch_nothing(ops):
    H, T = 128, 29
    x = torch.zeros((0, H), dtype=BF16, device=DEV)
    w = torch.ones((T, H), dtype=F32, device=DEV)
    b = torch.ones(T, dtype=F32, device=DEV)
    assert ops.head_fwd(x, w, b).shape == (0, T)
    dw = torch.full((T, H), 2.5, dtype=F32, device=DEV)
    db = torch.full((T,), -1.5, dtype=F32, device=DEV)
    dx = ops.head_bwd(torch.zeros((0, T), dtype=F32, device=DEV), x, w, dw, db)
    torch.cuda.synchronize()
    assert dx.shape == (0, H) and bool((dw == 2.5).all()) and bool((db == -1.5).all())


HEAD_BWD_CASES = [(1, 128, 29), (64, 768, 32), (511, 1024, 29), (512, 128, 32), (513, 768, 29), (513, 1024, 32), (512, 1024, 29),
                  (8193, 1024, 29), (70000, 128, 32),                              # <32,16> up to 512 rows, <32,64> beyond
                  (64, 128, 33), (512, 768, 48), (513, 1024, 64), (8193, 264, 64), (1, 8, 64),   # <64,64>: T in 33..64
                  (300, 8, 29), (300, 264, 48), (577, 264, 21)]                    # a partly filled 256-column block of dw


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("R,H,T", HEAD_BWD_CASES)
def test_head_bwd(ops, R, H, T, kind):
    rng = np.random.default_rng(R * 3 + H + T)
    if kind == "exact":
        kx, kw = EXACT["head_bwd_dw"][0], EXACT["head_bwd_dx"][0]
        assert R <= EXACT["head_bwd_dw"][1] and T <= EXACT["head_bwd_dx"][1] and kx["de"] == kw["de"]
        de, x, w = ints(rng, kx["de"], (R, T)), ints(rng, kx["x"], (R, H)), ints(rng, kw["w"], (T, H))
        dw0, db0 = ints(rng, EXACT["head_bwd_dw"][2], (T, H)), ints(rng, EXACT["head_bwd_db"][2], (T,))
    else:
        de, x, w = 0.1 * rng.standard_normal((R, T)), rng.standard_normal((R, H)), 0.05 * rng.standard_normal((T, H))
        dw0, db0 = rng.standard_normal((T, H)), rng.standard_normal(T)
    xb, x64 = to_bf16(x)
    de, w, dw0, db0 = (a.astype(np.float32) for a in (de, w, dw0, db0))
    xfull, xd = padded(xb)
    defull, ded = padded(torch.from_numpy(de))
    dw, db = f32dev(dw0), f32dev(db0)                                            # accumulated INTO: not zero
    dx = ops.head_bwd(ded, xd, f32dev(w), dw, db)
    rdx, rdw, rdb = rowref.head_bwd(de, x64, w)
    rdw, rdb = rdw + dw0, rdb + db0
    case = "R=%d H=%d T=%d" % (R, H, T)
    if kind == "exact":
        check_exact(dx, rdx)
        check_exact(dw, rdw)
        check_exact(db, rdb)
    else:
        a64 = np.abs(de.astype(np.float64))
        check_real("head_bwd_dx", case, dx, rdx, rowref.seq_dot32(de, w.T), a64 @ np.abs(w.astype(np.float64)), bf16_out=True)
        check_real("head_bwd_dw", case, dw, rdw, rowref.seq_dot32(de.T, x64.T) + dw0, a64.T @ np.abs(x64) + np.abs(dw0))
        check_real("head_bwd_dw(db)", case, db, rdb, rowref.seq_sum32(de, 0) + db0, a64.sum(0) + np.abs(db0))
    del xfull, defull
    torch.cuda.empty_cache()


# ====================================================================== column sums
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("M,N", [(1, 8), (4, 504), (127, 512), (128, 520), (129, 4096), (300, 512), (300, 4096), (65536, 520),
                                 (65536, 8), (4, 4096)])
def test_colsum(ops, M, N, kind):
    rng = np.random.default_rng(M + N)
    if kind == "exact":
        k, terms, start = EXACT["colsum"]
        assert M <= terms
        x, out0 = ints(rng, k["x"], (M, N)), ints(rng, start, (N,))
    else:
        x, out0 = rng.standard_normal((M, N)), rng.standard_normal(N)
    xb, x64 = to_bf16(x)
    out0 = out0.astype(np.float32)
    full, _ = padded(xb, extra=5)                                                # M= smaller than the buffer, NaN behind it
    out = f32dev(out0)                                                           # accumulates
    ops.colsum(full, out, M=M)
    ref = rowref.colsum(x64) + out0
    if kind == "exact":
        check_exact(out, ref)
    else:
        check_real("colsum", "M=%d N=%d" % (M, N), out, ref, rowref.seq_sum32(x64, 0) + out0, np.abs(x64).sum(0) + np.abs(out0))
    del full
    torch.cuda.empty_cache()


def _ws_inputs(rng, kind, rows, N):
    if kind == "exact":
        k, terms, start = EXACT["colsum_rows"]
        assert rows <= terms
        return ints(rng, k["ws"], (rows, N)).astype(np.float32), ints(rng, start, (N,)).astype(np.float32)
    return rng.standard_normal((rows, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("rows,N", [(1, 8), (3, 256), (32, 264), (64, 4096), (72, 256), (80, 264), (128, 8), (128, 4096), (1024, 4096),
                                    (1024, 264), (80, 8)])
def test_colsum_rows_f32(ops, rows, N, kind):
    """64 and 72 rows take the single pass, 80 / 128 / 1024 (more than 64, a multiple of 16) the two-pass fold every full-size
    step uses.  The two-pass route folds IN PLACE: it overwrites `ws`, so only `out` is asserted (and each call gets a copy)."""
    rng = np.random.default_rng(rows + N)
    ws, out0 = _ws_inputs(rng, kind, rows, N)
    res = []
    for _ in range(2):
        full, _v = padded(torch.from_numpy(ws))                                  # NaN rows behind `rows`
        out = f32dev(out0)
        ops.colsum_rows_f32(full, rows, out)
        torch.cuda.synchronize()
        res.append(out)
    assert torch.equal(res[0], res[1])                                           # deterministic
    ref = ws.astype(np.float64).sum(0) + out0
    if kind == "exact":
        check_exact(res[0], ref)
    else:
        check_real("colsum_rows_f32", "rows=%d N=%d" % (rows, N), res[0], ref, rowref.seq_sum32(ws, 0) + out0,
                   np.abs(ws.astype(np.float64)).sum(0) + np.abs(out0))


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("items,N", [(1, 264), (2, 4096), (64, 264), (64, 8), (3, 256)])
def test_colsum_rows_f32_batched(ops, items, N, kind):
    """up to 64 workspaces with different row counts in one launch; each item has the bits of the single-pass call on the same
    data (`Same summation order per column`, csrc/rows.hip) -- so the row counts here are ones the single call folds in ONE pass
    (at most 64, or not a multiple of 16)."""
    rng = np.random.default_rng(items + N)
    counts = [1, 1000, 3, 64, 100, 72][:items] if items <= 6 else [1 + (7 * i) % 63 for i in range(items - 2)] + [1000, 200]
    assert all(c <= 64 or c % 16 for c in counts)
    data = [_ws_inputs(rng, kind, c, N) for c in counts]
    wss = [f32dev(w) for w, _ in data]
    outs = [f32dev(o) for _, o in data]
    ops.colsum_rows_f32_batched([(w, o, c) for w, o, c in zip(wss, outs, counts)], N)
    torch.cuda.synchronize()
    for (w, o0), wd, od, c in zip(data, wss, outs, counts):
        assert np.array_equal(bits(wd).numpy(), w.view(np.int32))                # the batched fold leaves ws as it is
        single = f32dev(o0)
        ops.colsum_rows_f32(wd, c, single)
        assert torch.equal(od, single)
        ref = w.astype(np.float64).sum(0) + o0
        if kind == "exact":
            check_exact(od, ref)
        else:
            check_real("colsum_rows_f32_batched", "items=%d rows=%d N=%d" % (items, c, N), od, ref, rowref.seq_sum32(w, 0) + o0,
                       np.abs(w.astype(np.float64)).sum(0) + np.abs(o0))


# ====================================================================== embeddings + LayerNorm
V_WORD, V_POS = 2048, 514


def _tables(rng, H):
    return dict(word=(0.1 * rng.standard_normal((V_WORD, H))).astype(np.float32), pos=(0.05 * rng.standard_normal((V_POS, H))).astype(np.float32),
                type0=(0.02 * rng.standard_normal(H)).astype(np.float32), gamma=(1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32),
                beta=(0.05 * rng.standard_normal(H)).astype(np.float32))


def _mult(ops, M, H, drop):
    """the dropout multiplier of a hidden-state site, from the library's own mask materialiser (as tests/selftest.py does)"""
    if not drop[1]:
        return None
    return ops.dropout_mask(1, M, H, drop[0], drop[1])[0].cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("M,H,eps,p", [(1, 128, 1e-5, 0.0), (3, 768, 1e-12, 0.0), (5, 1024, 1e-5, 0.1), (4096, 768, 1e-5, 0.1),
                                       (4097, 1024, 1e-12, 0.0), (33 * 320, 128, 1e-12, 0.1), (33 * 320, 1024, 1e-5, 0.0),
                                       (4097, 128, 1e-5, 0.0), (5, 768, 1e-12, 0.1)])
def test_embed_ln_fwd(ops, M, H, eps, p):
    rng = np.random.default_rng(M + H)
    t = _tables(rng, H)
    ids = rng.integers(0, V_WORD, size=M)
    pids = rng.integers(0, V_POS, size=M)
    drop = (4321 + M, ops.drop_thresh(p)) if p else ops.NO_DROP
    h0 = torch.full((M + 2, H), NAN, dtype=BF16, device=DEV)
    y = torch.full((M + 2, H), NAN, dtype=BF16, device=DEV)
    mean = torch.full((M + 2,), NAN, dtype=F32, device=DEV)
    rstd = torch.full((M + 2,), NAN, dtype=F32, device=DEV)
    ops.embed_ln_fwd(i32dev(ids), i32dev(pids), f32dev(t["word"]), f32dev(t["pos"]), f32dev(t["type0"]), f32dev(t["gamma"]),
                     f32dev(t["beta"]), eps, h0, y, mean, rstd, drop=drop)
    torch.cuda.synchronize()
    for buf in (h0, y, mean, rstd):                                              # nothing behind row M
        assert bool(torch.isnan(buf[M:]).all())
    # h0 = bf16((word + pos) + type0): the same association in float32, bit-exact
    tw, tp, tt = (torch.from_numpy(t[k]) for k in ("word", "pos", "type0"))
    h0_ref = ((tw[torch.from_numpy(ids)] + tp[torch.from_numpy(pids)]) + tt).bfloat16()
    assert torch.equal(bits(h0[:M]), bits(h0_ref))
    hq = h0_ref.float().numpy()                                                  # what is stored is what is normalised
    mult = _mult(ops, M, H, drop)
    _, ry, rmean, rrstd = rowref.embed_ln_fwd(ids, pids, t["word"], t["pos"], t["type0"], t["gamma"], t["beta"], eps, mult=mult, h0=hq)
    # the same in sequential float32
    m32 = rowref.seq_sum32(hq, 1) / np.float32(H)
    d32 = hq - m32[:, None]
    r32 = (np.float32(1.0) / np.sqrt(rowref.seq_sum32(d32 * d32, 1) / np.float32(H) + np.float32(eps))).astype(np.float32)
    y32 = d32 * r32[:, None] * t["gamma"] + t["beta"]
    if mult is not None:
        y32 = y32 * mult.astype(np.float32)
    case = "M=%d H=%d eps=%g p=%g" % (M, H, eps, p)
    h64 = hq.astype(np.float64)
    check_real("embed_ln_fwd(mean)", case, mean[:M], rmean, m32, np.abs(h64).sum(1) / H)
    # rstd is not a sum: the value passes four roundings (the variance sum, / H + eps, the root, the reciprocal), each up to
    # 2^-24 relative, and the hardware's reciprocal square root is good to one ulp: the floor counts 4 |rstd| as its `terms`
    check_real("embed_ln_fwd(rstd)", case, rstd[:M], rrstd, r32, 4.0 * np.abs(rrstd))
    terms = np.abs((h64 - rmean[:, None]) * rrstd[:, None] * t["gamma"]) + np.abs(t["beta"])
    if mult is not None:
        terms = terms * mult
    check_real("embed_ln_fwd(y)", case, y[:M], ry, y32, terms, bf16_out=True)


def _id_pattern(rng, pattern):
    """-> ids, pos_ids (int64 [M])"""
    kind = pattern[0]
    if kind == "distinct":                       # every word row at most once: dword[ids[r]] IS dh[r]
        M = pattern[1]
        return rng.permutation(V_WORD)[:M], rng.integers(0, V_POS, size=M)
    if kind == "equal":                          # M atomics on one word row and one position row
        M = pattern[1]
        return np.full(M, 7), np.full(M, 5)
    if kind == "randpos":                        # positions at random: every row flushes its position run
        M = pattern[1]
        return rng.integers(0, V_WORD // 4, size=M), rng.integers(0, V_POS, size=M)
    B, S = pattern[1], pattern[2]                # the engine's pattern: ragged sentences, positions 2..len+1, padding id 1 / position 1
    ids = np.ones((B, S), np.int64)
    pos = np.ones((B, S), np.int64)
    for b in range(B):
        n = S if b == 0 else int(rng.integers(max(1, S // 2), S + 1))
        ids[b, :n] = rng.integers(3, V_WORD // 2, size=n)
        pos[b, :n] = np.arange(2, n + 2)
    return ids.reshape(-1), pos.reshape(-1)


# 320 does not divide the 4096-wave grid (a wave's successive rows change position every time), 512 does, (5, 7) leaves waves
# without any row; 4097 equal ids: one wave takes two rows
EMBED_BWD_CASES = [(("distinct", 2000), 768, 0.1), (("equal", 4097), 128, 0.0), (("engine", 2, 64), 128, 0.0), (("engine", 8, 512), 1024, 0.1),
                   (("engine", 33, 320), 768, 0.0), (("engine", 5, 7), 128, 0.1), (("randpos", 33 * 320), 128, 0.0),
                   (("distinct", 5), 1024, 0.0)]


@pytest.mark.parametrize("route", ["plain", "row_flags", "deferred"])
@pytest.mark.parametrize("pattern,H,p", EMBED_BWD_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_embed_ln_bwd(ops, pattern, H, p, route):
    rng = np.random.default_rng(H + len(pattern[0]) + pattern[1])
    ids, pids = _id_pattern(rng, pattern)
    M = ids.shape[0]
    gamma = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    h0b, h64 = to_bf16(0.15 * rng.standard_normal((M, H)))
    dyb, dy64 = to_bf16(0.01 * rng.standard_normal((M, H)))
    mean = h64.mean(1).astype(np.float32)                                        # the statistics are INPUTS of the backward pass:
    rstd = (1.0 / np.sqrt(h64.var(1) + 1e-5)).astype(np.float32)                 # kernel and reference read the same float32 values
    drop = (99 + M, ops.drop_thresh(p)) if p else ops.NO_DROP
    mult = _mult(ops, M, H, drop)
    ref = rowref.embed_ln_bwd(dy64, h64, mean, rstd, gamma, ids, pids, V_WORD, V_POS, mult=mult)

    pre = {k: rng.standard_normal(H).astype(np.float32) for k in ("dgamma", "dbeta", "dtype0")}      # accumulated into
    dgamma, dbeta, dtype0 = (f32dev(pre[k]) for k in ("dgamma", "dbeta", "dtype0"))
    dword = torch.zeros((V_WORD, H), dtype=F32, device=DEV)
    dpos = torch.zeros((V_POS, H), dtype=F32, device=DEV)
    flags0 = (rng.random(V_WORD) < 0.2).astype(np.uint8)                         # some rows already live (1), the rest 0
    flags = torch.from_numpy(flags0).to(DEV) if route == "row_flags" else None
    args = (dyb.to(DEV), h0b.to(DEV), f32dev(mean), f32dev(rstd), f32dev(gamma), i32dev(ids), i32dev(pids), dgamma, dbeta, dword, dpos, dtype0)
    if route == "deferred":
        nb = ops.ln_bwd_blocks(M)
        ws = torch.full((nb * 3 * H + 16,), NAN, dtype=F32, device=DEV)
        ops.embed_ln_bwd(*args, drop=drop, defer_ws=ws)
        torch.cuda.synchronize()
        for k, buf in (("dgamma", dgamma), ("dbeta", dbeta), ("dtype0", dtype0)):                  # untouched until the batched reduce
            assert np.array_equal(bits(buf).numpy(), pre[k].view(np.int32))
        assert bool(torch.isnan(ws[nb * 3 * H:]).all()) and bool(torch.isfinite(ws[:nb * 3 * H]).all())
        ops.ln_colreduce_batched([(ws, dgamma, dbeta, dtype0, nb)], H)
    else:
        ops.embed_ln_bwd(*args, drop=drop, row_flags=flags)
    torch.cuda.synchronize()

    # the same formula in sequential float32
    g32 = gamma
    d32 = dy64.astype(np.float32) * (mult.astype(np.float32) if mult is not None else np.float32(1.0))
    xh32 = (h64.astype(np.float32) - mean[:, None]) * rstd[:, None]
    gd32 = d32 * g32
    s1 = rowref.seq_sum32(gd32, 1) / np.float32(H)
    s2 = rowref.seq_sum32(gd32 * xh32, 1) / np.float32(H)
    dh32 = rstd[:, None] * (gd32 - s1[:, None] - xh32 * s2[:, None])
    d64 = dy64 * (mult if mult is not None else 1.0)
    xh64 = (h64 - mean.astype(np.float64)[:, None]) * rstd.astype(np.float64)[:, None]
    g64 = d64 * gamma
    dh_terms = rstd.astype(np.float64)[:, None] * (np.abs(g64) + np.abs(g64).mean(1)[:, None] + np.abs(xh64) * np.abs(g64 * xh64).mean(1)[:, None])
    tol_dh, err_dh = rowref.tolerance(ref["dh"], dh32, dh_terms)                 # per element of dh [M, H]
    case = "%s H=%d p=%g %s" % ("-".join(map(str, pattern)), H, p, route)

    check_real("embed_ln_bwd(dgamma)", case, dgamma, ref["dgamma"] + pre["dgamma"], rowref.seq_sum32(d32 * xh32, 0) + pre["dgamma"],
               np.abs(d64 * xh64).sum(0) + np.abs(pre["dgamma"]))
    check_real("embed_ln_bwd(dbeta)", case, dbeta, ref["dbeta"] + pre["dbeta"], rowref.seq_sum32(d32, 0) + pre["dbeta"],
               np.abs(d64).sum(0) + np.abs(pre["dbeta"]))
    check_real("embed_ln_bwd(dtype0)", case, dtype0, ref["dtype0"] + pre["dtype0"], rowref.seq_sum32(dh32, 0) + pre["dtype0"],
               np.abs(ref["dh"]).sum(0) + np.abs(pre["dtype0"]))
    # every row of dword / dpos against the float64 scatter-add of the float64 dh: a row named k times carries k rows' worth of
    # the dh tolerance (the scatter-add of tol_dh) plus the rounding of adding them up
    absdh = np.abs(ref["dh"])
    for name, buf, index, nrow in (("dword", dword, ids, V_WORD), ("dpos", dpos, pids, V_POS)):
        tol = rowref.scatter_add(np.zeros((nrow, H)), tol_dh, index) + 2.0 * rowref.F32_EPS * rowref.scatter_add(np.zeros((nrow, H)), absdh, index)
        ev = np.zeros((nrow, H), np.float32)
        np.add.at(ev, index, dh32)
        check_real("embed_ln_bwd(%s)" % name, case, buf, ref[name], ev, None, tol=tol)
        named = np.zeros(nrow, bool)
        named[index] = True
        assert not bits(buf).numpy()[~named].any()                               # rows no id names stay exactly zero (+0.0)
    if pattern[0] == "distinct":                                                 # dh itself: with distinct ids dword[ids[r]] is dh[r]
        check_real("embed_ln_bwd(dh)", case, dword[torch.from_numpy(ids).to(DEV)], ref["dh"], dh32, dh_terms)
    # conservation: the three scatter targets hold the same total
    tol_sum = 2.0 * (tol_dh.sum(0) + 2.0 * rowref.F32_EPS * absdh.sum(0))
    tot_w, tot_p, tot_t = host(dword).sum(0), host(dpos).sum(0), host(dtype0) - pre["dtype0"].astype(np.float64)
    # (dtype0 was added to a pre-filled value of order 1: its own rounding, 2^-24 of that value, is part of the comparison)
    tol_t = tol_sum + 2.0 * rowref.F32_EPS * (np.abs(pre["dtype0"]) + np.abs(tot_t))
    assert (np.abs(tot_w - tot_p) <= tol_sum).all()
    assert (np.abs(tot_w - tot_t) <= tol_t).all() and (np.abs(tot_p - tot_t) <= tol_t).all()
    if route == "row_flags":                                                     # exactly the named rows become 3, all others keep their value
        assert np.array_equal(flags.cpu().numpy(), np.where(ref["flags"] == 3, 3, flags0).astype(np.uint8))


# ====================================================================== AdamW
def _sq_ws(ops):
    from kbner import lib as L
    return torch.zeros(L.load().kbner_sqnorm_ws_floats(), dtype=F32, device=DEV)


# check_adamw's tolerance (tests/selftest.py) on p.  m and v have none there; theirs comes from the kernel's float32 constants:
# 1.0f - 0.999f is 1.00004673e-3 (4.7e-5 above 1 - 0.999), 1.0f - 0.9f is 2.4e-7 above 0.1, so v may differ from the float64
# formula by 5e-5 relative and m by 3e-7 (+ 2^-24 per operation): 2e-4 and 1e-5 of the largest value
P_ABS, M_REL, V_REL = 2e-6, 1e-5, 2e-4


def _adam_close(pd, md, vd, p, m, v):
    assert float(np.abs(host(pd) - p).max()) < P_ABS
    assert float(np.abs(host(md) - m).max()) <= M_REL * float(np.abs(m).max())
    assert float(np.abs(host(vd) - v).max()) <= V_REL * float(np.abs(v).max())


@pytest.mark.parametrize("n", [4, 4092, 4096, 4100, 4160, 1052672, 8192 * 4096 + 4 * 1028])
def test_adamw_three_steps(ops, n):
    """three steps with the clip active in the second; the last size has more 16-KiB chunks than the 8192 workgroups of the
    grid (the chunk loop strides) and a ragged last chunk"""
    rng = np.random.default_rng(n % 1000)
    p = rng.standard_normal(n)
    m, v = np.zeros(n), np.zeros(n)
    pd = f32dev(p)
    p = pd.cpu().numpy().astype(np.float64)
    md, vd = torch.zeros(n, dtype=F32, device=DEV), torch.zeros(n, dtype=F32, device=DEV)
    sh = torch.zeros(n, dtype=BF16, device=DEV)
    ws, nsq = _sq_ws(ops), torch.zeros(1, dtype=F32, device=DEV)
    lr = 1e-3
    for step in range(1, 4):
        # norm 3 sqrt(n) in the second step (clipped), at most 2 in the others
        g = (rng.standard_normal(n) * (3.0 if step == 2 else min(0.01, 2.0 / math.sqrt(n)))).astype(np.float32)
        gd = f32dev(g)
        ops.grad_sqnorm(gd, ws, nsq)
        bc = math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
        ops.adamw(pd, gd, md, vd, sh, n, lr * bc, 0.0, 0.9, 0.999, 1e-6, nsq, 5.0, 1.0, True)
        torch.cuda.synchronize()
        exact_sq = rowref.sqnorm(g)
        assert (math.sqrt(exact_sq) > 5.0) == (step == 2) or n < 64            # the clip is active in step 2 (not for a handful of values)
        p, m, v, _ = rowref.adamw_hf(p, g, m, v, np.float32(lr * bc), 0.0, 0.9, 0.999, 1e-6, exact_sq, 5.0, 1.0)
        _adam_close(pd, md, vd, p, m, v)
        assert not bits(gd).numpy().any()                                        # zeroed (+0.0)
        assert abs(float(nsq) - exact_sq) <= 1e-6 * exact_sq
        assert torch.equal(bits(sh), bits(pd.cpu().bfloat16()))                  # the shadow is bf16 of the kernel's own p, bit for bit
        del gd
    del pd, md, vd, sh
    torch.cuda.empty_cache()


@pytest.mark.parametrize("variant", ["weight_decay", "shadow_0", "shadow_4", "shadow_n-4", "keep_grad", "grad_scale", "no_norm"])
@pytest.mark.parametrize("n", [4160, 1052672])
def test_adamw_variants(ops, n, variant):
    rng = np.random.default_rng(n % 1000 + len(variant))
    lr, step = 1e-3, 2
    step_size = float(np.float32(lr * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)))
    p, m = rng.standard_normal(n).astype(np.float32), (0.01 * rng.standard_normal(n)).astype(np.float32)
    v = (1e-4 * rng.random(n)).astype(np.float32)
    # norm far above 5: the clip is active where a norm is given -- except for grad_scale, which a clipped step cannot show
    # (the coefficient divides by the scaled norm: the product is 5 / norm whatever the scale), so there the norm is about 1
    g = ((1.0 / math.sqrt(n) if variant == "grad_scale" else 3.0) * rng.standard_normal(n)).astype(np.float32)
    lr_wd = float(np.float32(1e-2 * lr)) if variant == "weight_decay" else 0.0
    n_shadow = {"shadow_0": 0, "shadow_4": 4, "shadow_n-4": n - 4}.get(variant, n)
    zero_grad = variant != "keep_grad"
    scale = 0.25 if variant == "grad_scale" else 1.0
    pd, gd, md, vd = f32dev(p), f32dev(g), f32dev(m), f32dev(v)
    sentinel = 0x7b7b
    sh = torch.full((n,), sentinel, dtype=torch.int16, device=DEV)
    exact_sq = rowref.sqnorm(g)
    nsq = None if variant == "no_norm" else f32dev(np.array([exact_sq]))
    ops.adamw(pd, gd, md, vd, sh.view(BF16), n_shadow, step_size, lr_wd, 0.9, 0.999, 1e-6, nsq, 5.0, scale, zero_grad)
    torch.cuda.synchronize()
    rp, rm, rv, _ = rowref.adamw_hf(p, g, m, v, step_size, lr_wd, 0.9, 0.999, 1e-6, None if nsq is None else float(np.float32(exact_sq)), 5.0, scale)
    _adam_close(pd, md, vd, rp, rm, rv)
    if variant == "weight_decay":                                                # the decay is visible above the tolerance
        assert float(np.abs(rp - rowref.adamw_hf(p, g, m, v, step_size, 0.0, gnorm_sq=exact_sq)[0]).max()) > 10 * P_ABS
    if variant == "grad_scale":
        assert float(np.abs(rm - rowref.adamw_hf(p, g, m, v, step_size, 0.0, gnorm_sq=exact_sq)[1]).max()) > 100 * M_REL * float(np.abs(rm).max())
    if zero_grad:
        assert not bits(gd).numpy().any()
    else:
        assert np.array_equal(bits(gd).numpy(), g.view(np.int32))                # g unchanged bit for bit
    shc = sh.cpu()
    assert torch.equal(shc[:n_shadow], bits(pd.cpu().bfloat16())[:n_shadow])
    assert bool((shc[n_shadow:] == sentinel).all())                              # nothing behind n_shadow


# ====================================================================== grad_sqnorm
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("n", [4, 1020, 4160, 2048 * 1024 + 4, 40000004])
def test_grad_sqnorm(ops, n, kind, accumulate):
    """2048 * 1024 + 4 is the first size past one float4 per thread of the capped grid (the stride loop); 40 000 004 walks it 20 times"""
    rng = np.random.default_rng(n % 997)
    if kind == "exact":
        k, terms, _ = EXACT["sqnorm_block"]
        assert (n // 4 + 2048 * 256 - 1) // (2048 * 256) * 256 * 4 <= terms      # the floats one workgroup adds up
        g = rng.integers(-k["g"], k["g"] + 1, size=n).astype(np.float32)
    else:
        g = rng.standard_normal(n).astype(np.float32)
    out0 = np.float32(5.0)
    out = f32dev(np.array([out0]))
    ops.grad_sqnorm(f32dev(g), _sq_ws(ops), out, accumulate=accumulate)
    torch.cuda.synchronize()
    exact = rowref.sqnorm(g) + (float(out0) if accumulate else 0.0)
    if kind == "exact":                                                          # exact partials, final sum in double: one rounding
        assert float(out) == float(np.float32(exact))
    else:                                                                        # float32 per-thread partials of n / (2048 * 256) terms
        print("[rowk] grad_sqnorm n=%d accumulate=%d: relative error %.3e" % (n, accumulate, abs(float(out) - exact) / exact))
        assert abs(float(out) - exact) <= 1e-6 * exact


# ====================================================================== conversions
def _f32_bits(u):
    return torch.from_numpy(np.ascontiguousarray(u, dtype=np.uint32).view(np.int32)).view(F32)


def _to_bf16_dev(ops, x):
    y = torch.full((x.numel() + 4,), 0x7b7b, dtype=torch.int16, device=DEV)
    ops.f32_to_bf16(x.to(DEV), y.view(BF16)[:x.numel()])
    torch.cuda.synchronize()
    assert bool((y[x.numel():] == 0x7b7b).all())
    return y[:x.numel()].cpu()


def test_f32_to_bf16(ops):
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal(1 << 20).astype(np.float32) * np.exp(rng.uniform(-20, 20, 1 << 20)).astype(np.float32))
    assert torch.equal(_to_bf16_dev(ops, x), bits(x.bfloat16()))
    # every tie pattern: low half exactly 0x8000 under an even and an odd upper half (all normal exponents, both signs)
    upper = np.arange(0x0080, 0x7f80, dtype=np.uint32)
    upper = np.concatenate([upper, upper | 0x8000])
    assert (upper & 1).any() and not (upper & 1).all()
    ties = _f32_bits((upper << 16) | 0x8000)
    assert torch.equal(_to_bf16_dev(ops, ties), bits(ties.bfloat16()))
    near = _f32_bits(np.concatenate([(upper << 16) | 0x7fff, (upper << 16) | 0x8001]))      # one float32 ulp either side of a tie
    assert torch.equal(_to_bf16_dev(ops, near), bits(near.bfloat16()))
    # +-0, +-inf, the largest finite values (round up to inf), and an exact tie below inf with an odd upper half
    special = _f32_bits(np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0xff7f8000], np.uint32))
    got = _to_bf16_dev(ops, special)
    assert torch.equal(got, bits(special.bfloat16()))
    assert got.numpy().view(np.uint16).tolist() == [0x0000, 0x8000, 0x7f80, 0xff80, 0x7f80, 0xff80, 0x7f80, 0xff80]
    # NaN stays NaN, also when its payload lies in the low half only (a bare truncation would turn it into inf)
    nans = _f32_bits(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7f80ffff, 0x7fffffff, 0x7fa00000, 0x7f808000], np.uint32))
    assert bool(torch.isnan(_to_bf16_dev(ops, nans).view(BF16).float()).all())
    # subnormal inputs: torch's value (round to nearest even into bf16's subnormals) or flushed to a zero of the same sign.
    # What the MI355X does: it keeps them -- all 4096 values below came out equal to torch's (v_cvt_pk_bf16_f32 with the
    # default denormal mode of a HIP kernel), none was flushed.
    sub = np.concatenate([rng.integers(1, 0x00800000, size=2044, dtype=np.int64), [1, 0x007fffff, 0x00008000, 0x00018000]]).astype(np.uint32)
    sub = _f32_bits(np.concatenate([sub, sub | 0x80000000]))
    got, ref = _to_bf16_dev(ops, sub).numpy().view(np.uint16), bits(sub.bfloat16()).numpy().view(np.uint16)
    sign = (sub.view(torch.int32).numpy().view(np.uint32) >> 16).astype(np.uint16) & 0x8000
    same, flushed = got == ref, got == sign
    assert (same | flushed).all()
    print("[rowk] f32_to_bf16 subnormal inputs: %d equal to torch, %d flushed to a signed zero (of %d, %d where both coincide)"
          % (same.sum(), flushed.sum(), got.size, (same & flushed).sum()))
    assert same.all() or flushed.all()                                           # one behaviour, not a mixture
    # n = 0 and n = 4
    ops.f32_to_bf16(torch.zeros(0, dtype=F32, device=DEV), torch.zeros(0, dtype=BF16, device=DEV))
    four = torch.tensor([1.0, -2.5, 3.0e38, 1.0e-3])
    assert torch.equal(_to_bf16_dev(ops, four), bits(four.bfloat16()))


def test_bf16_to_f32_all_patterns(ops):
    u = np.arange(65536, dtype=np.uint32)
    x = torch.from_numpy(u.astype(np.uint16).view(np.int16)).to(DEV)
    y = torch.full((65536 + 4,), 0x7b7b7b7b, dtype=I32, device=DEV)
    ops.bf16_to_f32(x.view(BF16), y.view(F32)[:65536])
    torch.cuda.synchronize()
    assert np.array_equal(y[:65536].cpu().numpy().view(np.uint32), u << 16)      # bit-exact, NaN payloads included
    assert bool((y[65536:] == 0x7b7b7b7b).all())
    ops.bf16_to_f32(torch.zeros(0, dtype=BF16, device=DEV), torch.zeros(0, dtype=F32, device=DEV))     # n = 0
    y4 = torch.zeros(4, dtype=F32, device=DEV)
    ops.bf16_to_f32(x[0x3f80:0x3f84].contiguous().view(BF16), y4)                                      # n = 4
    assert np.array_equal(y4.cpu().numpy().view(np.uint32), u[0x3f80:0x3f84] << 16)


# ====================================================================== wdiff_sum
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_wdiff_sum(ops, n, kind):
    rng = np.random.default_rng(n)
    if kind == "exact":
        k, terms, _ = EXACT["wdiff_sum"]
        assert n <= terms
        a, b, w = ints(rng, k["d"] // 2, n), ints(rng, k["d"] // 2, n), ints(rng, k["w"], n)
    else:
        a, b, w = 30.0 + rng.standard_normal(n), 25.0 + rng.standard_normal(n), rng.random(n) / max(n, 1)
    a, b, w = (t.astype(np.float32) for t in (a, b, w))
    out = torch.full((3,), 123.0, dtype=F32, device=DEV)                         # a sentinel: n = 0 must WRITE 0
    ops.wdiff_sum(f32dev(a), f32dev(b), f32dev(w), out[:1])
    torch.cuda.synchronize()
    assert bool((out[1:] == 123.0).all())
    ref = rowref.wdiff_sum(a, b, w)
    if kind == "exact" or n == 0:
        assert float(out[0]) == ref
    else:
        terms32 = w * (a - b)
        check_real("wdiff_sum", "n=%d" % n, out[:1], np.array([ref]), np.array([rowref.seq_sum32(terms32, 0)]),
                   float(np.abs(w.astype(np.float64) * (a.astype(np.float64) - b)).sum()))
