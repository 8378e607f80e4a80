"""TEST INFRASTRUCTURE: float64 reference of kbner_pool_rows_layers (include/kbner.h) -- the sub-token pooling of a frozen
TransformerWordEmbeddings over a layer selection (flair/embeddings.py:3303-3345) -- written from its definition, the case list the GPU
test runs, and the check.  numpy only; no import of kbner.

k sources x_j [rows_src, H]; word r owns the rows span_rows[span_ptr[r]:span_ptr[r + 1]] (m of them, in order).  Per layer
    first: p_j = x_j[rows[0]]   last: p_j = x_j[rows[m-1]]   first_last: p_j = [x_j[rows[0]], x_j[rows[m-1]]]   mean: p_j = sum_t x_j[rows[t]] / m
and the row is p_0 .. p_{k-1} side by side or, layer_mean, sum_j p_j / k.  m == 0: zeros.

THE CHECK (per element, against the float64 reference; the kernel reads bf16, computes in float32, stores bf16 once):
    first / last / first_last without the layer mean copy: bit equality.
    everything else   |got - ref| <= 2^-8 |ref| + (m + k + 4) * 2^-24 * abs
                      abs = the same pooling of |x| (it bounds every intermediate).  m - 1 float32 additions over the span, the rounded
                      constant 1 / m and its product; k - 1 additions over the layers, the rounded constant 1 / k and its product:
                      (m - 1) + 2 + (k - 1) + 2 = m + k + 2 roundings of at most 2^-24 each relative to abs, two more for the
                      compounding of the (1 + 2^-24) factors; then ONE bf16 rounding of the result (2^-8 covers round-to-nearest's 2^-9
                      with the float32 error under it).  A derived bound, in the style of layersref.gather_mean_bound.
    exact cases       integer-valued inputs, m and k powers of two: every partial sum and both scalings are exact in float32, so the
                      result is the float64 reference rounded once -- bit equality (one of them sits on bf16 ties: nearest EVEN)."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
OPS = ("first", "last", "first_last", "mean")
SENTINEL = 123.0          # a bf16 number; what the output matrix holds before the launch


def width(op, k, H, layer_mean):
    return (2 * H if op == "first_last" else H) * (1 if layer_mean else k)


def is_copy(op, layer_mean):
    return op != "mean" and not layer_mean


def span_lengths(span_ptr):
    sp = np.asarray(span_ptr, np.int64)
    return sp[1:] - sp[:-1]


def pool_layers(xs64, span_ptr, span_rows, op, layer_mean):
    """float64, unrounded -> [R, W]"""
    xs = [np.asarray(x, F64) for x in xs64]
    sp, sr = np.asarray(span_ptr, np.int64), np.asarray(span_rows, np.int64)
    k, H, R = len(xs), xs[0].shape[1], sp.size - 1
    out = np.zeros((R, width(op, k, H, layer_mean)), F64)
    for r in range(R):
        rows = sr[sp[r]:sp[r + 1]]
        if rows.size == 0:
            continue
        ps = []
        for x in xs:
            if op == "first":
                ps.append(x[rows[0]])
            elif op == "last":
                ps.append(x[rows[-1]])
            elif op == "first_last":
                ps.append(np.concatenate([x[rows[0]], x[rows[-1]]]))
            else:
                ps.append(x[rows].sum(0) / rows.size)
        out[r] = sum(ps[1:], ps[0].copy()) / k if layer_mean else np.concatenate(ps)
    return out


def pool_abs(xs64, span_ptr, span_rows, op, layer_mean):
    """the same pooling of |x|: what the bound is relative to"""
    return pool_layers([np.abs(np.asarray(x, F64)) for x in xs64], span_ptr, span_rows, op, layer_mean)


def pool_layers_f32(xs, span_ptr, span_rows, op, layer_mean, fma=False):
    """float32 in the kernel's order of operations (unrounded to bf16).  fma: the span mean's scaling fused into the layer sum's
    addition, acc = fma(sum, 1 / m, acc) -- one rounding instead of two, as a compiler may contract it (emulated in float64: the
    product of two float32 numbers is exact there)"""
    xs = [np.asarray(x, F32) for x in xs]
    sp, sr = np.asarray(span_ptr, np.int64), np.asarray(span_rows, np.int64)
    k, H, R = len(xs), xs[0].shape[1], sp.size - 1
    out = np.zeros((R, width(op, k, H, layer_mean)), F32)
    inv_k = F32(1.0) / F32(k)
    for r in range(R):
        rows = sr[sp[r]:sp[r + 1]]
        m = rows.size
        if m == 0:
            continue
        inv_m = F32(1.0) / F32(m)
        ps, sums = [], []
        for x in xs:
            if op == "mean":
                s = x[rows[0]].copy()
                for t in rows[1:]:
                    s = (s + x[t]).astype(F32)
                sums.append(s)
                ps.append((s * inv_m).astype(F32))
            elif op == "first_last":
                ps.append(np.concatenate([x[rows[0]], x[rows[-1]]]))
            else:
                ps.append(x[rows[0] if op == "first" else rows[-1]].copy())
        if not layer_mean:
            out[r] = np.concatenate(ps)
            continue
        acc = ps[0]
        for j in range(1, k):
            if fma and op == "mean":
                acc = (acc.astype(F64) + sums[j].astype(F64) * F64(inv_m)).astype(F32)
            else:
                acc = (acc + ps[j]).astype(F32)
        out[r] = (acc * inv_k).astype(F32)
    return out


def round_bf16(a):
    """float -> the nearest bf16 number (ties to even), as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).bfloat16().float().numpy().astype(F64)


def bound(ref64, abs64, span_ptr, k):
    m = span_lengths(span_ptr).astype(F64)[:, None]
    return 2.0 ** -8 * np.abs(ref64) + (m + k + 4) * 2.0 ** -24 * np.abs(abs64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def check(got, xs64, span_ptr, span_rows, op, layer_mean, exact=False):
    """got [R, W]: the kernel's block as float (bf16 numbers).  Raises AssertionError with the first offending element."""
    got = np.asarray(got, F64)
    ref = pool_layers(xs64, span_ptr, span_rows, op, layer_mean)
    assert got.shape == ref.shape, "shape %s, expected %s" % (got.shape, ref.shape)
    assert np.isfinite(got).all(), "non-finite output"
    if is_copy(op, layer_mean) or exact:
        want = ref if is_copy(op, layer_mean) else round_bf16(ref)
        bad = _bits(got) != _bits(want)
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError("%s%s: not bit-equal at [%d, %d]: got %r, expected %r (%d elements differ)"
                                 % (op, " + layer mean" if layer_mean else "", r, c, got[r, c], want[r, c], int(bad.sum())))
        return
    tol = bound(ref, pool_abs(xs64, span_ptr, span_rows, op, layer_mean), span_ptr, len(xs64))
    bad = np.abs(got - ref) > tol
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError("%s%s: |got - ref| = %.3e > %.3e at [%d, %d] (got %r, ref %r; %d elements outside the bound)"
                             % (op, " + layer mean" if layer_mean else "", abs(got[r, c] - ref[r, c]), tol[r, c], r, c, got[r, c],
                                ref[r, c], int(bad.sum())))


def check_matrix(full, R, col, xs64, span_ptr, span_rows, op, layer_mean, exact=False):
    """full [rows_out, ld]: the whole output matrix, filled with SENTINEL before the launch.  Everything outside rows [0, R) x columns
    [col, col + W) must still hold it; the block goes through check()."""
    full = np.asarray(full, F64)
    W = width(op, len(xs64), np.asarray(xs64[0]).shape[1], layer_mean)
    outside = np.ones(full.shape, bool)
    outside[:R, col:col + W] = False
    touched = outside & (full != SENTINEL)
    if touched.any():
        r, c = np.argwhere(touched)[0]
        raise AssertionError("wrote outside its block: element [%d, %d] (block rows [0, %d), columns [%d, %d))" % (r, c, R, col, col + W))
    check(full[:R, col:col + W], xs64, span_ptr, span_rows, op, layer_mean, exact)


# ------------------------------------------------------------------ the case list
ROWS = [1, 6, 70]
WIDTHS = [8, 128, 520, 1024]        # H = 520: the tail of the second 512-column chunk
KS = [1, 2, 4]


def pool_cases():
    """(R, H, k, op, layer_mean): a pruned walk over the grid, as layersref.gather_cases prunes its own -- every value of every axis
    occurs, H = 520 with every op, R = 1 with the smallest and the widest row"""
    cases, i = [], 0
    for R in ROWS:
        for H in WIDTHS:
            for k in KS:
                for op in OPS:
                    for lm in (False, True):
                        i += 1
                        must = (H == 520 and k == 2 and R == 70) or (R == 1 and H in (8, 1024) and k == 4 and op in ("mean", "first_last"))
                        if must or i % 7 == 0:
                            cases.append((R, H, k, op, lm))
    return cases


POOL_CASES = pool_cases()


def bf16_values(rng, shape):
    """Gaussian values that are bf16 numbers, none of them 0 (float64)"""
    t = torch.from_numpy(rng.standard_normal(shape).astype(F32)).bfloat16()
    t[t == 0] = 1.0
    return t.float().numpy().astype(F64)


def spans_for(R, rows_src, rng):
    """The span table of a case.  R == 1: one span of 3 rows.  Otherwise: empty spans at the first and the last row, lengths 1, 2, 3 and
    17, a seam (rows that jump backwards: non-consecutive, non-monotone), one source row named by two words; the rest random of 0 .. 4
    rows, drawn with replacement from all source rows."""
    if R == 1:
        lens = [3]
    else:
        lens = [0, 1, 2, 3, 17] + [int(x) for x in rng.integers(0, 5, size=R - 6)] + [0]
    spans = [[int(x) for x in rng.integers(0, rows_src, size=m)] for m in lens]
    if R > 1:
        spans[2] = [rows_src - 2, 1]                  # a seam: the second piece lies far before the first
        spans[3][0] = spans[1][0]                     # a source row two words name
    span_ptr = np.concatenate([[0], np.cumsum([len(s) for s in spans])]).astype(np.int64)
    span_rows = np.asarray([x for s in spans for x in s], np.int64)
    return span_ptr, span_rows


def pool_inputs(R, H, k, salt=0):
    """-> (k bf16-valued sources [2 R + 24, H], span_ptr [R + 1], span_rows)"""
    rng = np.random.default_rng(R * 131 + H + 1000 * k + salt)
    rows_src = 2 * R + 24
    span_ptr, span_rows = spans_for(R, rows_src, rng)
    return [bf16_values(rng, (rows_src, H)) for _ in range(k)], span_ptr, span_rows


def exact_inputs(H=136, k=4, seed=7):
    """Integer-valued bf16 inputs in [-128, 128], spans of 0, 1, 2, 4, 8 and 16 rows (powers of two): with k a power of two every
    partial sum (|.| <= 16 * 4 * 128 < 2^24) and both scalings are exact in float32"""
    rng = np.random.default_rng(seed)
    rows_src = 40
    lens = [0, 1, 2, 4, 8, 16, 2, 0]
    spans = [[int(x) for x in rng.integers(0, rows_src, size=m)] for m in lens]
    span_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    span_rows = np.asarray([x for s in spans for x in s], np.int64)
    xs = [rng.integers(-128, 129, size=(rows_src, H)).astype(F64) for _ in range(k)]
    return xs, span_ptr, span_rows


def tie_inputs():
    """One source, one word of two rows whose exact means lie halfway between neighbouring bf16 numbers (spacing 2 in [256, 512)):
    (256 + 258) / 2 = 257 -> 256, (258 + 260) / 2 = 259 -> 260 (nearest EVEN significand both times), and the negatives"""
    a = np.asarray([256, 258, -256, -258, 260, 262, 384, 386], F64)
    b = a + np.sign(a) * 2
    want = np.asarray([256, 260, -256, -260, 260, 264, 384, 388], F64)
    return [np.stack([a, b])], np.asarray([0, 2], np.int64), np.asarray([0, 1], np.int64), want[None, :]


EXACT_CASES = [(op, lm) for op in OPS for lm in (False, True)]      # on exact_inputs(); the copies among them are bit-equal anyway
