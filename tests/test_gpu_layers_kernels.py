"""GPU: kbner_gather_rows_layers, kbner_scatter_add_rows_ld and kbner_head_bwd_dx above 1024 columns (csrc/rows.hip) through
kbner.ops against tests/layersref.py and tests/rowref.py, with NaN canary rows behind every output.

Gather: the case list of layersref.GATHER_CASES -- (R, n) in {(1, 1), (6, 3), (70, 7)}, H in {8, 128, 520, 1024}, k in 1..4, both
modes, dropout none / element / locked / both -- on Gaussian bf16 sources of 3 R rows with an unsorted index holding -1 entries.
Concatenation without dropout is a copy: bit equality; with dropout headdropref.real_bound; the mean layersref.gather_mean_bound.
Dropped elements and -1 rows are exactly 0.  EXACT cases: integers of [-8, 8], k in {2, 4} for the mean (|sum| <= 32, / k exact in
bf16), p in {0, 0.5} (scale 1, 2 or 4): the output must EQUAL the reference.  k = 1 equals ops.gather_rows / gather_rows_drop bit for
bit.  Scatter-add: layersref.SCATTER_CASES (col0 in {0, H, 3 H} of ld = 4 H, scale in {1, 0.25}, dst pre-filled) within
layersref.scatter_add_bound; exact: integers of [-64, 64] into a start of [-64, 64]; rows idx does not name keep their bits.
head_bwd: (R, H, T) in {(5, 1032, 29), (70, 2048, 137), (3, 8192, 3)}, exact and real kinds as tests/test_gpu_head_wide.py."""
import numpy as np
import pytest
import torch

import headdropref as hd
import layersref as lr
import mmaref
import rowref
from rowref import ints

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
CANARY = 3


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    return _ops


def _dev_bf16(a64):
    """float64 values that ARE bf16 numbers -> device bf16 tensor (asserted lossless)"""
    t = torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).bfloat16()
    assert np.array_equal(t.float().numpy().astype(np.float64), a64)
    return t.to(DEV)


def _f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _idx(idx):
    return torch.from_numpy(idx.astype(np.int32)).to(DEV)


def _run_gather(ops, xs, idx, n, mean, de, dl):
    R, H, k = idx.size, xs[0].shape[1], len(xs)
    W = H if mean else k * H
    full = torch.full((R + CANARY, W), NAN, dtype=BF16, device=DEV)
    out = full[:R]
    got = ops.gather_rows_layers([_dev_bf16(x) for x in xs], _idx(idx), n, mean=mean, drop_e=de, drop_l=dl, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (R, W)
    assert torch.isnan(full[R:]).all(), "gather_rows_layers wrote behind its output"
    return out


@pytest.mark.parametrize("R,n,H,k,mean,drop", lr.GATHER_CASES)
def test_gather_real(ops, R, n, H, k, mean, drop):
    xs, idx = lr.gather_inputs(R, n, H, k)
    de, dl = lr.sites(drop, R + H)
    got = _run_gather(ops, xs, idx, n, mean, de, dl)
    g64 = _f64(got)
    ref = lr.gather_layers(xs, idx, n, mean, de, dl)
    mag = lr.gather_abs(xs, idx, n, mean, de, dl)
    assert np.isfinite(g64).all() and (g64[mag == 0] == 0).all(), "a dropped element or a -1 row is not exactly 0"
    if mean:
        bound = lr.gather_mean_bound(ref, mag, k)
    elif drop == "none":
        assert torch.equal(_bits(got), _bits(_dev_bf16(ref))), "concatenation without dropout is a copy"
        bound = np.zeros_like(ref)
    else:
        bound = hd.real_bound(ref)
    diff = np.abs(g64 - ref)
    nz = bound > 0
    share = float((diff[nz] / bound[nz]).max()) if nz.any() else 0.0
    print("[layers] gather R=%d n=%d H=%d k=%d %s %s: worst error %.3e, worst share of the bound %.3f"
          % (R, n, H, k, "mean" if mean else "concat", drop, float(diff.max()), share))
    assert (diff <= bound).all()
    if drop != "none" and R * H >= 512:
        assert (mag == 0).any() and (g64 != 0).any()


EXACT_P = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]


@pytest.mark.parametrize("p_e,p_l", EXACT_P)
@pytest.mark.parametrize("R,n,H,k,mean", [(1, 1, 8, 2, True), (6, 3, 520, 4, True), (70, 7, 1024, 2, True), (6, 3, 520, 3, False),
                                           (70, 7, 128, 4, False), (6, 3, 1024, 4, True)])
def test_gather_exact(ops, R, n, H, k, mean, p_e, p_l):
    rng = np.random.default_rng(R + H + k)
    rows = 3 * R
    xs = [ints(rng, 8, (rows, H)) for _ in range(k)]
    idx = rng.permutation(rows)[:R].astype(np.int64)
    idx[rng.random(R) < 0.25] = -1
    de, dl = (0x1234567 + R, mmaref.dropout_thresh(p_e)), (0x7654321 + H, mmaref.dropout_thresh(p_l))
    got = _run_gather(ops, xs, idx, n, mean, de, dl)
    ref = lr.gather_layers(xs, idx, n, mean, de, dl)
    assert np.abs(ref).max() <= 8 * 4
    assert torch.equal(_bits(got), _bits(_dev_bf16(ref)))
    ke, kl = hd.keep(R, ref.shape[1], n, de, dl)
    dead = ~(ke & kl & (idx >= 0)[:, None])
    assert (_f64(got)[dead] == 0).all()


@pytest.mark.parametrize("R,n,H", [(1, 1, 8), (6, 3, 520), (70, 7, 1024), (8200, 8, 8)])
def test_one_layer_equals_the_plain_kernels(ops, R, n, H):
    """k = 1, concatenation: gather_rows without dropout, gather_rows_drop with it, bit for bit (R = 8200: more rows than the grid has
    waves, the row stride loop)"""
    xs, idx = lr.gather_inputs(R, n, H, 1)
    src, idx_d = _dev_bf16(xs[0]), _idx(idx)
    got = _run_gather(ops, xs, idx, n, False, ops.NO_DROP, ops.NO_DROP)
    assert torch.equal(_bits(got), _bits(ops.gather_rows(src, idx_d)))
    for drop in ("element", "locked", "both"):
        de, dl = lr.sites(drop, R)
        got = _run_gather(ops, xs, idx, n, False, de, dl)
        assert torch.equal(_bits(got), _bits(ops.gather_rows_drop(src, idx_d, n, de, dl)))
    # the mean of one layer is that layer
    got = _run_gather(ops, xs, idx, n, True, ops.NO_DROP, ops.NO_DROP)
    assert torch.equal(_bits(got), _bits(ops.gather_rows(src, idx_d)))


def _run_scatter(ops, dst, d, col0, idx, scale, n, de, dl):
    rows, H = dst.shape
    full = torch.full((rows + CANARY, H), NAN, dtype=BF16, device=DEV)
    full[:rows] = _dev_bf16(dst)
    view = full[:rows]
    dfull = torch.full((d.shape[0] + CANARY, d.shape[1]), NAN, dtype=BF16, device=DEV)      # NaN rows behind dout: a read past R shows
    dfull[:d.shape[0]] = _dev_bf16(d)
    ops.scatter_add_rows_ld(dfull[:d.shape[0]], col0, _idx(idx), view, n, scale, de, dl)
    torch.cuda.synchronize()
    assert torch.isnan(full[rows:]).all(), "scatter_add_rows_ld wrote behind its output"
    return view


@pytest.mark.parametrize("R,n,H,c,scale,drop", lr.SCATTER_CASES)
def test_scatter_add_real(ops, R, n, H, c, scale, drop):
    dst, d, idx = lr.scatter_inputs(R, n, H)
    de, dl = lr.sites(drop, R + H)
    got = _run_scatter(ops, dst, d, c * H, idx, scale, n, de, dl)
    ref, mag = lr.scatter_add_ld(dst, d, 4 * H, c * H, idx, scale, n, de, dl)
    named = idx[idx >= 0]
    untouched = np.setdiff1d(np.arange(dst.shape[0]), named)
    assert torch.equal(_bits(got)[untouched], _bits(_dev_bf16(dst))[untouched]), "a row idx does not name was written"
    g64 = _f64(got)
    assert np.isfinite(g64).all()
    bound = lr.scatter_add_bound(ref, mag)
    diff = np.abs(g64 - ref)[named]
    share = float((diff / bound[named]).max()) if named.size else 0.0
    print("[layers] scatter_add R=%d n=%d H=%d col0=%d scale=%g %s: worst error %.3e, worst share of the bound %.3f"
          % (R, n, H, c * H, scale, drop, float(diff.max()) if named.size else 0.0, share))
    assert (diff <= bound[named]).all()
    # a dropped element leaves dst as it was
    ke, kl = hd.keep(R, 4 * H, n, de, dl)
    dead = ~(ke & kl)[:, c * H:(c + 1) * H][idx >= 0]
    assert np.array_equal(g64[named][dead], dst[named][dead])


@pytest.mark.parametrize("p_e,p_l", EXACT_P)
@pytest.mark.parametrize("R,n,H,c,scale", [(1, 1, 8, 0, 1.0), (6, 3, 520, 3, 0.25), (70, 7, 1024, 1, 1.0), (70, 7, 128, 3, 0.25)])
def test_scatter_add_exact(ops, R, n, H, c, scale, p_e, p_l):
    rng = np.random.default_rng(R * 3 + H + c)
    rows = 3 * R
    dst, d = ints(rng, 64, (rows, H)), ints(rng, 64, (R, 4 * H))
    if scale != 1.0:
        d = d * 4                                               # d * 0.25 stays an integer of [-64, 64]; |4 d| <= 256 is a bf16 number
    idx = rng.permutation(rows)[:R].astype(np.int64)
    idx[rng.random(R) < 0.25] = -1
    de, dl = (0xABCDEF + R, mmaref.dropout_thresh(p_e)), (0xFEDCBA + H, mmaref.dropout_thresh(p_l))
    got = _run_scatter(ops, dst, d, c * H, idx, scale, n, de, dl)
    ref, _ = lr.scatter_add_ld(dst, d, 4 * H, c * H, idx, scale, n, de, dl)
    assert np.abs(ref).max() <= 64 + 64 * 4                      # integers up to 320: below 2^8 every integer is a bf16 number, ...
    ref_b = lr.round_bf16(ref)                                   # ... above it the one rounding of the store
    assert np.array_equal(ref_b[np.abs(ref) <= 256], ref[np.abs(ref) <= 256])
    assert torch.equal(_bits(got), _bits(_dev_bf16(ref_b)))


# ---------------------------------------------------------------------- head_bwd above 1024 columns
def _f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("R,H,T", [(5, 1032, 29), (70, 2048, 137), (3, 8192, 3)])
def test_head_bwd_wide_rows(ops, R, H, T, kind):
    rng = np.random.default_rng(R * 3 + H + T)
    if kind == "exact":
        assert T < 256 and R * 4 + 8 < rowref.EXACT_LIMIT
        de, x, w = ints(rng, 1, (R, T)), ints(rng, 4, (R, H)), ints(rng, 1, (T, H))
        dw0, db0 = ints(rng, 8, (T, H)), ints(rng, 8, (T,))
    else:
        de, x, w = 0.1 * rng.standard_normal((R, T)), rng.standard_normal((R, H)), 0.05 * rng.standard_normal((T, H))
        dw0, db0 = rng.standard_normal((T, H)), rng.standard_normal(T)
    xb = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16()
    x64 = xb.float().numpy().astype(np.float64)
    de, w, dw0, db0 = (a.astype(np.float32) for a in (de, w, dw0, db0))
    xfull = torch.full((R + CANARY, H), NAN, dtype=BF16, device=DEV)
    xfull[:R] = xb.to(DEV)
    defull = torch.full((R + CANARY, T), NAN, dtype=F32, device=DEV)
    defull[:R] = _f32dev(de)
    dw, db = _f32dev(dw0), _f32dev(db0)
    dx = ops.head_bwd(defull[:R], xfull[:R], _f32dev(w), dw, db)
    torch.cuda.synchronize()
    assert tuple(dx.shape) == (R, H)
    rdx, rdw, rdb = rowref.head_bwd(de, x64, w)
    rdw, rdb = rdw + dw0, rdb + db0
    if kind == "exact":
        for got, ref in ((dx, rdx), (dw, rdw), (db, rdb)):
            assert np.abs(ref).max() < rowref.EXACT_LIMIT
            assert np.array_equal(_f64(got).reshape(ref.shape), ref)
    else:
        a64 = np.abs(de.astype(np.float64))
        for name, got, ref, e32, sabs, bf in (
                ("head_bwd_dx", dx, rdx, rowref.seq_dot32(de, w.T), a64 @ np.abs(w.astype(np.float64)), True),
                ("head_bwd_dw", dw, rdw, rowref.seq_dot32(de.T, x64.T) + dw0, a64.T @ np.abs(x64) + np.abs(dw0), False)):
            tol, err32 = rowref.tolerance(ref, e32, sabs, bf16_out=bf)
            g = _f64(got).reshape(ref.shape)
            diff = np.abs(g - ref)
            print("[layers] %s R=%d H=%d T=%d: kernel_err %.3e  f32_numpy_err %.3e  tolerance_share %.3f"
                  % (name, R, H, T, float(diff.max()), err32, float((diff / np.maximum(tol, 1e-300)).max())))
            assert np.isfinite(g).all() and (diff <= tol).all()


# ---------------------------------------------------------------------- argument errors
def test_argument_errors_launch_nothing(ops):
    from kbner import lib as L
    lib = L.load()
    st = L.stream_ptr()
    import ctypes
    site = (1, mmaref.dropout_thresh(0.5))

    def raw_gather(srcs, k, mean, idx, out, R, H, n):
        ptrs = (ctypes.c_void_p * max(len(srcs), 1))(*[s.data_ptr() for s in srcs])
        return lib.kbner_gather_rows_layers(ptrs, k, mean, L.ptr(idx), L.ptr(out), R, H, n, site[0], site[1], site[0], site[1], st)

    idx = torch.arange(4, dtype=I32, device=DEV)
    out = torch.full((4, 9 * 1024), NAN, dtype=BF16, device=DEV)
    src16 = torch.ones(8, 16, dtype=BF16, device=DEV)
    src12 = torch.ones(8, 12, dtype=BF16, device=DEV)
    src1k = torch.ones(8, 1024, dtype=BF16, device=DEV)
    # k = 0, k = 33, H = 12, a concatenation of 9 * 1024 columns, R % n != 0: refused by ops and by the C entry point (EINVAL)
    for srcs, n in (([], 2), ([src16] * 33, 2), ([src12], 2), ([src1k] * 9, 2), ([src16], 3)):
        with pytest.raises(L.KbnerError):
            ops.gather_rows_layers(srcs, idx, n, drop_e=site, drop_l=site)
        k = len(srcs)
        H = srcs[0].shape[1] if srcs else 16
        assert raw_gather(srcs if srcs else [src16], k, 0, idx, out, 4, H, n) == -22
    outm = torch.full((4 + CANARY, 1024), NAN, dtype=BF16, device=DEV)
    assert raw_gather([src1k] * 9, 9, 1, idx, outm, 4, 1024, 2) == 0              # the mean of 9 layers is H wide: taken
    torch.cuda.synchronize()
    assert torch.isnan(outm[4:]).all() and bool(((outm[:4] == 0) | (outm[:4] == 4)).all())      # 1 * the two scales of p = 0.5, or dropped
    with pytest.raises(L.KbnerError):
        ops.gather_rows_layers([src16, src1k], idx, 2)                              # sources of different widths
    with pytest.raises(L.KbnerError):
        ops.gather_rows_layers([src16.float()], idx, 2)
    # scatter-add: ld, col0 multiples of 8; col0 + H inside the row; R % n == 0
    dst = torch.full((8, 16), 7.0, dtype=BF16, device=DEV)
    for ld, col0, n in ((36, 0, 2), (32, 4, 2), (32, 24, 2), (32, 0, 3)):
        dout = torch.ones(4, ld, dtype=BF16, device=DEV)
        with pytest.raises(L.KbnerError):
            ops.scatter_add_rows_ld(dout, col0, idx, dst, n, 1.0, site, site)
        rc = lib.kbner_scatter_add_rows_ld(L.ptr(dout), ld, col0, L.ptr(idx), L.ptr(dst), 4, 16, 1.0, n, site[0], site[1], site[0], site[1], st)
        assert rc == -22, rc
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and bool((dst == 7.0).all())
    # R = 0 returns cleanly
    empty = torch.empty(0, dtype=I32, device=DEV)
    assert tuple(ops.gather_rows_layers([src16, src16], empty, 3).shape) == (0, 32)
    ops.scatter_add_rows_ld(torch.empty(0, 32, dtype=BF16, device=DEV), 16, empty, dst, 3)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
