"""GPU: kbner_gather_rows_drop / kbner_scatter_rows_drop (csrc/rows.hip) through kbner.ops against the integer / float64
reference of tests/headdropref.py, with NaN canary rows behind every output.

EXACT cases: p in {0.5, 0.75} at either or both sites -- drop_thresh(0.5) = 2^31, so a scale is exactly 2 or 4, the product of
two scales a power of two, and a bf16 input times it is a bf16 number: the assertion is BIT equality with the reference, and the
zero pattern equals the integer keep test.  REAL cases: p_e = 0.1 and / or p_l = 0.3 on Gaussian bf16 inputs, per element within
2^-8 |ref| (one bf16 rounding: half an ulp reaches 2^-8 relative at the bottom of a binade) + 4 * 2^-24 |ref| (the float32
roundings of the multiplier and of the product); dropped elements are exactly 0; the worst share of the bound used is printed
(MI355X run that accompanied this module: 61 cases, 2.4 s; worst share 0.923, gather and scatter alike, at p = (0.1, 0.3))."""
import numpy as np
import pytest
import torch

import headdropref as hd
import mmaref

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
CANARY = 3

# (R, n, H): smallest; small rows with n = 3; one full 64-lane chunk, R no multiple of 4; chunk + an 8-wide tail; two chunks;
# more rows than rows_grid's 2048 x 4 waves (the row stride loop, and r / n across strides)
SHAPES = [(1, 1, 8), (6, 3, 8), (7, 1, 512), (12, 4, 520), (10, 5, 1024), (8200, 8, 8)]
EXACT_P = [(0.5, 0.0), (0.0, 0.5), (0.75, 0.0), (0.0, 0.75), (0.5, 0.5), (0.5, 0.75), (0.75, 0.5), (0.75, 0.75)]
REAL_P = [(0.1, 0.0), (0.0, 0.3), (0.1, 0.3)]


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    return _ops


def _sites(p_e, p_l, salt):
    return (0x9E3779B9 ^ (salt * 7919), mmaref.dropout_thresh(p_e)), ((0xC2B2AE35 + salt * 104729) & 0xFFFFFFFF, mmaref.dropout_thresh(p_l))


def _case(R, n, H, salt):
    """bf16 source with more rows than R (no zero element), a cotangent, and idx: a permutation of source rows, ~1/4 of them -1"""
    rng = np.random.default_rng(R * 131 + n * 17 + H + salt)
    rows_src = R + 5
    idx = rng.permutation(rows_src)[:R].astype(np.int64)
    idx[rng.random(R) < 0.25] = -1
    def bf(shape):
        t = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).bfloat16()
        t[t == 0] = 1.0
        return t
    return bf((rows_src, H)), bf((R, H)), idx, rows_src


def _padded(t, fill=NAN):
    full = torch.full((t.shape[0] + CANARY,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=DEV)
    full[:t.shape[0]] = t.to(DEV)
    return full, full[:t.shape[0]]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _as_bf16(a64):
    """float64 values that ARE bf16 numbers -> bf16 tensor (asserted lossless)"""
    t = torch.from_numpy(np.ascontiguousarray(a64, dtype=np.float32)).bfloat16()
    assert np.array_equal(t.float().numpy().astype(np.float64), a64)
    return t


def _f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _run_gather(ops, src, idx, n, de, dl):
    R, H = idx.size, src.shape[1]
    full, out = _padded(torch.zeros(R, H, dtype=BF16))
    out.fill_(NAN)
    got = ops.gather_rows_drop(src.to(DEV), torch.from_numpy(idx.astype(np.int32)).to(DEV), n, de, dl, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.isnan(full[R:]).all(), "gather_rows_drop wrote behind its output"
    return out.cpu()


SENTINEL = 7.0


def _run_scatter(ops, d, idx, rows_src, n, de, dl):
    H = d.shape[1]
    full, dsrc = _padded(torch.full((rows_src, H), SENTINEL, dtype=BF16))
    ops.scatter_rows_drop(d.to(DEV), torch.from_numpy(idx.astype(np.int32)).to(DEV), dsrc, n, de, dl)
    torch.cuda.synchronize()
    assert torch.isnan(full[rows_src:]).all(), "scatter_rows_drop wrote behind its output"
    return dsrc.cpu()


def _scatter_expected(ref_dx, idx, rows_src):
    """the reference's rows where idx names them, the pre-filled sentinel everywhere else"""
    exp = np.full(ref_dx.shape, SENTINEL, np.float64)
    named = idx[idx >= 0]
    exp[named] = ref_dx[named]
    return exp


@pytest.mark.parametrize("p_e,p_l", EXACT_P)
@pytest.mark.parametrize("R,n,H", SHAPES)
def test_exact(ops, R, n, H, p_e, p_l):
    de, dl = _sites(p_e, p_l, R + H)
    src, d, idx, rows_src = _case(R, n, H, 1)
    ke, kl = hd.keep(R, H, n, de, dl)
    live = ke & kl & (idx >= 0)[:, None]
    # gather: the reference's bits, and the integer keep test's zero pattern
    got = _run_gather(ops, src, idx, n, de, dl)
    ref = hd.gather(_f64(src), idx, n, de, dl)
    assert torch.equal(_bits(got), _bits(_as_bf16(ref)))
    assert np.array_equal(_f64(got) != 0, live)
    # scatter of a cotangent of the gather's shape: the same masks; only the rows idx names are written
    gotd = _run_scatter(ops, d, idx, rows_src, n, de, dl)
    exp = _scatter_expected(hd.scatter(_f64(d), idx, rows_src, n, de, dl), idx, rows_src)
    assert torch.equal(_bits(gotd), _bits(_as_bf16(exp)))
    named = idx[idx >= 0]
    assert np.array_equal(_f64(gotd)[named] != 0, live[idx >= 0])
    untouched = np.setdiff1d(np.arange(rows_src), named)
    assert (_f64(gotd)[untouched] == SENTINEL).all()


def _check_real(what, got64, ref, dead):
    assert np.isfinite(got64).all()
    assert (got64[dead] == 0).all(), "%s: a dropped element is not exactly 0" % what
    bound = hd.real_bound(ref)
    diff = np.abs(got64 - ref)
    nz = bound > 0
    share = float((diff[nz] / bound[nz]).max()) if nz.any() else 0.0
    print("[headdrop] %s: worst error %.3e, worst share of the bound %.3f" % (what, float(diff.max()), share))
    assert (diff <= bound).all(), "%s: worst share of the bound %.3f" % (what, share)


@pytest.mark.parametrize("p_e,p_l", REAL_P)
@pytest.mark.parametrize("R,n,H", [(12, 4, 520), (10, 5, 1024)])
def test_real(ops, R, n, H, p_e, p_l):
    de, dl = _sites(p_e, p_l, R + H + 1)
    src, d, idx, rows_src = _case(R, n, H, 2)
    ke, kl = hd.keep(R, H, n, de, dl)
    dead = ~(ke & kl & (idx >= 0)[:, None])
    assert dead.any() and (~dead).any()
    case = "R=%d n=%d H=%d p=(%.1f, %.1f)" % (R, n, H, p_e, p_l)
    _check_real("gather " + case, _f64(_run_gather(ops, src, idx, n, de, dl)), hd.gather(_f64(src), idx, n, de, dl), dead)
    gotd = _f64(_run_scatter(ops, d, idx, rows_src, n, de, dl))
    ref = hd.scatter(_f64(d), idx, rows_src, n, de, dl)
    named = idx[idx >= 0]
    _check_real("scatter " + case, gotd[named], ref[named], dead[idx >= 0])
    untouched = np.setdiff1d(np.arange(rows_src), named)
    assert (gotd[untouched] == SENTINEL).all()


@pytest.mark.parametrize("R,n,H", SHAPES)
def test_both_sites_off_equal_the_plain_kernels(ops, R, n, H):
    src, d, idx, rows_src = _case(R, n, H, 3)
    idx_d = torch.from_numpy(idx.astype(np.int32)).to(DEV)
    for de, dl in ((ops.NO_DROP, ops.NO_DROP), ((12345, 0), (67890, 0))):      # a seed without a threshold is no dropout
        got = _run_gather(ops, src, idx, n, de, dl)
        plain = ops.gather_rows(src.to(DEV), idx_d)
        assert torch.equal(_bits(got), _bits(plain))
        gotd = _run_scatter(ops, d, idx, rows_src, n, de, dl)
        pd = torch.full((rows_src, H), SENTINEL, dtype=BF16, device=DEV)
        ops.scatter_rows(d.to(DEV), idx_d, pd)
        assert torch.equal(_bits(gotd), _bits(pd))


def test_argument_errors_launch_nothing(ops):
    from kbner import lib as L
    lib = L.load()
    st = L.stream_ptr()
    site = (1, mmaref.dropout_thresh(0.5))
    for H, R, n in ((12, 4, 2), (16, 4, 0), (16, 7, 2), (16, 4, -1)):
        src = torch.ones(8, H, dtype=BF16, device=DEV)
        idx = torch.arange(R, dtype=I32, device=DEV)
        out = torch.full((R, H), NAN, dtype=BF16, device=DEV)
        with pytest.raises(L.KbnerError):
            ops.gather_rows_drop(src, idx, n, site, site, out=out)
        with pytest.raises(L.KbnerError):
            ops.scatter_rows_drop(src[:R].contiguous(), idx, out, n, site, site)
        # the C entry points themselves refuse (EINVAL) before any launch
        for fn in (lib.kbner_gather_rows_drop, lib.kbner_scatter_rows_drop):
            rc = fn(L.ptr(src), L.ptr(idx), L.ptr(out), R, H, n, site[0], site[1], site[0], site[1], st)
            assert rc == -22, rc
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    assert lib.kbner_gather_rows_drop(L.ptr(src), L.ptr(idx), L.ptr(out), -1, 16, 1, 1, 1, 1, 1, st) == -22
    # R = 0: returns cleanly, nothing to write
    src = torch.ones(8, 16, dtype=BF16, device=DEV)
    empty = torch.empty(0, dtype=I32, device=DEV)
    got = ops.gather_rows_drop(src, empty, 3, site, site)
    assert tuple(got.shape) == (0, 16)
    keepme = torch.full((8, 16), SENTINEL, dtype=BF16, device=DEV)
    ops.scatter_rows_drop(torch.empty(0, 16, dtype=BF16, device=DEV), empty, keepme, 3, site, site)
    torch.cuda.synchronize()
    assert (keepme == SENTINEL).all()
    # wrong dtype / a non-contiguous tensor: the usual _chk refusal
    with pytest.raises(L.KbnerError):
        ops.gather_rows_drop(src.float(), torch.arange(4, dtype=I32, device=DEV), 2, site, site)
