"""GPU: the emission head (csrc/rows.hip: kbner_head_fwd, kbner_head_bwd_dx, kbner_head_bwd_dw) above 64 tags, through kbner.ops
against tests/rowref.py.  T in {65, 128, 137, 192}: one tag past a block of 64, two full blocks, a 33-type BIOES dictionary, the
limit; (R, H) in {(5, 128), (513, 1024), (70, 2048)}: the (row, tag) forward kernel, the row kernel (R > 512) with more than one
64-row block of the weight gradient and a partly filled last one, and the wide-row forward kernel (H > 1024; forward only:
kbner_head_bwd_dx stops at H = 1024).

"real" inputs are checked under rowref.tolerance against the float64 reference.  "exact" inputs are integers whose every partial sum
stays below 2^24, so float32 addition is exact in any order (atomics included) and the output must EQUAL the float64 result:
    head_fwd      x in [-4, 4], w in [-2, 2], b in [-8, 8] (rowref.EXACT["head_fwd"]): |sum| <= 2048 * 8 + 8
    head_bwd_dx   de, w in [-1, 1]: |sum over 192 tags| <= 192 < 256, so the bf16 output is exact too
    head_bwd_dw   de in [-1, 1], x in [-4, 4], dw pre-filled from [-8, 8]: |sum| <= 513 * 4 + 8;  db: <= 513 + 8
dw and db are pre-filled and must be added to; R = 0 touches nothing."""
import numpy as np
import pytest
import torch

import rowref
from rowref import EXACT, ints

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
NAN = float("nan")
TAGS = [65, 128, 137, 192]
K_DE, K_W, K_X, K_START = 1, 1, 4, 8          # the exact ranges of the backward cases (see the docstring)


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    return _ops


def f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


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


def check_exact(got, ref64):
    ref = np.ascontiguousarray(ref64, dtype=np.float32)
    assert np.abs(ref64).max() < rowref.EXACT_LIMIT and np.array_equal(ref.astype(np.float64), ref64)
    assert np.array_equal(host(got).reshape(ref64.shape), ref64)


def check_real(kernel, case, got, ref64, eval32, sum_abs, bf16_out=False):
    ref64 = np.asarray(ref64, np.float64)
    tol, err32 = rowref.tolerance(ref64, eval32, sum_abs, bf16_out=bf16_out)
    g = host(got).reshape(ref64.shape)
    assert np.isfinite(g).all()
    diff = np.abs(g - ref64)
    print("[headw] %s %s: kernel_err %.3e  f32_numpy_err %.3e  tolerance_share %.3f"
          % (kernel, case, float(diff.max()), err32, float((diff / np.maximum(tol, 1e-300)).max())))
    assert (diff <= tol).all(), "%s %s: worst error %.3e" % (kernel, case, float(diff.max()))


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("T", TAGS)
@pytest.mark.parametrize("R,H", [(5, 128), (513, 1024), (70, 2048)])
def test_head_fwd_wide(ops, R, H, T, kind):
    rng = np.random.default_rng(R * 7 + H + T)
    if kind == "exact":
        k = EXACT["head_fwd"][0]
        assert H <= EXACT["head_fwd"][1]
        x, w, b = ints(rng, k["x"], (R, H)), ints(rng, k["w"], (T, H)), ints(rng, k["b"], (T,))
    else:
        x, w, b = rng.standard_normal((R, H)), 0.05 * rng.standard_normal((T, H)), 0.1 * rng.standard_normal(T)
    xb, x64 = to_bf16(x)
    w, b = w.astype(np.float32), b.astype(np.float32)
    full, xd = padded(xb)                                                        # NaN rows behind R: a kernel that reads them shows
    out = ops.head_fwd(xd, f32dev(w), f32dev(b))
    assert out.shape == (R, T) and bool(torch.isfinite(out).all())
    ref = rowref.head_fwd(x64, w, b)
    if kind == "exact":
        check_exact(out, ref)
    else:
        check_real("head_fwd", "R=%d H=%d T=%d" % (R, H, T), out, ref, rowref.seq_dot32(x64, w) + b,
                   np.abs(x64) @ np.abs(w.astype(np.float64)).T + np.abs(b))


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("T", TAGS)
@pytest.mark.parametrize("R,H", [(5, 128), (513, 1024)])
def test_head_bwd_wide(ops, R, H, T, kind):
    rng = np.random.default_rng(R * 3 + H + T)
    if kind == "exact":
        assert T * K_DE * K_W < 256 and R * K_DE * K_X + K_START < rowref.EXACT_LIMIT
        de, x, w = ints(rng, K_DE, (R, T)), ints(rng, K_X, (R, H)), ints(rng, K_W, (T, H))
        dw0, db0 = ints(rng, K_START, (T, H)), ints(rng, K_START, (T,))
    else:
        de, x, w = 0.1 * rng.standard_normal((R, T)), rng.standard_normal((R, H)), 0.05 * rng.standard_normal((T, H))
        dw0, db0 = rng.standard_normal((T, H)), rng.standard_normal(T)
    xb, x64 = to_bf16(x)
    de, w, dw0, db0 = (a.astype(np.float32) for a in (de, w, dw0, db0))
    xfull, xd = padded(xb)
    defull, ded = padded(torch.from_numpy(de))
    dwfull, dw = padded(torch.from_numpy(dw0), extra=1)                          # a NaN row behind dw and an element behind db:
    dbfull, db = padded(torch.from_numpy(db0), extra=1)                          # an add behind tag T - 1 would not leave NaN alone
    dx = ops.head_bwd(ded, xd, f32dev(w), dw, db)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dwfull[T:]).all()) and bool(torch.isnan(dbfull[T:]).all())
    rdx, rdw, rdb = rowref.head_bwd(de, x64, w)
    rdw, rdb = rdw + dw0, rdb + db0                                              # accumulated INTO: not zero
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


@pytest.mark.parametrize("T", TAGS)
def test_head_wide_zero_rows_touch_nothing(ops, T):
    H = 128
    x = torch.zeros((0, H), dtype=BF16, device=DEV)
    w = torch.ones((T, H), dtype=F32, device=DEV)
    b = torch.ones(T, dtype=F32, device=DEV)
    assert ops.head_fwd(x, w, b).shape == (0, T)
    dw = torch.full((T, H), 2.5, dtype=F32, device=DEV)
    db = torch.full((T,), -1.5, dtype=F32, device=DEV)
    dx = ops.head_bwd(torch.zeros((0, T), dtype=F32, device=DEV), x, w, dw, db)
    torch.cuda.synchronize()
    assert dx.shape == (0, H) and bool((dw == 2.5).all()) and bool((db == -1.5).all())


def test_head_rejects_more_than_192_tags(ops):
    from kbner import lib as L
    R, H, T = 4, 128, 193
    x = torch.zeros((R, H), dtype=BF16, device=DEV)
    w, b = torch.zeros((T, H), dtype=F32, device=DEV), torch.zeros(T, dtype=F32, device=DEV)
    with pytest.raises(L.KbnerError, match="-22"):
        ops.head_fwd(x, w, b)
    with pytest.raises(L.KbnerError, match="-22"):
        ops.head_bwd(torch.zeros((R, T), dtype=F32, device=DEV), x, w, torch.zeros_like(w), torch.zeros_like(b))
