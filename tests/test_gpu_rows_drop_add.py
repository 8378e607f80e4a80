"""GPU: kbner_rows_drop_add (csrc/rows.hip) -- hidden dropout on compact rows, row r drawing the mask bits of row row_ids[r] of the
full hidden state.  The keep pattern EQUALS kbner_dropout_mask at row_ids (and mmaref.dropout_keep, the integer restatement of the
contract) bit for bit; with integer-valued inputs and p = 0.5 (scale exactly 2) every float32 intermediate is an integer, so the
output EQUALS the float64 formula bit for bit."""
import numpy as np
import pytest
import torch

import mmaref
from mmaref import bf16_rne

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")


def _row_ids(rng, R, M):
    ids = rng.permutation(M)[:R].astype(np.int32)
    ids[rng.permutation(R)[:max(1, R // 7)]] = -1
    return ids


@pytest.mark.parametrize("R,H,M,p,y32", [(5, 64, 300, 0.1, True), (37, 1024, 131072, 0.1, False), (300, 128, 512, 0.5, True),
                                         (64, 256, 70000, 0.1, True)])
def test_keep_pattern_is_the_full_rows(R, H, M, p, y32):
    from kbner import ops
    rng = np.random.default_rng(R + H)
    seed, thresh = 0x9E3779B9 ^ R, mmaref.dropout_thresh(p)
    ids = _row_ids(rng, R, M)
    y = torch.ones((R, H), dtype=F32 if y32 else BF16, device=DEV)
    out = torch.full((R + 3, H), NAN, dtype=BF16, device=DEV)
    ops.rows_drop_add(y, torch.from_numpy(ids).to(DEV), out, (seed, thresh))
    full = ops.dropout_mask(1, M, H, seed, thresh)[0]                       # [M, H] multipliers of the full hidden state
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[R:]).all())
    got = out[:R].float().cpu().numpy()
    want = full.cpu().numpy()[np.maximum(ids, 0)]
    want[ids < 0] = 1.0                                                     # no row, no mask
    assert np.array_equal(got != 0.0, want != 0.0)
    assert np.array_equal(got, bf16_rne(want.astype(np.float64)).astype(np.float32))
    keep = mmaref.dropout_keep(1, M, H, seed, thresh)[0][np.maximum(ids, 0)]
    assert np.array_equal((got != 0.0)[ids >= 0], keep[ids >= 0])


@pytest.mark.parametrize("y32,bias,addend", [(True, True, True), (True, False, False), (False, False, False), (False, False, True)])
def test_values_exact(y32, bias, addend):
    from kbner import ops
    R, H, M = 41, 192, 5000
    rng = np.random.default_rng(7 + y32 + 2 * bias + 4 * addend)
    seed, thresh = 20220711, mmaref.dropout_thresh(0.5)
    assert float(mmaref.dropout_scale(thresh)) == 2.0
    ids = _row_ids(rng, R, M)
    y = mmaref.ints(rng, 8, (R, H))
    bv = mmaref.ints(rng, 8, H) if bias else None
    av = mmaref.ints(rng, 8, (R, H)) if addend else None
    yd = torch.from_numpy(y.astype(np.float32)).to(F32 if y32 else BF16).to(DEV)
    out = torch.full((R + 3, H), NAN, dtype=BF16, device=DEV)
    ops.rows_drop_add(yd, torch.from_numpy(ids).to(DEV), out, (seed, thresh),
                      bias=None if bv is None else torch.from_numpy(bv.astype(np.float32)).to(DEV),
                      addend=None if av is None else torch.from_numpy(av.astype(np.float32)).to(BF16).to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[R:]).all())
    mult = mmaref.dropout_mult(1, M, H, seed, thresh)[0].astype(np.float64)[np.maximum(ids, 0)]
    mult[ids < 0] = 1.0
    want = (y + (bv[None, :] if bias else 0.0)) * mult + (av if addend else 0.0)
    assert np.array_equal(bf16_rne(want), want)      # precondition of the equality: the expected values are bf16 values
    assert np.array_equal(out[:R].float().cpu().numpy().astype(np.float64), want)


@pytest.mark.parametrize("R,H,M", [(37, 128, 600), (300, 1024, 4096)])
def test_ln_bwd_rows_draws_the_original_rows_bits(R, H, M):
    """kbner_ln_bwd_rows on compact rows against kbner_ln_bwd on the FULL rows (the compact rows at row_ids, zero dy elsewhere),
    same site: dh and dhm of compact row r EQUAL those of full row row_ids[r] bit for bit -- the mask is applied to the same fp32
    dh with the bits of the original row -- the keep pattern is kbner_dropout_mask's at row_ids, and dgamma / dbeta / dbias agree
    to the order of their float32 sums."""
    from kbner import ops
    rng = np.random.default_rng(R + H)
    seed, thresh = 0x51ED270B ^ R, mmaref.dropout_thresh(0.1)
    ids = rng.permutation(M)[:R].astype(np.int32)          # (every compact row has an original row here: -1 rows carry dy = 0)
    ids_d = torch.from_numpy(ids).to(DEV)
    h_c = torch.from_numpy(rng.standard_normal((R, H)).astype(np.float32)).to(BF16).to(DEV)
    dy_c = torch.from_numpy(rng.standard_normal((R, H)).astype(np.float32)).to(BF16).to(DEV)
    gamma = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)).to(DEV)
    beta = torch.zeros(H, dtype=F32, device=DEV)
    h_f = torch.from_numpy(rng.standard_normal((M, H)).astype(np.float32)).to(BF16).to(DEV)
    h_f[ids_d.long()] = h_c
    dy_f = torch.zeros((M, H), dtype=BF16, device=DEV)
    dy_f[ids_d.long()] = dy_c

    def stats(h):
        y, mean, rstd = torch.empty_like(h), torch.empty(h.shape[0], dtype=F32, device=DEV), torch.empty(h.shape[0], dtype=F32, device=DEV)
        ops.ln_fwd(h, gamma, beta, 1e-5, y, mean, rstd)
        return mean, rstd

    def run(dy, h, row_ids):
        mean, rstd = stats(h)
        n = h.shape[0]
        dh, dhm = torch.full((n + 3, H), NAN, dtype=BF16, device=DEV), torch.full((n + 3, H), NAN, dtype=BF16, device=DEV)
        acc = torch.zeros((3, H), dtype=F32, device=DEV)
        ops.ln_bwd(dy, h, mean, rstd, gamma, dh[:n], acc[0], acc[1], acc[2], dhm=dhm[:n], drop=(seed, thresh), row_ids=row_ids)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dh[n:]).all()) and bool(torch.isnan(dhm[n:]).all())
        return dh[:n], dhm[:n], acc

    dh_c, dhm_c, acc_c = run(dy_c, h_c, ids_d)
    dh_f, dhm_f, acc_f = run(dy_f, h_f, None)
    assert torch.equal(dh_c, dh_f[ids_d.long()]) and torch.equal(dhm_c, dhm_f[ids_d.long()])
    mask = ops.dropout_mask(1, M, H, seed, thresh)[0][ids_d.long()]
    live = dh_c.float() != 0
    assert bool(((dhm_c.float() != 0) == ((mask != 0) & live)).all()) and bool((mask == 0).any())
    assert torch.allclose(acc_c, acc_f, rtol=1e-4, atol=1e-4 * float(acc_f.abs().max()))
