"""GPU: kbner_attn_rows_fwd / kbner_attn_rows_bwd (csrc/attn_rows.hip) -- attention of a few listed queries per sentence against
all its keys -- through the C ABI with test-owned, NaN-canaried buffers, against the float64 attention reference of tests/mmaref.py
restricted to the listed queries: the full reference fed a dO that is zero outside the listed rows gives dK, dV and the listed dQ;
its context rows at the listed positions are the expected ctx_c.

The bounds are those tests/test_gpu_mma_kernels.py applies to kbner_attn_fwd / kbner_attn_bwd, through its own functions: REAL cases
under check_real per (row, head) with the row's own scale -- 8 x the worst error of mmaref.attn_eval32 (the float32 evaluation with
the kernels' rounding points), plus one bf16 ulp for bf16 outputs -- and the EXACT uniform case (Q = 0, a power of two of real keys)
as equality.  The cross-check runs the full kernels on the same inputs and asserts the two implementations against each other
under the same rule.  Every check prints its figures (run with -s)."""
import math

import numpy as np
import pytest
import torch

import mmaref
import rowref
import test_gpu_mma_kernels as mk
from mmaref import D, bf16_rne

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    return _ops


def make_qpos(rng, B, S, nq):
    """[B, nq] distinct positions per sentence in random (non-monotone) order, -1 holes, the last sentence all -1"""
    qp = np.full((B, nq), -1, np.int32)
    for b in range(B - 1):
        qp[b] = rng.permutation(S)[:nq]
        if nq > 1:
            qp[b, rng.permutation(nq)[:max(1, nq // 5)]] = -1
    return qp


def make_mask(B, S):
    """sentence 0: masked tail that starts inside a 16-key fragment; sentence 1 (B >= 3): a tail aligned to the fragments"""
    mb = np.zeros((B, S), np.float32)
    mb[0, S - 21:] = -10000.0
    if B >= 3:
        mb[1, S - 32:] = -10000.0
    return mb


def run_rows(ops, qkv, mb, qp, dctx_c, B, S, A, drop):
    H = A * D
    nq = qp.shape[1]
    qd, mbd, qpd = mk.dev_bf16(qkv), mk.dev_f32(mb), torch.from_numpy(qp).to(DEV)
    R = B * nq
    ctx_c = torch.full((R + 3, H), NAN, dtype=BF16, device=DEV)
    o32 = torch.full((R + 3, H), NAN, dtype=F32, device=DEV)
    lse_c = torch.full((B * A * nq + 64,), NAN, dtype=F32, device=DEV)
    ops.attn_rows_fwd(qd, mbd, qpd, ctx_c, o32, lse_c, B, S, H, A, drop=drop)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx_c[R:]).all()) and bool(torch.isnan(o32[R:]).all()) and bool(torch.isnan(lse_c[B * A * nq:]).all())
    assert bool(torch.isfinite(ctx_c[:R]).all()) and bool(torch.isfinite(o32[:R]).all()) and bool(torch.isfinite(lse_c[:B * A * nq]).all())
    out = {"ctx": mk.host(ctx_c[:R]), "o32": mk.host(o32[:R]), "lse": mk.host(lse_c[:B * A * nq]).reshape(B, A, nq)}
    if dctx_c is None:
        return out
    dqkv = torch.full((B * S + 3, 3 * H), NAN, dtype=BF16, device=DEV)
    dbias = torch.zeros(3 * H, dtype=F32, device=DEV)
    ops.attn_rows_bwd(qd, qpd, mk.dev_bf16(dctx_c), o32, lse_c, mbd, dqkv, B, S, H, A, drop=drop, dbias=dbias)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv[B * S:]).all()), "rows >= B*S of dqkv were written"
    assert bool(torch.isfinite(dqkv[:B * S]).all())
    g = mk.host(dqkv[:B * S])
    out.update({"dq": g[:, :H], "dk": g[:, H:2 * H], "dv": g[:, 2 * H:], "dbias": mk.host(dbias)})
    return out


def _row_scale(ref, A):
    scale = np.abs(np.asarray(ref, np.float64).reshape(-1, A, D)).max(-1, keepdims=True)
    scale[scale == 0.0] = 1.0
    return scale


def check_rows(kernel, case, got, ref, ev, A, bf16_out=True, ev_ref=None):
    """[R, A * 64] arrays: every (row, head) relative to the reference row's own largest value, as test_attention_real does.
    ev: the float32 evaluation of the rows of ev_ref (default: of ref itself; a sample of batch entries, as test_attention_real
    takes one, when the whole batch would be slow)"""
    ev_ref = ref if ev_ref is None else ev_ref
    ev, ev_ref = (np.asarray(x, np.float64).reshape(-1, A, D) for x in (ev, ev_ref))
    e32 = float((np.abs(ev - ev_ref).max(-1, keepdims=True) / _row_scale(ev_ref, A)).max()) if ev_ref.size else 0.0
    got, ref = (np.asarray(x, np.float64).reshape(-1, A, D) for x in (got, ref))
    scale = _row_scale(ref, A)
    mk.check_real(kernel, case, got / scale, ref / scale, e32, 1.0, bf16_out=bf16_out, got_is_numpy=True)


CASES = [(B, S, A, nq, p) for (B, S, A) in ((2, 64, 2), (3, 192, 2), (2, 512, 2)) for nq in (1, 16, 17, 40) for p in (0.0, 0.1)]
# Enough heads for kbner_attn_fwd / _bwd to take their 32-row kernels (a row tile of 256, mmaref.pick_rpw -- asserted below): the
# few-query kernels then follow THAT arithmetic -- forward maxima per half of the keys with the online-softmax step (no dropout),
# backward probabilities from accumulators started at -lse / scale -- which is what the benchmark shape runs.  The float32
# evaluation is taken on a sample of batch entries, as test_attention_real does.
ROUTE_CASES = [(32, 512, 8, 16, 0.0), (32, 512, 8, 17, 0.1), (64, 256, 8, 40, 0.0), (64, 256, 8, 16, 0.1)]


@pytest.mark.parametrize("B,S,A,nq,p", CASES + ROUTE_CASES)
def test_attn_rows_real(ops, B, S, A, nq, p):
    H = A * D
    routes = (B, S, A, nq, p) in ROUTE_CASES
    assert (mmaref.pick_rpw(B, S, A) % 256 == 0) == routes
    rng = np.random.default_rng(B * 1009 + S * 7 + nq * 131 + int(p * 100))
    qkv = bf16_rne(rng.standard_normal((B * S, 3 * H)))
    dfull = bf16_rne(rng.standard_normal((B * S, H)))
    mb = make_mask(B, S)
    qp = make_qpos(rng, B, S, nq)
    listed = [(b, i, int(qp[b, i])) for b in range(B) for i in range(nq) if qp[b, i] >= 0]
    lrow = np.array([b * nq + i for b, i, _ in listed], np.int64)         # rows of the compact arrays
    frow = np.array([b * S + pos for b, _, pos in listed], np.int64)      # the same queries' rows of the full arrays
    dctx_c = np.zeros((B * nq, H))
    dctx_c[lrow] = dfull[frow]
    dmasked = np.zeros_like(dfull)
    dmasked[frow] = dfull[frow]
    keep, pmask, drop = None, None, (0, 0)
    if p:
        drop = (424242, mmaref.dropout_thresh(p))
        keep = mmaref.dropout_keep(B * A, S, S, *drop).reshape(B, A, S, S)
        pmask = keep.astype(np.float32) * mmaref.dropout_scale(drop[1])
    ref = mmaref.attn_ref(qkv, mb, B, S, A, dmasked, pmask)
    ne = 3 if routes else B            # the batch entries the float32 evaluation covers: the leading ne
    ev = mmaref.attn_eval32(qkv, mb, B, S, A, dmasked, keep=keep, thresh=drop[1], entries=range(ne))
    evr = {n: mmaref._rows(np.ascontiguousarray(ev[n].astype(np.float64)), ne, S, A) for n in ("ctx", "dq", "dk", "dv")}
    refe = {n: ref[n][:ne * S] for n in evr}
    sel = frow[frow < ne * S]          # the listed queries among them
    r = run_rows(ops, qkv, mb, qp, dctx_c, B, S, A, drop)
    cs = "B=%d S=%d A=%d nq=%d p=%g" % (B, S, A, nq, p)
    sfx = " dropout" if p else ""
    # forward: listed rows against the reference's rows, the others exactly zero
    unl = np.setdiff1d(np.arange(B * nq), lrow)
    assert not r["ctx"][unl].any() and not r["o32"][unl].any(), cs + ": a row without a query is not zero"
    check_rows("attn_rows ctx (bf16)" + sfx, cs, r["ctx"][lrow], ref["ctx"][frow], evr["ctx"][sel], A, ev_ref=ref["ctx"][sel])
    check_rows("attn_rows o32" + sfx, cs, r["o32"][lrow], ref["ctx"][frow], evr["ctx"][sel], A, bf16_out=False, ev_ref=ref["ctx"][sel])
    lse_ref = np.array([[ref["lse"][b, a, pos] for a in range(A)] for b, _, pos in listed]).reshape(-1, A)
    lse_e32 = max([abs(float(ev["lse"][b, a, pos]) - ref["lse"][b, a, pos]) for b, _, pos in listed if b < ne for a in range(A)], default=0.0)
    lse_got = np.array([[r["lse"][b, a, i] for a in range(A)] for b, i, _ in listed]).reshape(-1, A)
    mk.check_real("attn_rows lse", cs, lse_got, lse_ref, lse_e32, np.abs(lse_ref) + 8.0, got_is_numpy=True)
    # backward: the Q third of every unlisted row is exactly zero; listed dQ, every dK and dV row against the reference
    unlf = np.setdiff1d(np.arange(B * S), frow)
    assert not r["dq"][unlf].any(), cs + ": the Q third of an unlisted row is not zero"
    check_rows("attn_rows dq (bf16)" + sfx, cs, r["dq"][frow], ref["dq"][frow], evr["dq"][sel], A, ev_ref=ref["dq"][sel])
    check_rows("attn_rows dk (bf16)" + sfx, cs, r["dk"], ref["dk"], evr["dk"], A, ev_ref=refe["dk"])
    check_rows("attn_rows dv (bf16)" + sfx, cs, r["dv"], ref["dv"], evr["dv"], A, ev_ref=refe["dv"])
    last = slice((B - 1) * S, B * S)   # the sentence whose list is all -1: zeros, written
    assert not r["dq"][last].any() and not r["dk"][last].any() and not r["dv"][last].any()
    bsum = np.concatenate([ref[n].sum(0) for n in ("dq", "dk", "dv")])
    esum = np.concatenate([evr[n].sum(0) for n in ("dq", "dk", "dv")])
    rsum = np.concatenate([refe[n].sum(0) for n in ("dq", "dk", "dv")])
    sabs = np.concatenate([np.abs(ref[n]).sum(0) for n in ("dq", "dk", "dv")])
    mk.check_real("attn_rows dbias", cs, r["dbias"], bsum, float(np.abs(esum - rsum).max()) * B / ne, sabs, got_is_numpy=True)
    # cross-check: the full kernels fed the dO that is zero outside the listed rows
    full = mk._run_attention(ops, qkv, dmasked, mb, B, S, A, True, drop)
    # (the full kernels' output stands in for the reference; the float32 evaluation's error is carried over row by row)
    for n, rows, erows in (("dq", frow, sel), ("dk", slice(None), slice(0, ne * S)), ("dv", slice(None), slice(0, ne * S))):
        check_rows("attn_rows vs full %s (bf16)%s" % (n, sfx), cs, r[n][rows], full[n][rows],
                   full[n][erows] + (evr[n][erows] - ref[n][erows]), A, ev_ref=full[n][erows])


@pytest.mark.parametrize("B,S,A,n_real,nq", [(2, 64, 2, 16, 5), (3, 192, 2, 64, 17), (2, 512, 2, 256, 40), (2, 512, 2, 512, 16),
                                                (32, 512, 8, 256, 16), (64, 256, 8, 64, 17)])   # (the last two: the two-part forward)
def test_attn_rows_exact_uniform(ops, B, S, A, n_real, nq):
    """Q = 0 and a power of two of real keys: every real key has probability 1 / n_real exactly, so a listed context row EQUALS
    bf16(mean of the real V rows) for integer V (o32: the mean itself), and lse is log(n_real) to one float32 ulp"""
    H = A * D
    rng = np.random.default_rng(B + S + n_real + nq)
    qkv = np.zeros((B * S, 3 * H))
    qkv[:, H:] = mmaref.ints(rng, 4, (B * S, 2 * H))
    mb = np.zeros((B, S), np.float32)
    mb[:, n_real:] = -10000.0
    qp = make_qpos(rng, B, S, nq)
    r = run_rows(ops, qkv, mb, qp, None, B, S, A, (0, 0))
    mean = qkv[:, 2 * H:].reshape(B, S, H)[:, :n_real].sum(1) / n_real
    want = np.where((qp >= 0)[:, :, None], mean[:, None, :], 0.0).reshape(B * nq, H)
    assert np.array_equal(r["o32"], want)
    assert np.array_equal(r["ctx"], bf16_rne(want))
    ref = np.float32(math.log(n_real))
    lse = r["lse"].transpose(0, 2, 1)[qp >= 0]
    assert (np.abs(lse - float(ref)) <= float(np.spacing(ref))).all()
    assert (r["lse"].transpose(0, 2, 1)[qp < 0] == 0.0).all()
