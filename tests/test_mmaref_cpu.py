"""CPU: the float64 references of tests/mmaref.py against torch.autograd, the bounds of its EXACT input generators, the
one-hot attention construction in float32, and the properties of its integer restatement of the dropout mask.  What
tests/test_gpu_mma_kernels.py compares the HIP kernels with is proven here, without a GPU."""
import math

import numpy as np
import pytest
import torch

import mmaref
from mmaref import D, NN, NT, TN

F64 = torch.float64


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("layout", [NT, NN, TN])
@pytest.mark.parametrize("epi", [0, 1, 1 | 4, 1 | 2, 1 | 1024, 8, 4, 1 | 4 | 128])
def test_gemm_ref_vs_torch(layout, epi):
    rng = np.random.default_rng(layout * 100 + epi)
    M, N, K = 24, 40, 56
    a, b = rng.standard_normal((M, K)), rng.standard_normal((N, K))
    A = a.T.copy() if layout == TN else a
    B = b if layout == NT else b.T.copy()
    bias, add, aux = rng.standard_normal(N), rng.standard_normal((M, N)), rng.standard_normal((M, N))
    mask = (rng.random((M, N)) < 0.5) * 2.0 if epi & 128 else None
    alpha = -0.75
    got, dgot = mmaref.gemm_ref(layout, A, B, epi, bias, add, aux, alpha, mask)
    pre = alpha * (torch.from_numpy(a) @ torch.from_numpy(b).t())
    if epi & 1:
        pre = pre + torch.from_numpy(bias)
    if mask is not None:
        pre = pre * torch.from_numpy(mask)
    if epi & 4:
        pre = pre + torch.from_numpy(add)
    if epi & 8:
        pre = pre * torch.from_numpy(aux)
    if epi & (2 | 1024):
        x = pre.clone().requires_grad_(True)
        y = torch.nn.functional.gelu(x)
        y.sum().backward()
        assert rel(got, y.detach().numpy()) < 1e-12
        if epi & 2:
            assert rel(dgot, x.grad.numpy()) < 1e-12
        else:
            assert dgot is None
    else:
        assert rel(got, pre.numpy()) < 1e-12
    ev, dev = mmaref.gemm_eval32(layout, A, B, epi, bias, add, aux, alpha, mask)
    assert ev.dtype == np.float32 and rel(ev, got) < 1e-4
    rows = np.array([0, 5, 23])
    evr, _ = mmaref.gemm_eval32(layout, A, B, epi, bias, add, aux, alpha, mask, rows=rows)
    assert np.array_equal(evr, ev[rows])


def test_erf_against_libm():
    x = np.linspace(-6, 6, 2001)
    assert max(abs(mmaref._erf(x)[i] - math.erf(x[i])) for i in range(x.size)) < 1e-15


def test_gemm_exact_generators_stay_below_2_pow_24():
    assert mmaref.gemm_exact_bound() < 2 ** 24
    out, cs = mmaref.gemm_colsum_exact_bound()
    assert out <= 256 and cs < 2 ** 24
    # the worst case itself, at the largest K: every partial sum in float32 equals the float64 one
    g = mmaref.GEMM_EXACT
    K = g["K"]
    A = np.full((2, K), float(g["ab"]))
    B = np.full((3, K), -float(g["ab"]))
    part = np.cumsum((A[:, None, :] * B[None, :, :]).astype(np.float32), axis=2, dtype=np.float32)
    assert np.array_equal(part.astype(np.float64), np.cumsum(A[:, None, :] * B[None, :, :], axis=2))
    ref, _ = mmaref.gemm_ref(NT, A, B, 1 | 4 | 8, np.full(3, -8.0), np.full((2, 3), -8.0), np.full((2, 3), 2.0), g["alpha"],
                             np.full((2, 3), g["drop_scale"]))
    assert float(np.abs(ref).max()) + g["preload"] == mmaref.gemm_exact_bound()
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    # alpha = 0.5: half-integers, still float32 values
    ref, _ = mmaref.gemm_ref(NT, A[:, :K - 1], B[:, :K - 1], 0, alpha=0.5)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    # dropout 0.5 / 0.75: the scale is exactly 2 / 4
    assert mmaref.dropout_scale(mmaref.dropout_thresh(0.5)) == 2.0 and mmaref.dropout_scale(mmaref.dropout_thresh(0.75)) == 4.0


# ------------------------------------------------------------------ attention
def _attn_autograd(qkv, mb, B, S, A, dctx, pmask):
    H = A * D
    x = torch.from_numpy(qkv).clone().requires_grad_(True)
    sp = lambda t: t.reshape(B, S, A, D).transpose(1, 2)  # noqa: E731
    q, k, v = sp(x[:, :H]), sp(x[:, H:2 * H]), sp(x[:, 2 * H:])
    sc = q @ k.transpose(-1, -2) / 8.0 + torch.from_numpy(mb).double()[:, None, None, :]
    pr = torch.softmax(sc, -1)
    if pmask is not None:
        pr = pr * torch.from_numpy(pmask)
    ctx = (pr @ v).transpose(1, 2).reshape(B * S, H)
    ctx.backward(torch.from_numpy(dctx))
    return ctx.detach().numpy(), torch.logsumexp(sc, -1).detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("drop", [False, True])
def test_attn_ref_vs_autograd(drop):
    rng = np.random.default_rng(3 + drop)
    B, S, A = 3, 64, 2
    H = A * D
    qkv, dctx = rng.standard_normal((B * S, 3 * H)), rng.standard_normal((B * S, H))
    mb = np.zeros((B, S), np.float32)
    mb[1, 40:] = -10000.0
    mb[2, 1:] = -10000.0
    pmask = (rng.random((B, A, S, S)) < 0.9) / 0.9 if drop else None
    r = mmaref.attn_ref(qkv, mb, B, S, A, dctx, pmask)
    ctx, lse, dqkv = _attn_autograd(qkv, mb, B, S, A, dctx, pmask)
    assert rel(r["ctx"], ctx) < 1e-12 and rel(r["lse"], lse) < 1e-12
    assert rel(r["dq"], dqkv[:, :H]) < 1e-12 and rel(r["dk"], dqkv[:, H:2 * H]) < 1e-12 and rel(r["dv"], dqkv[:, 2 * H:]) < 1e-12
    # the float32 evaluation models bf16 probabilities: close to the reference at that precision, both exponential paths
    keep = None if pmask is None else pmask != 0
    for use_exp2 in (True, False):
        e = mmaref.attn_eval32(qkv, mb, B, S, A, dctx, keep=keep, thresh=mmaref.dropout_thresh(0.1), use_exp2=use_exp2)
        hd = lambda t: mmaref._heads(t, B, S, A)  # noqa: E731
        assert rel(e["ctx"], hd(r["ctx"])) < 2e-2 and rel(e["lse"], r["lse"]) < 2e-3   # the row sum is the sum of the bf16 e
        assert rel(e["dq"], hd(r["dq"])) < 3e-2 and rel(e["dk"], hd(r["dk"])) < 3e-2 and rel(e["dv"], hd(r["dv"])) < 2e-2


@pytest.mark.parametrize("use_exp2", [True, False])
@pytest.mark.parametrize("S,n_real", [(512, 66), (512, 512), (64, 1), (192, 17)])
def test_onehot_attention_is_exact_in_float32(S, n_real, use_exp2):
    rng = np.random.default_rng(S + n_real)
    B, A = 1, 2
    qkv, dctx, mb, pi = mmaref.onehot_case(rng, B, S, A, None if n_real == S else [n_real])
    assert np.array_equal(mmaref.bf16_rne(qkv), qkv) and np.array_equal(mmaref.bf16_rne(dctx), dctx)
    H = A * D
    q, k = mmaref._heads(qkv[:, :H], B, S, A), mmaref._heads(qkv[:, H:2 * H], B, S, A)
    sc = q[0] @ k[0].transpose(0, 2, 1) / 8.0
    hit = np.zeros(sc.shape, bool)
    for a in range(A):
        hit[a, np.arange(S), pi[0, a]] = True
    assert (sc[hit] == mmaref.ONEHOT_HIT).all() and sc[~hit].max() <= mmaref.ONEHOT_MISS
    assert (pi[0] < n_real).all()
    # float32 softmax of these scores: exactly one non-zero probability per row, equal to 1, at pi; lse == 504
    s32 = np.float32(sc) + mb[0][None, None, :]
    mx = s32.max(-1, keepdims=True)
    if use_exp2:
        e = np.exp2((s32 - mx) * mmaref.LOG2E32)
        lse = (mx * mmaref.LOG2E32 + np.log2(e.sum(-1, keepdims=True, dtype=np.float32))) * mmaref.LN2_32
    else:
        e = np.exp(s32 - mx)
        lse = mx + np.log(e.sum(-1, keepdims=True, dtype=np.float32))
    assert e.dtype == np.float32 and np.array_equal(e, hit.astype(np.float32))
    assert (lse == np.float32(504.0)).all()
    # the evaluation that mirrors the kernels gives the expected outputs bit for bit, and P == 1 again in the backward pass
    ev = mmaref.attn_eval32(qkv, mb, B, S, A, dctx, use_exp2=use_exp2)
    ctx, dv = mmaref.onehot_expected(qkv, dctx, pi, B, S, A)
    assert np.array_equal(ev["ctx"], mmaref._heads(ctx, B, S, A)) and (ev["lse"] == 504.0).all()
    assert np.array_equal(ev["dv"], mmaref._heads(dv, B, S, A))
    assert not ev["dq"].any() and not ev["dk"].any()
    r = mmaref.attn_ref(qkv, mb, B, S, A, dctx)
    assert rel(r["ctx"], ctx) < 1e-12 and rel(r["dv"], dv) < 1e-12 and np.abs(r["lse"] - 504.0).max() < 1e-12


@pytest.mark.parametrize("case", [c for c in mmaref.ONEHOT_CASES if c[0] * c[2] <= 64], ids=str)
def test_onehot_cases_have_representable_gradients(case):
    """dV[j] = (1/(1-p)) sum of the kept dO[i] over pi(i) = j must be a bf16 value for the GPU test's equality (small cases
    here; the GPU test asserts the same precondition on every case before it looks at the kernel's output)"""
    B, S, A, ragged, _res, p = case
    qkv, dctx, mb, pi = mmaref.onehot_inputs(case)
    keep, scale = None, 1.0
    if p:
        th = mmaref.dropout_thresh(p)
        keep, scale = mmaref.dropout_keep(B * A, S, S, 99, th).reshape(B, A, S, S), float(mmaref.dropout_scale(th))
    ctx, dv = mmaref.onehot_expected(qkv, dctx, pi, B, S, A, keep, scale)
    assert np.array_equal(mmaref.bf16_rne(dv), dv) and np.array_equal(mmaref.bf16_rne(ctx), ctx)
    assert float(np.abs(dv.sum(0)).max()) < 2 ** 24
    if ragged:
        lst = mmaref.n_real_list(S)
        assert all((mb[b] == 0).sum() == lst[b % len(lst)] for b in range(B))
        assert B >= len(lst)    # every n_real of the list occurs


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("M,H", [(1, 8), (5, 504), (7, 1024)])
def test_ln_ref_vs_autograd(M, H):
    rng = np.random.default_rng(M + H)
    h, dy = rng.standard_normal((M, H)) * 2 + 0.3, rng.standard_normal((M, H))
    gamma, beta = rng.standard_normal(H) * 0.2 + 1, rng.standard_normal(H) * 0.1
    mult = (rng.random((M, H)) < 0.9) / 0.9
    r = mmaref.ln_ref(h, gamma, beta, 1e-5, dy, mult)
    ht, gt, bt = (torch.from_numpy(t).clone().requires_grad_(True) for t in (h, gamma, beta))
    y = torch.nn.functional.layer_norm(ht, (H,), gt, bt, 1e-5)
    y.backward(torch.from_numpy(dy))
    assert rel(r["y"], y.detach().numpy()) < 1e-12 and rel(r["dh"], ht.grad.numpy()) < 1e-12
    assert rel(r["dgamma"], gt.grad.numpy()) < 1e-12 and rel(r["dbeta"], bt.grad.numpy()) < 1e-12
    assert rel(r["mean"], h.mean(1)) < 1e-12 and rel(r["rstd"], 1 / np.sqrt(h.var(1) + 1e-5)) < 1e-12
    assert rel(r["dhm"], ht.grad.numpy() * mult) < 1e-12 and rel(r["dbias"], (ht.grad.numpy() * mult).sum(0)) < 1e-12
    e = mmaref.ln_eval32(h, gamma, beta, 1e-5, dy, mult)
    for k in r:
        assert e[k].dtype == np.float32 and rel(e[k], r[k]) < 1e-4, k


def test_ln_exact_case():
    rng = np.random.default_rng(0)
    for H in (8, 504, 1024):
        h, gamma, beta = mmaref.ln_exact_case(rng, 5, H)
        assert (np.abs(h) == 1).all() and (h.sum(1) == 0).all()
        for r in (mmaref.ln_ref(h, gamma, beta, 0.0), mmaref.ln_eval32(h, gamma, beta, 0.0)):
            assert (r["mean"] == 0).all() and (r["rstd"] == 1).all() and np.array_equal(r["y"], h * gamma + beta)
        assert np.array_equal(mmaref.bf16_rne(h * gamma + beta), h * gamma + beta)


# ------------------------------------------------------------------ dropout
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keep_properties(p):
    th = mmaref.dropout_thresh(p)
    Z, M, N = 3, 256, 384
    k = mmaref.dropout_keep(Z, M, N, 12345, th)
    n = k.size
    assert abs(k.mean() - (1 - p)) < 4 * math.sqrt(p * (1 - p) / n)
    assert np.array_equal(k, mmaref.dropout_keep(Z, M, N, 12345, th))              # replay
    other = mmaref.dropout_keep(Z, M, N, 12346, th)
    assert 0.2 * n * 2 * p * (1 - p) < (k != other).sum()                            # another seed: another mask
    # element (z, i, j) -> keys (z*M + i, z*N + j): slab z of a [Z, M, N] site is the block (zM.., zN..) of the flat [ZM, ZN] site
    flat = mmaref.dropout_keep(1, Z * M, Z * N, 12345, th)[0]
    for z in range(Z):
        assert np.array_equal(k[z], flat[z * M:(z + 1) * M, z * N:(z + 1) * N])
    # thresh = 1 keeps everything but a product of exactly 0; seeds with the top bit set wrap modulo 2^32
    assert mmaref.dropout_keep(1, 64, 64, 0xFFFFFFF0, 1).mean() > 0.99
    assert float(mmaref.dropout_scale(th)) == pytest.approx(1 / (1 - p), rel=1e-6)


def test_drop_mix_is_the_documented_hash():
    # lowbias32 with the constants of include/kbner.h / csrc/common.h, by hand on Python integers
    def mix(x):
        x ^= x >> 16
        x = x * 0x7feb352d & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846ca68b & 0xFFFFFFFF
        return x ^ (x >> 16)
    xs = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 123456789]
    assert [int(v) for v in mmaref.drop_mix(np.array(xs, np.uint64))] == [mix(x) for x in xs]
    seed, thresh, i, j = 0xDEADBEEF, 1 << 31, 5, 9
    key = mix((seed + i) & 0xFFFFFFFF) ^ mix(((seed * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF) ^ j)
    assert bool(mmaref.dropout_keep(1, 8, 16, seed, thresh)[0, i, j]) == (((key & 0xFFFFFF) * 0x9E3779 & 0xFFFFFFFF) >= thresh)


def test_pick_rpw_routes_named_in_the_case_list():
    assert mmaref.pick_rpw(13, 512, 2) == 128 and mmaref.pick_rpw(64, 256, 8) == 256 and mmaref.pick_rpw(64, 512, 8) == 512
    assert mmaref.pick_rpw(32, 512, 8) == 256 and mmaref.pick_rpw(64, 192, 8) == 256 and mmaref.pick_rpw(64, 384, 8) == 512
    assert {c[1] for c in mmaref.ONEHOT_CASES} == set(range(64, 513, 64))


def test_pick_rpw_never_reaches_the_forward_kernels_that_are_not_instantiated():
    """csrc/attention.hip launch_attn_fwd instantiates the 32-row forward (needs rpw % 256 == 0) only for S >= 192 and the
    persistent walk (rpw == S) only for S in {128, 256, 512}: pick_rpw offers nothing else."""
    batches = list(range(1, 600)) + [1024, 4096, 65536]
    for S in range(64, 513, 64):
        rpws = {mmaref.pick_rpw(B, S, A) for A in (1, 2, 3, 4, 8, 12, 16, 24, 32, 64) for B in batches}
        assert rpws <= {128, 256, 512}
        assert S >= 192 or not any(r % 256 == 0 for r in rpws), (S, rpws)
        assert S in (128, 256, 512) or S not in rpws, (S, rpws)


def test_e5m2_round_and_the_dropout_residual_mechanism():
    """the residual byte's rounding, and what it does in the one-hot case with dropout: the fused forward exponent leaves
    e = 1 + delta, the dropout path divides by the float32 sum of e, the residual hands O = 2 V / (1 + delta) to D -> the
    evaluation's dQ is small but NOT zero there, and exactly zero without the residual"""
    x = np.array([0, 1e-6, 1.5e-5, 2.3e-5, 0.1, 0.72, -3.3, 57344, 1e6], np.float32)
    assert np.array_equal(mmaref.e5m2_round(x), np.array([0, 0, 2.0 ** -16, 2.0 ** -15, 0.09375, 0.75, -3.5, 57344, 57344], np.float32))
    case = (13, 448, 1, True, True, 0.5)
    B, S, A = case[:3]
    qkv, dctx, mb, pi = mmaref.onehot_inputs(case)
    th = mmaref.dropout_thresh(0.5)
    keep = mmaref.dropout_keep(B * A, S, S, 99, th).reshape(B, A, S, S)
    plain = mmaref.attn_eval32(qkv, mb, B, S, A, dctx, keep=keep, thresh=th, entries=[0, 5])
    res = mmaref.attn_eval32(qkv, mb, B, S, A, dctx, keep=keep, thresh=th, entries=[0, 5], residual=True)
    assert not plain["dq"].any() and not plain["dk"].any()
    assert 0 < np.abs(res["dq"]).max() < 2e-3
    ctx, _ = mmaref.onehot_expected(qkv, dctx, pi, B, S, A, keep, 2.0)
    assert np.array_equal(mmaref.bf16_rne(res["ctx"]), mmaref._heads(ctx, B, S, A)[[0, 5]])
