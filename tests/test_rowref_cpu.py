"""CPU: the float64 references of tests/rowref.py are right -- head_*, embed_ln_* and colsum against torch.autograd in
float64 on Linear and Embedding + Embedding + LayerNorm, adamw_hf against oracle/optim.py -- and the integer-valued inputs
of the exact GPU cases (tests/test_gpu_row_kernels.py) cannot leave the range in which float32 addition is exact."""
import math

import numpy as np
import pytest
import torch

import rowref

REL = 1e-12


def _close(got, ref, rel=REL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert float(np.abs(got - ref).max()) <= rel * max(float(np.abs(ref).max()), 1e-300)


@pytest.mark.parametrize("R,H,T", [(1, 8, 1), (37, 264, 29), (130, 1032, 64)])
def test_head_against_autograd_linear(R, H, T):
    g = torch.Generator().manual_seed(R)
    lin = torch.nn.Linear(H, T).double()
    x = torch.randn(R, H, generator=g, dtype=torch.float64, requires_grad=True)
    de = torch.randn(R, T, generator=g, dtype=torch.float64)
    out = lin(x)
    out.backward(de)
    w, b = lin.weight.detach().numpy(), lin.bias.detach().numpy()
    _close(rowref.head_fwd(x.detach().numpy(), w, b), out.detach().numpy())
    dx, dw, db = rowref.head_bwd(de.numpy(), x.detach().numpy(), w)
    _close(dx, x.grad.numpy())
    _close(dw, lin.weight.grad.numpy())
    _close(db, lin.bias.grad.numpy())
    # colsum is the bias gradient of a Linear: the column sums of the incoming gradient
    _close(rowref.colsum(de.numpy()), lin.bias.grad.numpy())


@pytest.mark.parametrize("M,H,eps,drop", [(1, 8, 1e-5, False), (67, 128, 1e-12, True), (300, 264, 1e-5, True)])
def test_embed_ln_against_autograd(M, H, eps, drop):
    V, P = 50, 20
    g = torch.Generator().manual_seed(M)
    word = torch.nn.Embedding(V, H).double()
    pos = torch.nn.Embedding(P, H).double()
    ln = torch.nn.LayerNorm(H, eps=eps).double()
    type0 = torch.randn(H, generator=g, dtype=torch.float64, requires_grad=True)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.3 * torch.randn(H, generator=g, dtype=torch.float64))
        ln.bias.copy_(0.2 * torch.randn(H, generator=g, dtype=torch.float64))
    ids = torch.randint(0, V // 2, (M,), generator=g)        # repeats; the upper half of the table is never named
    pids = torch.randint(0, P, (M,), generator=g)
    mult = (torch.rand(M, H, generator=g, dtype=torch.float64) > 0.1).double() / 0.9 if drop else None
    dy = torch.randn(M, H, generator=g, dtype=torch.float64)
    h0 = (word(ids) + pos(pids)) + type0
    h0.retain_grad()
    y = ln(h0)
    if drop:
        y = y * mult
    y.backward(dy)

    n = lambda t: t.detach().numpy()  # noqa: E731
    mnp = n(mult) if drop else None
    r_h0, r_y, r_mean, r_rstd = rowref.embed_ln_fwd(n(ids), n(pids), n(word.weight), n(pos.weight), n(type0), n(ln.weight), n(ln.bias),
                                                    eps, mult=mnp)
    _close(r_h0, n(h0))
    _close(r_y, n(y))
    _close(r_mean, n(h0).mean(1))
    _close(r_rstd, 1.0 / np.sqrt(n(h0).var(1) + eps))
    # normalising a given matrix instead of the sum: the same function of that matrix
    alt = np.round(n(h0) * 64.0) / 64.0
    _, a_y, a_mean, _ = rowref.embed_ln_fwd(n(ids), n(pids), n(word.weight), n(pos.weight), n(type0), n(ln.weight), n(ln.bias), eps, h0=alt)
    _close(a_mean, alt.mean(1))
    _close(a_y, n(torch.nn.functional.layer_norm(torch.from_numpy(alt), (H,), ln.weight, ln.bias, eps)))

    b = rowref.embed_ln_bwd(n(dy), r_h0, r_mean, r_rstd, n(ln.weight), n(ids), n(pids), V, P, mult=mnp)
    rel = REL
    _close(b["dh"], n(h0.grad), rel)
    _close(b["dgamma"], n(ln.weight.grad), rel)
    _close(b["dbeta"], n(ln.bias.grad), rel)
    _close(b["dword"], n(word.weight.grad), rel)
    _close(b["dpos"], n(pos.weight.grad), rel)
    _close(b["dtype0"], n(type0.grad), rel)
    named = np.zeros(V, bool)
    named[n(ids)] = True
    assert np.array_equal(b["flags"], np.where(named, 3, 0).astype(np.uint8))
    assert not b["dword"][~named].any()


def test_row_moves():
    rng = np.random.default_rng(0)
    src = rng.standard_normal((9, 4))
    idx = np.array([3, -1, 0, 8, -1, 3])
    out = rowref.gather(src, idx)
    for r, s in enumerate(idx):
        assert np.array_equal(out[r], src[s] if s >= 0 else np.zeros(4))
    # gather is the index_select of torch behind a mask
    t = torch.from_numpy(src).index_select(0, torch.from_numpy(np.maximum(idx, 0))) * torch.from_numpy((idx >= 0)[:, None].astype(np.float64))
    assert np.array_equal(out, t.numpy())
    rows = rng.standard_normal((4, 4))
    uidx = np.array([7, -1, 2, 0])
    dst = rng.standard_normal((9, 4))
    sc = rowref.scatter(dst, rows, uidx)
    exp = dst.copy()
    for r, d in enumerate(uidx):
        if d >= 0:
            exp[d] = rows[r]
    assert np.array_equal(sc, exp)
    # scatter_add is the backward of gather: torch.index_add_
    ridx = np.array([7, -1, 2, 7])
    sa = rowref.scatter_add(dst, rows, ridx)
    keep = ridx >= 0
    exp = torch.from_numpy(dst.copy()).index_add_(0, torch.from_numpy(ridx[keep]), torch.from_numpy(rows[keep])).numpy()
    _close(sa, exp)


@pytest.mark.parametrize("wd,scale,clip", [(0.0, 1.0, False), (0.0, 1.0, True), (0.01, 0.25, True), (0.01, 1.0, False)])
def test_adamw_against_oracle(wd, scale, clip):
    from oracle import optim as oopt
    rng = np.random.default_rng(3)
    n = 4160
    lr = 1e-3
    p = rng.standard_normal(n)
    m = np.zeros(n)
    v = np.zeros(n)
    op, om, ov = p.copy(), m.copy(), v.copy()
    for step in range(1, 4):
        g = rng.standard_normal(n) * (3.0 if clip and step == 2 else 0.01)
        nsq = float((g * g).sum())
        bc = math.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step)
        p, m, v, shadow = rowref.adamw_hf(p, g, m, v, lr * bc, lr * wd, 0.9, 0.999, 1e-6, nsq, 5.0, scale, n_shadow=n - 4)
        ge = g * scale
        coef = oopt.clip_coef(float(np.sqrt((ge * ge).sum())), 5.0)
        if clip and step == 2:
            assert coef < 1.0
        oopt.adamw_hf_step(op, ge * coef, om, ov, step, lr, wd=wd)
        # the oracle rounds b1, 1 - b1, b2, 1 - b2, eps and the step size to float32 before it uses them: 2^-24 relative each
        _close(p, op, 1e-6)
        _close(m, om, 1e-6)
        _close(v, ov, 1e-6)
        assert shadow.shape == (n - 4,)
        assert np.array_equal(shadow, torch.from_numpy(p.astype(np.float32)[:n - 4]).bfloat16().float().numpy())
    # no clipping without a norm, whatever the gradient
    g = rng.standard_normal(n) * 30.0
    a = rowref.adamw_hf(p, g, m, v, lr, 0.0, gnorm_sq=None)[0]
    b = rowref.adamw_hf(p, g, m, v, lr, 0.0, gnorm_sq=1e-12)[0]
    assert np.array_equal(a, b)
    assert rowref.sqnorm(g) == pytest.approx(float(np.dot(g, g)), rel=1e-14)
    w = rng.standard_normal(33)
    assert rowref.wdiff_sum(g[:33], p[:33], w) == pytest.approx(float(np.dot(w, g[:33] - p[:33])), rel=1e-13)
    assert rowref.wdiff_sum(g[:0], p[:0], w[:0]) == 0.0


@pytest.mark.parametrize("name", sorted(rowref.EXACT))
def test_exact_inputs_stay_below_2_to_24(name):
    """the largest partial sum an exact case can reach is a float32 integer"""
    assert rowref.exact_bound(name) < rowref.EXACT_LIMIT
    ranges = rowref.EXACT[name][0]
    rng = np.random.default_rng(0)
    for k in ranges.values():
        x = rowref.ints(rng, k, (4096,))
        assert float(np.abs(x).max()) <= k and np.array_equal(x, np.round(x))
        assert k <= 256                                       # bf16 holds the integers up to 256
        assert np.array_equal(rowref.bf16_round(x.astype(np.float32)), x.astype(np.float32))
    if name == "head_bwd_dx":
        assert rowref.exact_bound(name) <= 256                # dx is stored as bf16


def test_tolerance_rule():
    ref = np.array([1.0, -2.0, 0.0])
    ev = ref + np.array([1e-7, 0.0, -3e-7])
    tol, err = rowref.tolerance(ref, ev, np.array([4.0, 4.0, 0.0]))
    assert err == pytest.approx(3e-7)
    assert np.allclose(tol, 8 * 3e-7)
    tol, _ = rowref.tolerance(ref, ref, np.array([4.0, 4.0, 0.0]), bf16_out=True)      # exact float32 evaluation: the floor
    assert np.allclose(tol, 2 * 2.0 ** -24 * np.array([4.0, 4.0, 0.0]) + 2.0 ** -8 * np.abs(ref))
    # sequential float32 helpers: the plain loops they stand for
    rng = np.random.default_rng(1)
    a = rng.standard_normal((5, 70)).astype(np.float32)
    b = rng.standard_normal((3, 70)).astype(np.float32)
    acc = np.zeros((5, 3), np.float32)
    s = np.zeros(5, np.float32)
    for k in range(70):
        acc += a[:, k, None] * b[None, :, k]
        s += a[:, k]
    assert np.array_equal(rowref.seq_dot32(a, b), acc)
    assert np.array_equal(rowref.seq_sum32(a, 1), s)
