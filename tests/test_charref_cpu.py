"""CPU: proves tests/charref.py -- the restatement of the character BiLSTM (csrc/char_lstm.hip) -- against torch.nn.Embedding plus a
bidirectional torch.nn.LSTM over pack_padded_sequence(enforce_sorted=False) with autograd in float64 (the model of
flair/embeddings.py:670-758): the block and every parameter gradient, with masks, dropped words and colliding character ids; the
float32 evaluation against the same; the mask against the multiplier the row kernels' reference gives for the same elements; and the
power of the comparison tests/test_gpu_char_kernels.py uses (charref.check): seven defective evaluations are refused."""
import numpy as np
import pytest
import torch

import charref as C
import mmaref
import rowref

F64 = np.float64


def torch_problem(p, chars, lens, rows, G, mask):
    """the reference's model on the words that are not dropped, loss = sum(block * mask * G) -> block, gradients by autograd"""
    V, E = p.emb.shape
    Hc = p.whh.shape[2]
    emb = torch.nn.Embedding(V, E).double()
    rnn = torch.nn.LSTM(E, Hc, num_layers=1, bidirectional=True).double()
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(p.emb))
        for d, s in enumerate(C.SFX):
            getattr(rnn, "weight_ih_l0" + s).copy_(torch.from_numpy(p.wih[d]))
            getattr(rnn, "weight_hh_l0" + s).copy_(torch.from_numpy(p.whh[d]))
            getattr(rnn, "bias_ih_l0" + s).copy_(torch.from_numpy(p.bih[d]))
            getattr(rnn, "bias_hh_l0" + s).copy_(torch.from_numpy(p.bhh[d]))
    live = np.nonzero(rows >= 0)[0]
    x = emb(torch.from_numpy(chars[live].astype(np.int64)).t())                                   # [Lmax, W', E]
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.from_numpy(lens[live].astype(np.int64)), enforce_sorted=False)
    _, (hidden, _) = rnn(packed)
    block = torch.cat([hidden[0], hidden[1]], 1)                                                   # [W', 2Hc]
    (block * torch.from_numpy(np.asarray(mask, dtype=F64)[live] * G[live])).sum().backward()
    g = {"d_emb": emb.weight.grad.numpy()}
    for name, key in (("d_wih", "weight_ih_l0"), ("d_whh", "weight_hh_l0"), ("d_bih", "bias_ih_l0"), ("d_bhh", "bias_hh_l0")):
        g[name] = np.stack([getattr(rnn, key + s).grad.numpy() for s in C.SFX])
    return live, block.detach().numpy(), g


def problem(seed, V, E, Hc, W, Lmax, n=4, col0=64, drop=True, dropped=0.25):
    rng = np.random.default_rng(seed)
    p = C.params(rng, V, E, Hc)
    chars, lens, rows = C.tables(rng, W, Lmax, V, 2 * W + 3, dropped=dropped)
    de, dl = ((11, mmaref.dropout_thresh(0.3)), (12, mmaref.dropout_thresh(0.5))) if drop else ((0, 0), (0, 0))
    G = rng.standard_normal((W, 2 * Hc))
    return C.NS(p=p, chars=chars, lens=lens, rows=rows, G=G, n=n, col0=col0, de=de, dl=dl, Hc=Hc,
                mask=C.block_mask(rows, n, col0, Hc, de, dl))


CASES = [(1, 3, 5, 7, 9, 6), (2, 40, 25, 25, 12, 5), (3, 11, 8, 6, 1, 1), (4, 5, 4, 32, 6, 3)]


@pytest.mark.parametrize("seed,V,E,Hc,W,Lmax", CASES)
def test_reference_equals_torch_autograd(seed, V, E, Hc, W, Lmax):
    q = problem(seed, V, E, Hc, W, Lmax)
    r64 = C.evaluate(q.p, q.chars, q.lens, q.rows, q.G, q.mask)
    live, block, g = torch_problem(q.p, q.chars, q.lens, q.rows, q.G, q.mask)
    assert np.isnan(r64.h[q.rows < 0]).all() and np.abs(r64.h[live] - block).max() < 1e-12
    for name, _ in C.GRADS:
        assert np.abs(getattr(r64, name) - g[name]).max() < 1e-10, name
        sa = getattr(r64, dict(C.GRADS)[name])
        assert (sa >= np.abs(g[name]) * (1 - 1e-12)).all(), name           # a sum of magnitudes bounds the sum
    assert (r64.d_bih == r64.d_bhh).all()
    # the float32 evaluation is the same formula, and passes the comparison it calibrates
    r32 = C.evaluate(q.p, q.chars, q.lens, q.rows, q.G, q.mask, f32=True)
    assert r32.h.dtype == np.float32 and r32.d_wih.dtype == np.float32
    assert np.abs(r32.h[live] - block).max() < 1e-5
    for name, _ in C.GRADS:
        assert np.abs(getattr(r32, name) - g[name]).max() < 1e-4 * max(1.0, np.abs(g[name]).max()), name


def test_mask_is_the_row_kernels_mask_of_the_same_elements():
    """block_mask(rows, n, col0) = the multiplier of sites e and l at (row, col0 + c) / (row // n, col0 + c) of an ld-wide matrix"""
    rows, n, col0, Hc, R, ld = np.array([7, 0, -1, 5, 12], np.int32), 4, 32, 9, 16, 64
    de, dl = (5, mmaref.dropout_thresh(0.25)), (9, mmaref.dropout_thresh(0.5))
    me = mmaref.dropout_mult(1, R, ld, *de)[0]
    ml = mmaref.dropout_mult(1, R // n, ld, *dl)[0]
    got = C.block_mask(rows, n, col0, Hc, de, dl)
    for w, r in enumerate(rows):
        exp = np.zeros(2 * Hc, np.float32) if r < 0 else me[r, col0:col0 + 2 * Hc] * ml[r // n, col0:col0 + 2 * Hc]
        assert (got[w] == exp).all()
    assert (C.block_mask(rows, n, col0, Hc)[rows >= 0] == 1).all()
    assert 0 < (got[rows >= 0] == 0).mean() < 1


def test_store_is_two_roundings():
    h = np.array([0.3337, -0.777, 1e-3], np.float32)
    m = np.array([2.857143, 0.0, 1.0], np.float32)
    assert (C.stored(h) == rowref.bf16_round(h)).all()
    assert (C.stored(h, m) == rowref.bf16_round(rowref.bf16_round(h) * m)).all()
    assert (C.stored(h, np.ones(3, np.float32)) == C.stored(h)).all()


def _as_got(r32):
    got = {name: getattr(r32, name) for name, _ in C.GRADS}
    got["h"] = C.stored(r32.h)
    return got


def test_check_accepts_the_float32_evaluation():
    q = problem(5, 3, 25, 25, 21, 7)
    r64 = C.evaluate(q.p, q.chars, q.lens, q.rows, q.G, q.mask)
    r32 = C.evaluate(q.p, q.chars, q.lens, q.rows, q.G, q.mask, f32=True)
    stats = {}
    C.check(_as_got(r32), r64, r32, stats=stats)
    assert set(stats) == {"h"} | {name for name, _ in C.GRADS}


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_check_refuses_defective_evaluations(defect):
    """V = 3: every character id collides; col0 != 0 with both sites on; lengths 1 .. Lmax; dropped words present"""
    q = problem(6, 3, 25, 25, 21, 7)
    assert (q.rows < 0).any() and (q.lens == 1).any() and (q.lens == 7).any() and (q.lens[q.rows >= 0] < 7).any()
    r64 = C.evaluate(q.p, q.chars, q.lens, q.rows, q.G, q.mask)
    r32 = C.evaluate(q.p, q.chars, q.lens, q.rows, q.G, q.mask, f32=True)
    mask = C.block_mask(q.rows, q.n, q.col0, q.Hc, q.de, q.dl, defect=defect)
    if defect == "dropped_contributes":
        mask = np.where((q.rows < 0)[:, None], 1.0, mask).astype(np.float32)
    bad = C.evaluate(q.p, q.chars, q.lens, q.rows, q.G, mask, f32=True, defect=defect)
    with pytest.raises(AssertionError):
        C.check(_as_got(bad), r64, r32, what=defect)
    if defect not in ("dropped_contributes",):                    # ... and by the gradients alone (h equal, or not looked at)
        got = _as_got(bad)
        got.pop("h")
        with pytest.raises(AssertionError):
            C.check(got, r64, r32, what=defect)
