"""TEST INFRASTRUCTURE: a plain restatement of the character BiLSTM of FastCharacterEmbeddings (csrc/char_lstm.hip:
kbner_char_lstm_fwd, kbner_char_lstm_bwd), written from the formulas in include/kbner.h (numpy only, no kernel structure: no waves, no
LDS images, no summation order).  tests/test_charref_cpu.py proves it against torch.nn.Embedding + a bidirectional torch.nn.LSTM over
pack_padded_sequence(enforce_sorted=False) with autograd; tests/test_gpu_char_kernels.py compares the HIP kernels with it.

    evaluate(p, chars, lens, rows, dout, mask)            float64: the block before the bf16 store, every gradient, and the first-order
                                                          sum_abs bounds rowref.tolerance takes
    evaluate(..., f32=True)                               the same formulas in plain float32 with sequential sums
    block_mask(rows, n, col0, Hc, drop_e, drop_l)         the multiplier of the head's two pre-RNN dropout sites on the block
    stored(h, mask)                                       what the kernel stores: bf16(bf16(h) * mask), as float32

Masks: m = m_e * m_l formed in float32; element site keyed (row, col0 + c), locked site (row // n, col0 + c): the keys of
kbner_gather_rows_drop for the same element of the ld-wide matrix.  rows[w] == -1: the word is dropped -- no output, no gradient.

`defect` names one wrong evaluation (DEFECTS); test_charref_cpu.py shows that the comparison refuses each of them.
"""
import types

import numpy as np

import mmaref
import rowref

F64, F32 = np.float64, np.float32
NS = types.SimpleNamespace
SFX = ("", "_reverse")
DEFECTS = ("bwd_not_reversed", "final_at_lmax", "gate_order", "mask_block_col", "emb_overwrite", "no_bias_hh", "dropped_contributes")


def params(rng, V, E, Hc, scale=1.0):
    """emb [V, E], wih [2, 4Hc, E], whh [2, 4Hc, Hc], bih / bhh [2, 4Hc]: float32-representable float64 values"""
    def draw(*shape):
        return (rng.standard_normal(shape) * scale).astype(F32).astype(F64)
    k = 1.0 / np.sqrt(Hc)
    return NS(emb=draw(V, E), wih=draw(2, 4 * Hc, E) * 1.0, whh=(draw(2, 4 * Hc, Hc) * k).astype(F32).astype(F64),
              bih=draw(2, 4 * Hc), bhh=draw(2, 4 * Hc))


def tables(rng, W, Lmax, V, n_rows, dropped=0.0):
    """chars [W, Lmax], lens [W] (1 and Lmax both present when W >= 2), rows [W]: unique, non-contiguous, some -1"""
    lens = rng.integers(1, Lmax + 1, size=W)
    lens[0] = Lmax
    if W >= 2:
        lens[-1] = 1
    chars = rng.integers(0, V, size=(W, Lmax))
    for w in range(W):
        chars[w, lens[w]:] = 0
    rows = rng.permutation(n_rows)[:W].astype(np.int64)
    if dropped:
        rows[rng.random(W) < dropped] = -1
    return chars.astype(np.int32), lens.astype(np.int32), rows.astype(np.int32)


def block_mask(rows, n, col0, Hc, drop_e=(0, 0), drop_l=(0, 0), defect=None):
    """float32 [W, 2Hc]: m_e[row, col0 + c] * m_l[row // n, col0 + c] (rows of dropped words: 0)"""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.arange(2 * Hc, dtype=np.uint64) + np.uint64(0 if defect == "mask_block_col" else col0)
    M32 = np.uint64(0xFFFFFFFF)

    def site(pair, keys):
        seed, thresh = int(pair[0]) & 0xFFFFFFFF, int(pair[1])
        rk = mmaref.drop_mix((keys.astype(np.uint64) + np.uint64(seed)) & M32)
        ck = mmaref.drop_mix(np.uint64((seed * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF) ^ cols)
        x = (rk[:, None] ^ ck[None, :]) & np.uint64(0xFFFFFF)
        return ((x * np.uint64(0x9E3779)) & M32) >= np.uint64(thresh)

    live = rows >= 0
    r = np.where(live, rows, 0)
    keep = site(drop_e, r) & site(drop_l, r // int(n)) & live[:, None]
    scale = F32(mmaref.dropout_scale(drop_e[1])) * F32(mmaref.dropout_scale(drop_l[1]))
    return keep.astype(F32) * scale


def stored(h, mask=None):
    """the kernel's store: one rounding of h to bf16, the mask multiplies the rounded value in float32, one more rounding"""
    v = rowref.bf16_round(np.asarray(h, dtype=F32))
    if mask is not None:
        v = rowref.bf16_round(v * np.asarray(mask, dtype=F32))
    return v


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _dot(a, b, f32):
    """a [R, K] . b [N, K]^T;  float32: one rank-1 update per k"""
    return rowref.seq_dot32(a, b) if f32 else a @ b.T


def evaluate(p, chars, lens, rows, dout=None, mask=None, f32=False, defect=None):
    """-> NS(h [W, 2Hc] before the store (NaN for dropped words), sa_h; with dout [W, 2Hc] (gradient of the MASKED block as stored,
    any values at dropped words): d_emb, d_wih, d_whh, d_bih, d_bhh and sa_* of each).  float64, or float32 with sequential sums."""
    T = F32 if f32 else F64
    emb, wih, whh, bih, bhh = (np.asarray(a, dtype=T) for a in (p.emb, p.wih, p.whh, p.bih, p.bhh))
    chars, lens, rows = np.asarray(chars), np.asarray(lens), np.asarray(rows)
    W, Lmax = chars.shape
    E, Hc = emb.shape[1], whh.shape[2]
    live = rows >= 0
    if defect == "dropped_contributes":
        live = np.ones(W, bool)
    order = [0, 1, 2, 3] if defect != "gate_order" else [0, 2, 1, 3]
    gate = [slice(q * Hc, (q + 1) * Hc) for q in order]
    res = NS(h=np.full((W, 2 * Hc), np.nan, T), sa_h=np.zeros((W, 2 * Hc)))
    if dout is not None:
        res.d_emb, res.sa_emb = np.zeros(emb.shape, T), np.zeros(emb.shape)
        res.d_wih, res.sa_wih = np.zeros(wih.shape, T), np.zeros(wih.shape)
        res.d_whh, res.sa_whh = np.zeros(whh.shape, T), np.zeros(whh.shape)
        res.d_bih, res.d_bhh, res.sa_b = np.zeros(bih.shape, T), np.zeros(bih.shape, T), np.zeros(bih.shape)
        m = np.ones((W, 2 * Hc), T) if mask is None else np.asarray(mask, dtype=T)
    t_idx = np.arange(Lmax)[None, :]
    for d in range(2):
        fin = np.full(W, Lmax) if defect == "final_at_lmax" else lens
        pos = t_idx if (d == 0 or defect == "bwd_not_reversed") else fin[:, None] - 1 - t_idx
        act = (t_idx < fin[:, None]) & live[:, None]
        ids = np.where(act, chars[np.arange(W)[:, None], np.clip(pos, 0, Lmax - 1)], 0)
        bias = bih[d] + bhh[d]
        aW, aU = np.abs(wih[d]).astype(F64), np.abs(whh[d]).astype(F64)
        h, c = np.zeros((W, Hc), T), np.zeros((W, Hc), T)
        sah, sac = np.zeros((W, Hc)), np.zeros((W, Hc))
        sv = []
        for t in range(Lmax):
            a_ = act[:, t, None]
            x = emb[ids[:, t]]
            pre = (bias[None, :] + _dot(x, wih[d], f32)) + _dot(h, whh[d], f32)
            sap = np.abs(bih[d]) + np.abs(bhh[d]) + np.abs(x).astype(F64) @ aW.T + (np.abs(h).astype(F64) + sah) @ aU.T
            ig, fg, gg, og = _sig(pre[:, gate[0]]), _sig(pre[:, gate[1]]), np.tanh(pre[:, gate[2]]), _sig(pre[:, gate[3]])
            cn = fg * c + ig * gg
            tc = np.tanh(cn)
            hn = og * tc
            e = NS(i=ig * (1 - ig) * sap[:, gate[0]], f=fg * (1 - fg) * sap[:, gate[1]], g=(1 - gg * gg) * sap[:, gate[2]],
                   o=og * (1 - og) * sap[:, gate[3]], cp=sac)
            sacn = fg * sac + np.abs(c) * e.f + np.abs(gg) * e.i + ig * e.g + np.abs(fg * c) + np.abs(ig * gg)
            e.c, e.tc = sacn, (1 - tc * tc) * sacn
            sahn = np.abs(tc) * e.o + og * e.tc + np.abs(hn)
            sv.append(NS(act=act[:, t], ids=ids[:, t], x=x, i=ig, f=fg, g=gg, o=og, tc=tc, cp=c, hp=h, e=e))
            h, c = np.where(a_, hn, h).astype(T), np.where(a_, cn, c).astype(T)
            sah, sac = np.where(a_, sahn, sah), np.where(a_, sacn, sac)
        blk = slice(d * Hc, (d + 1) * Hc)
        res.h[live, blk] = h[live]
        res.sa_h[:, blk] = sah
        if dout is None:
            continue
        dh = np.where(live[:, None], np.asarray(dout, dtype=T)[:, blk] * m[:, blk], 0).astype(T)
        sdh = np.abs(dh).astype(F64)
        dc, sdc = np.zeros((W, Hc), T), np.zeros((W, Hc))
        for t in range(Lmax - 1, -1, -1):
            s = sv[t]
            a_ = s.act[:, None]
            dcn = dc + dh * s.o * (1 - s.tc * s.tc)
            sdcn = sdc + sdh * s.o * (1 - s.tc * s.tc) + np.abs(dh) * (s.e.o + s.o * 2 * s.e.tc) + np.abs(dcn)
            da = np.zeros((W, 4 * Hc), T)
            sda = np.zeros((W, 4 * Hc))
            da[:, gate[0]] = dcn * s.g * s.i * (1 - s.i)
            da[:, gate[1]] = dcn * s.cp * s.f * (1 - s.f)
            da[:, gate[2]] = dcn * s.i * (1 - s.g * s.g)
            da[:, gate[3]] = dh * s.tc * s.o * (1 - s.o)
            adc, adh = np.abs(dcn), np.abs(dh)
            sda[:, gate[0]] = sdcn * np.abs(s.g) * s.i * (1 - s.i) + adc * (s.e.g * s.i * (1 - s.i) + np.abs(s.g) * s.e.i)
            sda[:, gate[1]] = sdcn * np.abs(s.cp) * s.f * (1 - s.f) + adc * (s.e.cp * s.f * (1 - s.f) + np.abs(s.cp) * s.e.f)
            sda[:, gate[2]] = sdcn * s.i * (1 - s.g * s.g) + adc * (s.e.i * (1 - s.g * s.g) + s.i * 2 * s.e.g)
            sda[:, gate[3]] = sdh * np.abs(s.tc) * s.o * (1 - s.o) + adh * (s.e.tc * s.o * (1 - s.o) + np.abs(s.tc) * s.e.o)
            sda = (sda + 4 * np.abs(da)) * a_
            da = (da * a_).astype(T)
            v = np.concatenate([s.x, s.hp], 1)
            av = np.abs(v).astype(F64)
            terms = da[:, :, None] * v[:, None, :]                                   # [W, 4Hc, E + Hc]
            dW = rowref.seq_sum32(terms, 0) if f32 else terms.sum(0)
            sW = np.einsum("wr,wk->rk", sda, av)
            res.d_wih[d] += dW[:, :E]
            res.d_whh[d] += dW[:, E:]
            res.sa_wih[d] += sW[:, :E]
            res.sa_whh[d] += sW[:, E:]
            db = rowref.seq_sum32(da, 0) if f32 else da.sum(0)
            res.d_bih[d] += db
            if defect != "no_bias_hh":
                res.d_bhh[d] += db
            res.sa_b[d] += sda.sum(0)
            dx = _dot(da, wih[d].T, f32)
            sdx = sda @ aW
            on = np.nonzero(s.act)[0]
            if defect == "emb_overwrite":
                res.d_emb[s.ids[on]] = dx[on]
            else:
                np.add.at(res.d_emb, s.ids[on], dx[on])
            np.add.at(res.sa_emb, s.ids[on], sdx[on])
            dhp = _dot(da, whh[d].T, f32)
            dh, sdh = np.where(a_, dhp, dh).astype(T), np.where(a_, sda @ aU, sdh)
            dc, sdc = np.where(a_, dcn * s.f, dc).astype(T), np.where(a_, sdcn * s.f + np.abs(dcn) * s.e.f, sdc)
    return res


GRADS = (("d_emb", "sa_emb"), ("d_wih", "sa_wih"), ("d_whh", "sa_whh"), ("d_bih", "sa_b"), ("d_bhh", "sa_b"))


def check(got, ref64, ref32, what="", stats=None):
    """got: dict name -> array for any of h (float32 values of the UNMASKED stored bf16 block) and the GRADS names, compared with the
    float64 evaluation under rowref.tolerance (h with the bf16 term).  Dropped words: h is NaN on both sides.  Raises AssertionError."""
    for name, val in got.items():
        ref = getattr(ref64, name)
        val = np.asarray(val, dtype=F64)
        assert val.shape == ref.shape, "%s %s: shape %s, expected %s" % (what, name, val.shape, ref.shape)
        if name == "h":
            nan = np.isnan(ref)
            assert (np.isnan(val) == nan).all(), "%s h: rows of dropped words must stay untouched, all others written" % what
            ok = ~nan
            tol, err32 = rowref.tolerance(ref[ok], getattr(ref32, name)[ok], ref64.sa_h[ok], bf16_out=True)
            err = np.abs(val[ok] - ref[ok])
        else:
            sa = getattr(ref64, dict(GRADS)[name])
            tol, err32 = rowref.tolerance(ref, getattr(ref32, name), sa)
            err = np.abs(val - ref)
        share = float((err / tol).max()) if err.size else 0.0
        if stats is not None:
            prev = stats.get(name, (0.0, 0.0))
            stats[name] = (max(prev[0], float(err.max()) / err32 if err32 > 0 and err.size else 0.0), max(prev[1], share))
        assert share <= 1.0, "%s %s: error %.3e is %.2f x its tolerance (float32 evaluation error %.3e)" % (what, name, err.max(), share, err32)


# ------------------------------------------------------------------ the whole step of the stacked tagger
def stack_reference64(x, char_cols, cstate, chars, lens, rows, cmask, lengths, tags, st, start, stop, weights=None):
    """float64 autograd of one step of the stacked tagger with a character embedding: lstmbwdref.head_reference64's model (torch.nn.LSTM,
    packed, bidirectional -> linear -> CRF NLL, sum_b weights[b] * nll_b) on an input whose columns [char_cols[0], char_cols[1]) are the
    character model's block -- torch.nn.Embedding -> bidirectional torch.nn.LSTM over pack_padded_sequence(enforce_sorted=False) ->
    hidden[0] -- times cmask [W, 2Hc], placed at the token-major rows `rows` (a word with rows < 0 contributes nothing).
    x [B, n, D]: the frozen features as the input GEMM sees them (masked, the character columns zero), reference column order;
    cstate: the character state dict (char_embedding.weight, char_layer.*).
    -> loss, head grads (named as head_reference64 names them), character grads (named as cstate), emissions"""
    import torch
    from oracle.train_step import crf_nll_torch
    t64 = lambda a: torch.as_tensor(np.asarray(a, F64))                         # noqa: E731
    B, n, D = x.shape
    V, E = np.asarray(cstate["char_embedding.weight"]).shape
    Hc = np.asarray(cstate["char_layer.weight_hh_l0"]).shape[1]
    emb = torch.nn.Embedding(V, E).double()
    crnn = torch.nn.LSTM(E, Hc, num_layers=1, bidirectional=True).double()
    with torch.no_grad():
        emb.weight.copy_(t64(cstate["char_embedding.weight"]))
        for k, p in crnn.named_parameters():
            p.copy_(t64(cstate["char_layer." + k]))
    rows = np.asarray(rows)
    live = np.nonzero(rows >= 0)[0]
    ce = emb(torch.from_numpy(np.asarray(chars)[live].astype(np.int64)).t())
    packed = torch.nn.utils.rnn.pack_padded_sequence(ce, torch.from_numpy(np.asarray(lens)[live].astype(np.int64)), enforce_sorted=False)
    _, (hidden, _) = crnn(packed)
    block = torch.cat([hidden[0], hidden[1]], 1) * t64(np.asarray(cmask, F64)[live])
    c0, c1 = char_cols
    assert c1 - c0 == 2 * Hc and not np.asarray(x)[:, :, c0:c1].any()
    place = torch.zeros((B * n, D), dtype=torch.float64)
    place = place.index_put((torch.from_numpy(rows[live].astype(np.int64))[:, None], torch.arange(c0, c1)[None, :]), block)
    xin = t64(x) + place.view(B, n, D)
    H = np.asarray(st["rnn"]["weight_hh_l0"]).shape[1]
    rnn = torch.nn.LSTM(D, H, 1, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for k, p in rnn.named_parameters():
            p.copy_(t64(st["rnn"][k]))
    lw, lb, tr = (t64(st[k]).clone().requires_grad_(True) for k in ("linear.weight", "linear.bias", "transitions"))
    ln = torch.as_tensor(np.asarray(lengths))
    y, _ = rnn(torch.nn.utils.rnn.pack_padded_sequence(xin, ln, batch_first=True, enforce_sorted=False))
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=n)
    em = y @ lw.t() + lb
    nll = crf_nll_torch(em, torch.as_tensor(np.asarray(tags)), ln, tr, start, stop)
    w = torch.full((B,), 1.0 / B, dtype=torch.float64) if weights is None else t64(weights)
    loss = (nll * w).sum()
    loss.backward()
    grads = {"rnn." + k: p.grad.numpy() for k, p in rnn.named_parameters()}
    grads.update({"linear.weight": lw.grad.numpy(), "linear.bias": lb.grad.numpy(), "transitions": tr.grad.numpy()})
    cgrads = {"char_embedding.weight": emb.weight.grad.numpy()}
    cgrads.update({"char_layer." + k: p.grad.numpy() for k, p in crnn.named_parameters()})
    return float(loss.detach()), grads, cgrads, em.detach().numpy()
