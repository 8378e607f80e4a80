"""TEST INFRASTRUCTURE: plain references of the stacked tagger's BiLSTM with more than one layer and a trained initial state
(kbner.stack.BiLSTMHead with rnn_layers > 1 / init_state; csrc/lstm_train.hip: kbner_lstm_seq_bwd_init), written from the formulas in
include/kbner.h (numpy only, no kernel structure).  tests/test_deepref_cpu.py proves them against float64 torch.nn.LSTM autograd and
proves that the comparisons refuse nine defective evaluations.  lstmbwdref is imported unchanged.

The reference's own forward() moves its tensors with .cuda() (flair/models/sequence_tagger_model.py:1028) and cannot run without a
GPU; its recurrence is exactly
    torch.nn.LSTM(D, H, num_layers=L, dropout=0.5 if L > 1 else 0, bidirectional=True) over pack_padded_sequence,
    started from lstm_init_h / lstm_init_c [2L, H] repeated over the batch (row 2k + d: layer k, direction d)
(:317-357, 969-994), so torch.nn.LSTM is the pin.  torch's inter-layer dropout draws its own masks; with given masks the pin is
single-layer torch.nn.LSTMs stacked by hand with the masks between them (torch_stack below), which test_deepref_cpu.py also shows
to equal the L-layer module when there is no mask.

deep_lstm       an L-layer packed BiLSTM with initial state and inter-layer masks, forward and every gradient, in float64 or -- with
                f=np.float32 -- the same formulas in plain float32; with `store` the values are rounded at the storage points of
                BiLSTMHead.loss_backward (the emulation of test_gpu_deep_stack_train.py):
                  every layer's gx = bf16(input . Wih^T + float32(bias_ih + bias_hh)) ; h_0 = bf16(lstm_init_h), c_0 float32 ;
                  h_t bf16, c_t float32, the saved gates bf16 ; the masked matrix between two layers bf16(out * multiplier) ;
                  every layer's dgx bf16, dc_carry float32 ; the gradient of a layer's input bf16(dgx . Wih), through the mask
                  bf16(. * multiplier) ; weight gradients float32
torch_stack     the float64 autograd pin
padded_weights  the device's padded operand layout of a reference-layout state (gate blocks padded to Hp; an upper layer's 2H input
                columns at [0, H) and [Hp, Hp + H)), so that deep_lstm on the padded operands proves the placement
init_case / check_init_case   the inputs of one kbner_lstm_seq_bwd_init case from a lstmbwdref case and THE comparison of its
                outputs (rowref.tolerance: float64 value, float32 restatement, sum_abs), through lstmbwdref.bwd_step on a table that
                has one virtual step in front whose saved c is c_0
"""
from types import SimpleNamespace as NS

import numpy as np

import lstmbwdref as R
import lstmref
import rowref

F64 = np.float64
NAN = float("nan")
SFX = ("", "_reverse")
DH0_GUARD = -3.5          # dh0 of a sequence that is never active: must come back bit for bit

DEFECTS = ("init_index_dL_plus_k", "c0_ignored_in_df", "dh0_without_recurrent_product", "dc0_one_direction_only", "h0_not_rounded",
           "mask_on_last_layer", "mask_not_rescaled", "upper_reads_unmasked", "upper_wih_cols_H_2H")


def _f64(a):
    return np.asarray(a, dtype=F64)


def bf(a):
    return rowref.bf16_round(_f64(a)).astype(F64)


def f32(a):
    return _f64(a).astype(np.float32).astype(F64)


STORE = NS(bf=bf, f32=f32)        # the storage types of the device path
EXACT = NS(bf=lambda a: a, f32=lambda a: a)


def layer_weights(rnn, L):
    """reference-layout state dict -> W[k][d] = (wih [4H, Din], whh [4H, H], bias_ih [4H], bias_hh [4H])"""
    return [[tuple(_f64(rnn[key % k + s]) for key in ("weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d")) for s in SFX]
            for k in range(L)]


def _sigmoid(x, f):
    one = f(1)
    return one / (one + np.exp(-x))


def _tanh(x, f):
    if f is F64:
        return np.tanh(x)
    one, two = f(1), f(2)
    with np.errstate(over="ignore"):
        return one - two / (np.exp(two * x) + one)


def deep_lstm(x, lengths, W, h0=None, c0=None, masks=None, dy=None, f=F64, store=None, defect=None):
    """x [B, n, D] ; lengths [B] ; W as layer_weights (any hidden width: the padded operands too) ; h0, c0 [2L, H] or None (zeros) ;
    masks: None or L - 1 multipliers [B, n, 2H] (0 or 1 / (1 - p)) applied to the output of every layer but the last ;
    dy [B, n, 2H]: the gradient of the last layer's output (None: forward only).
    Direction 0 reads t = 0 .. len - 1, direction 1 t = len - 1 .. 0 ; positions at or past len produce zeros and take no gradient.
    -> NS(y [B, n, 2H], ys: every layer's output, and with dy: dW[k][d] = (dwih, dwhh, dbias), dh0 / dc0 [2L, H] summed over the batch,
       dx [B, n, D], hprev0[k][d] [B, H]: the h the first step multiplied)"""
    st = EXACT if store is None else store
    L = len(W)
    H = W[0][0][1].shape[1]
    B, n, _ = np.shape(x)
    cast = lambda a: np.asarray(a, f)                                           # noqa: E731
    lengths = [int(v) for v in lengths]

    def init_row(k, d):
        return d * L + k if defect == "init_index_dL_plus_k" else 2 * k + d

    inp = cast(x)
    ys, inps, saved = [], [], []
    for k in range(L):
        inps.append(inp)
        y = np.zeros((B, n, 2 * H), f)
        sv = [[None] * B for _ in range(2)]
        for d in range(2):
            wih, whh, bih, bhh = (cast(w) for w in W[k][d])
            if store is not None:
                wih, whh = cast(st.bf(wih)), cast(st.bf(whh))
            gx = cast(st.bf(inp.reshape(B * n, -1) @ wih.T + cast(st.f32(bih + bhh)))).reshape(B, n, 4 * H)
            for b in range(B):
                h = cast(np.zeros(H) if h0 is None else h0[init_row(k, d)])
                c = cast(np.zeros(H) if c0 is None else c0[init_row(k, d)])
                if defect != "h0_not_rounded":
                    h = cast(st.bf(h))
                c = cast(st.f32(c))
                rec = NS(t=[], gates=[], c=[], hprev=[], c0=c)
                for s in range(lengths[b]):
                    t = s if d == 0 else lengths[b] - 1 - s
                    pre = (gx[b, t] + whh @ h).reshape(4, H)
                    i, fg, o = _sigmoid(pre[0], f), _sigmoid(pre[1], f), _sigmoid(pre[3], f)
                    g = _tanh(pre[2], f)
                    rec.hprev.append(h)
                    c = cast(st.f32(fg * c + i * g))
                    h = cast(st.bf(o * _tanh(c, f)))
                    rec.t.append(t)
                    rec.gates.append(cast(st.bf(np.stack([i, fg, g, o]))))
                    rec.c.append(c)
                    y[b, t, d * H:(d + 1) * H] = h
                sv[d][b] = rec
        ys.append(y)
        saved.append(sv)
        inp = y
        last = k == L - 1
        if masks is not None and (not last or (defect == "mask_on_last_layer" and L > 1)) and defect != "upper_reads_unmasked":
            m = cast(masks[min(k, L - 2)])
            if defect == "mask_not_rescaled":
                m = cast(m != 0)
            inp = cast(st.bf(y * m))
            if last:
                ys[-1] = inp
    out = NS(y=ys[-1], ys=ys)
    if dy is None:
        return out
    one = f(1)
    dyk = cast(dy)
    if masks is not None and defect == "mask_on_last_layer" and L > 1:
        dyk = dyk * cast(masks[L - 2])
    out.dW = [[None, None] for _ in range(L)]
    out.dh0, out.dc0 = np.zeros((2 * L, H), f), np.zeros((2 * L, H), f)
    out.hprev0 = [[None, None] for _ in range(L)]
    for k in range(L - 1, -1, -1):
        Din = inps[k].shape[2]
        dinp = np.zeros((B, n, Din), f)
        for d in range(2):
            wih, whh, _, _ = (cast(w) for w in W[k][d])
            if store is not None:
                wih, whh = cast(st.bf(wih)), cast(st.bf(whh))
            dgx = np.zeros((B, n, 4 * H), f)
            hprev = np.zeros((B, n, H), f)
            out.hprev0[k][d] = np.stack([saved[k][d][b].hprev[0] if lengths[b] else np.zeros(H, f) for b in range(B)])
            for b in range(B):
                rec = saved[k][d][b]
                carry, back = np.zeros(H, f), np.zeros(H, f)
                for s in range(lengths[b] - 1, -1, -1):
                    t = rec.t[s]
                    dh = dyk[b, t, d * H:(d + 1) * H] + back
                    i, fg, g, o = rec.gates[s]
                    c = rec.c[s]
                    cp = rec.c[s - 1] if s > 0 else (np.zeros(H, f) if defect == "c0_ignored_in_df" else rec.c0)
                    tc = _tanh(c, f)
                    dc = carry + dh * o * (one - tc * tc)
                    row = cast(st.bf(np.concatenate([dc * g * i * (one - i), dc * cp * fg * (one - fg), dc * i * (one - g * g),
                                                     dh * tc * o * (one - o)])))
                    carry = cast(st.f32(dc * fg))
                    dgx[b, t] = row
                    hprev[b, t] = rec.hprev[s]
                    back = row @ whh                                                  # the recurrent product: [4H] . [4H, H]
                if lengths[b]:
                    if defect != "dh0_without_recurrent_product":
                        out.dh0[init_row(k, d)] += cast(st.f32(back))
                    if not (defect == "dc0_one_direction_only" and d == 1):
                        out.dc0[init_row(k, d)] += carry
            flat = dgx.reshape(B * n, 4 * H)
            out.dW[k][d] = (cast(st.f32(flat.T @ inps[k].reshape(B * n, Din))), cast(st.f32(flat.T @ hprev.reshape(B * n, H))),
                            cast(st.f32(flat.sum(0))))
            dinp += (flat @ wih).reshape(B, n, Din)
        dinp = cast(st.bf(dinp))                          # (one product over both directions' gate columns, rounded once)
        if k > 0 and masks is not None and defect != "upper_reads_unmasked":
            m = cast(masks[k - 1])
            if defect == "mask_not_rescaled":
                m = cast(m != 0)
            dinp = cast(st.bf(dinp * m))
        dyk = dinp
    out.dx = dyk
    return out


def rnn_grads(res, L):
    """deep_lstm's weight gradients under torch.nn.LSTM's names (bias_ih and bias_hh receive one gradient)"""
    g = {}
    for k in range(L):
        for d, s in enumerate(SFX):
            dwih, dwhh, db = res.dW[k][d]
            g["weight_ih_l%d%s" % (k, s)], g["weight_hh_l%d%s" % (k, s)] = dwih, dwhh
            g["bias_ih_l%d%s" % (k, s)] = g["bias_hh_l%d%s" % (k, s)] = db
    return g


# ------------------------------------------------------------------ the float64 autograd pin
def torch_stack(x, lengths, rnn, L, h0=None, c0=None, masks=None, module=False):
    """x [B, n, D]: an array, or a float64 torch tensor.  float64 torch: L single-layer bidirectional torch.nn.LSTMs over pack_padded_sequence(enforce_sorted=False) stacked by hand,
    layer k started from rows 2k, 2k + 1 of h0 / c0 repeated over the batch, masks[k] multiplying the output of layer k < L - 1 --
    or, with module=True (no masks), ONE torch.nn.LSTM(num_layers=L, dropout=0): the reference's call.
    -> y (requires grad through everything), params {name: tensor}, h0, c0, x as leaf tensors"""
    import torch
    if not isinstance(x, torch.Tensor):      # (a tensor: part of a larger graph, e.g. behind a character model -- used as it is)
        x = torch.tensor(_f64(x), requires_grad=True)
    B, n, D = x.shape
    H = np.shape(rnn["weight_hh_l0"])[1]
    lens = torch.as_tensor(np.asarray(lengths))
    th0 = None if h0 is None else torch.tensor(_f64(h0), requires_grad=True)
    tc0 = None if c0 is None else torch.tensor(_f64(c0), requires_grad=True)
    rep = lambda t: t.unsqueeze(1).repeat(1, B, 1)                              # noqa: E731

    def run(mod, inp, hx):
        packed = torch.nn.utils.rnn.pack_padded_sequence(inp, lens, batch_first=True, enforce_sorted=False)
        y, _ = mod(packed) if hx is None else mod(packed, hx)
        return torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=n)[0]

    params = {}
    if module:
        assert masks is None
        mod = torch.nn.LSTM(D, H, L, bidirectional=True, batch_first=True, dropout=0.0).double()
        with torch.no_grad():
            for k_, p in mod.named_parameters():
                p.copy_(torch.as_tensor(_f64(rnn[k_])))
        params = dict(mod.named_parameters())
        y = run(mod, x, None if th0 is None else (rep(th0), rep(tc0)))
        return y, params, th0, tc0, x
    inp = x
    for k in range(L):
        mod = torch.nn.LSTM(inp.shape[2], H, 1, bidirectional=True, batch_first=True).double()
        with torch.no_grad():
            for k_, p in mod.named_parameters():
                p.copy_(torch.as_tensor(_f64(rnn[k_.replace("_l0", "_l%d" % k)])))
        params.update({k_.replace("_l0", "_l%d" % k): p for k_, p in mod.named_parameters()})
        hx = None if th0 is None else (rep(th0[2 * k:2 * k + 2]), rep(tc0[2 * k:2 * k + 2]))
        y = run(mod, inp, hx)
        inp = y if (masks is None or k == L - 1) else y * torch.as_tensor(_f64(masks[k]))
    return y, params, th0, tc0, x


# ------------------------------------------------------------------ the device's padded operands
def padded_weights(rnn, L, H, Hp, defect=None):
    """reference layout -> W as layer_weights for hidden width Hp: every gate block zero-padded to Hp rows, Whh's H input columns at
    [0, H), an upper layer's 2H input columns at [0, H) and [Hp, Hp + H) (where the recurrence writes the two directions)"""
    def gates(w):
        w = _f64(w)
        out = np.zeros((4 * Hp,) + w.shape[1:])
        for q in range(4):
            out[q * Hp:q * Hp + H] = w[q * H:(q + 1) * H]
        return out

    W = []
    for k in range(L):
        row = []
        for s in SFX:
            wih = gates(rnn["weight_ih_l%d%s" % (k, s)])
            if k > 0:
                wide = np.zeros((4 * Hp, 2 * Hp))
                second = H if defect == "upper_wih_cols_H_2H" else Hp
                wide[:, :H], wide[:, second:second + H] = wih[:, :H], wih[:, H:]
                wih = wide
            whh = np.zeros((4 * Hp, Hp))
            whh[:, :H] = gates(rnn["weight_hh_l%d%s" % (k, s)])
            row.append((wih, whh, gates(rnn["bias_ih_l%d%s" % (k, s)]), gates(rnn["bias_hh_l%d%s" % (k, s)])))
        W.append(row)
    return W


def pad_cols(a, H, Hp):
    """[..., 2H] -> [..., 2Hp]: the two directions at [0, H) and [Hp, Hp + H)"""
    a = _f64(a)
    out = np.zeros(a.shape[:-1] + (2 * Hp,))
    out[..., :H], out[..., Hp:Hp + H] = a[..., :H], a[..., H:]
    return out


def unpad_cols(a, H, Hp):
    return np.concatenate([a[..., :H], a[..., Hp:Hp + H]], -1)


def unpad_gates(w, H, Hp):
    return np.concatenate([w[q * Hp:q * Hp + H] for q in range(4)], 0)


def pad_init(a, H, Hp):
    a = _f64(a)
    out = np.zeros((a.shape[0], Hp))
    out[:, :H] = a
    return out


# ------------------------------------------------------------------ the whole head
def head(x, lengths, tags, st, L, start, stop, masks=None, weights=None, store=None, defect=None):
    """BiLSTM (deep_lstm) -> linear -> CRF NLL (oracle.train_step.crf_nll_torch, float64), sum_b weights[b] nll_b (default 1 / B),
    and every gradient.  st: the reference-layout state BiLSTMHead.state() gives (lstm_init_h / lstm_init_c optional).
    store=STORE: the emulation of the device path (emissions, d emissions float32; d out = bf16(d emissions . linear.weight);
    linear.* and transitions float32; the rest as deep_lstm lists).  -> loss, grads {name: float64}, emissions [B, n, T]"""
    import torch
    from oracle.train_step import crf_nll_torch
    s_ = EXACT if store is None else store
    x = _f64(x)
    B, n, _ = x.shape
    W = layer_weights(st["rnn"], L)
    h0, c0 = st.get("lstm_init_h"), st.get("lstm_init_c")
    fw = deep_lstm(x, lengths, W, h0, c0, masks, store=store, defect=defect)
    lw, lb = _f64(st["linear.weight"]), _f64(st["linear.bias"])
    em = torch.tensor(s_.f32(fw.y.reshape(B * n, -1) @ lw.T + lb).reshape(B, n, -1), requires_grad=True)
    tr = torch.tensor(_f64(st["transitions"]), requires_grad=True)
    nll = crf_nll_torch(em, torch.as_tensor(np.asarray(tags)), torch.as_tensor(np.asarray(lengths)), tr, start, stop)
    w = torch.full((B,), 1.0 / B, dtype=torch.float64) if weights is None else torch.as_tensor(_f64(weights))
    loss = (nll * w).sum()
    loss.backward()
    dem = s_.f32(em.grad.numpy().reshape(B * n, -1))
    res = deep_lstm(x, lengths, W, h0, c0, masks, dy=s_.bf(dem @ lw).reshape(B, n, -1), store=store, defect=defect)
    grads = {"rnn." + k: v for k, v in rnn_grads(res, L).items()}
    grads.update({"linear.weight": s_.f32(dem.T @ fw.y.reshape(B * n, -1)), "linear.bias": s_.f32(dem.sum(0)),
                  "transitions": s_.f32(tr.grad.numpy())})
    if h0 is not None:
        grads["lstm_init_h"], grads["lstm_init_c"] = s_.f32(res.dh0), s_.f32(res.dc0)
    return float(loss.detach()), grads, em.detach().numpy()


def head_torch(x, lengths, tags, st, L, start, stop, masks=None, weights=None):
    """the same loss and gradients by float64 torch autograd through torch_stack: what the device path is compared with"""
    import torch
    from oracle.train_step import crf_nll_torch
    B, n = int(x.shape[0]), int(x.shape[1])
    y, params, h0, c0, _ = torch_stack(x, lengths, st["rnn"], L, st.get("lstm_init_h"), st.get("lstm_init_c"), masks)
    lw = torch.tensor(_f64(st["linear.weight"]), requires_grad=True)
    lb = torch.tensor(_f64(st["linear.bias"]), requires_grad=True)
    tr = torch.tensor(_f64(st["transitions"]), requires_grad=True)
    em = y @ lw.t() + lb
    nll = crf_nll_torch(em, torch.as_tensor(np.asarray(tags)), torch.as_tensor(np.asarray(lengths)), tr, start, stop)
    w = torch.full((B,), 1.0 / B, dtype=torch.float64) if weights is None else torch.as_tensor(_f64(weights))
    loss = (nll * w).sum()
    loss.backward()
    grads = {"rnn." + k: p.grad.numpy() for k, p in params.items()}
    grads.update({"linear.weight": lw.grad.numpy(), "linear.bias": lb.grad.numpy(), "transitions": tr.grad.numpy()})
    if h0 is not None:
        grads["lstm_init_h"], grads["lstm_init_c"] = h0.grad.numpy(), c0.grad.numpy()
    return float(loss.detach()), grads, em.detach().numpy()


# ------------------------------------------------------------------ kbner_lstm_seq_bwd_init: cases and THE comparison
# (kind, Hp, B, ndir, steps) as lstmbwdref's.  Hp 64 / 128 / 320 ; B 1 / 17 / 48 / 65: NT = 1, 2, 3, 4 and a second batch chunk ;
# 1 and 2 directions ; 1, 2 and 5 steps.  lstmbwdref.tables gives every case with steps >= 2 sequences of length 1 (step 0 is also
# their last), and from B = 3 on one sequence that is never active and one that never stores.
REAL_CASES = [("real", 64, 1, 2, 5), ("real", 64, 17, 1, 2), ("real", 64, 48, 2, 1), ("real", 64, 65, 2, 5), ("real", 128, 17, 2, 5),
              ("real", 128, 48, 1, 5), ("real", 128, 65, 2, 2), ("real", 320, 1, 1, 1), ("real", 320, 17, 2, 2), ("real", 320, 48, 2, 5),
              ("real", 320, 65, 1, 5)]
EXACT_CASES = [("exact", 64, 17, 2, 2), ("exact", 128, 65, 1, 1), ("exact", 320, 48, 2, 2)]
ZERO_STEP_CASES = [("exact", 64, 17, 2, 0)]


def init_case(case):
    """-> NS(d: the lstmbwdref case, c0 [ndir, B, Hp] float32 values, dh0_0: what dh0 holds on entry, aug: the case with one virtual
    step in front).  REAL: c0 Gaussian.  EXACT: c0 in {0, +-4}, so that df = dc c0 / 4 = +-dc or 0 stays a bf16 value (lstmbwdref's
    EXACT conditions bound dc by 8 significant bits) -- and then only df of step 0 changes: the walk's other values are
    lstmbwdref's."""
    d = R.build_case(case)
    rng = np.random.default_rng([7, d.Hp, d.B, d.ndir, d.steps])
    shape = (d.ndir, d.B, d.Hp)
    c0 = 4.0 * rng.integers(-1, 2, size=shape) if d.kind == "exact" else rng.standard_normal(shape).astype(np.float32).astype(F64)
    return NS(d=d, c0=c0, dh0_0=np.full(shape, DH0_GUARD), aug=_augment(d, c0), case=case)


def _augment(d, c0):
    """case d with a virtual step in front of step 0: the virtual step of (direction dd, sequence b) consumed row rows_gx + dd * B + b,
    whose saved c is c0[dd, b] (its gates are never read: lstmbwdref.bwd_step is only asked for steps >= 1 of this table, where
    gxi[s - 1] then names c_0 for the first real step)"""
    extra = d.ndir * d.B
    virt = (d.rows_gx + np.arange(extra)).reshape(1, d.ndir, d.B).astype(np.int32)
    ever = (d.gxi[:1] >= 0) if d.steps else np.zeros((1, d.ndir, d.B), bool)
    gxi = np.concatenate([np.where(ever, virt, -1).astype(np.int32), d.gxi], 0)
    outi = np.concatenate([np.full((1, d.ndir, d.B), -1, np.int32), d.outi], 0)
    cs = np.concatenate([d.cs, np.full((extra, d.ndir * d.Hp), NAN)], 0)
    for dd in range(d.ndir):
        cs[d.rows_gx + dd * d.B:d.rows_gx + (dd + 1) * d.B, dd * d.Hp:(dd + 1) * d.Hp] = c0[dd]
    gates = np.concatenate([d.gates, np.full((extra, d.gates.shape[1]), NAN)], 0)
    a = NS(**vars(d))
    a.gxi, a.outi, a.cs, a.gates, a.rows_gx, a.steps = gxi, outi, cs, gates, d.rows_gx + extra, d.steps + 1
    return a


def _grow(dgx, extra):
    return np.concatenate([_f64(dgx), np.full((extra, np.shape(dgx)[1]), NAN)], 0)


def dh0_reference(d, dgx, f32_eval=False):
    """dh0[dd, b] = dgx[gxi[0, dd, b], dd-block] . Whh_dd for the active (dd, b) -> value [ndir, B, Hp] (NaN elsewhere), sum_abs"""
    K = 4 * d.Hp
    val, sa = np.full((d.ndir, d.B, d.Hp), NAN), np.zeros((d.ndir, d.B, d.Hp))
    for dd in range(d.ndir):
        a = np.nonzero(d.gxi[0, dd] >= 0)[0]
        rows = _f64(dgx)[d.gxi[0, dd, a], dd * K:(dd + 1) * K]
        w = _f64(d.whh[dd])
        val[dd, a] = rowref.seq_dot32(rows, w.T).astype(F64) if f32_eval else rows @ w
        sa[dd, a] = np.abs(rows) @ np.abs(w)
    return val, sa


def evaluate_init(ic, defect=None):
    """the walk of an init case as a correct kernel leaves it in memory (dgx bf16, carries float32, dh0 float32) -- or with one defect:
    "c0_ignored_in_df", "dh0_without_recurrent_product", "dh0_at_finished" (written where gxi[0] < 0)"""
    d, a = ic.d, ic.aug
    extra = d.ndir * d.B
    if d.steps == 0:
        return NS(dgx=np.full((d.rows_gx, d.ndir * 4 * d.Hp), np.float32(NAN)), carry_after=[d.carry0.astype(np.float32)],
                  dh0=ic.dh0_0.astype(np.float32))
    src = a
    if defect == "c0_ignored_in_df":
        src = NS(**vars(a))
        src.cs = np.where(np.arange(a.rows_gx)[:, None] >= d.rows_gx, 0.0 * a.cs, a.cs)
    dgx = np.full((a.rows_gx, d.ndir * 4 * d.Hp), NAN)
    carry = _f64(d.carry0).copy()
    after = [None] * d.steps + [carry]
    for s in range(d.steps - 1, -1, -1):
        stp = R.bwd_step(src, s + 1, dgx, carry)
        R._put(dgx, d.Hp, stp, True)
        carry = stp.carry.astype(np.float32).astype(F64)
        after[s] = carry
    val, _ = dh0_reference(d, np.nan_to_num(dgx[:d.rows_gx]))
    dh0 = np.where(np.isnan(val), ic.dh0_0, val)
    if defect == "dh0_without_recurrent_product":
        dh0 = np.where(np.isnan(val), ic.dh0_0, 0.0)
    if defect == "dh0_at_finished":
        dh0 = np.where(np.isnan(val), 0.0, val)
    stored = R.as_stored(NS(dgx=dgx[:d.rows_gx], carry_after=after))
    stored.dh0 = dh0.astype(np.float32)
    return stored


def check_init_case(ic, got, what="", stats=None, log=None):
    """THE comparison of a kbner_lstm_seq_bwd_init run.  got.dgx [rows_gx, ndir*4Hp] (float32 values of the stored bf16; NaN where the
    call wrote nothing), got.carry_after: steps + 1 float32 arrays as lstmbwdref.check_bwd_case takes them, got.dh0 [ndir, B, Hp]
    float32.  Structure bit for bit (rows no step consumes, the carry and dh0 of finished / never-active sequences); EXACT cases
    equal the reference walk; REAL cases under rowref.tolerance, every step forced on the kernel's own dgx and carry."""
    d, a = ic.d, ic.aug
    steps, Hp, K, extra = d.steps, d.Hp, 4 * d.Hp, d.ndir * d.B
    used4 = np.repeat(R._consumed(d.gxi, d.rows_gx, d.ndir), K, axis=1)
    assert np.isnan(got.dgx[~used4]).all(), "%s: a dgx row that no step consumes was written" % what
    assert np.isfinite(got.dgx[used4]).all(), "%s: a consumed dgx row was not written (or is not finite)" % what
    assert R._bits_equal(got.carry_after[steps], d.carry0), "%s: the initial carry is not the case's" % what
    for s in range(steps - 1, -1, -1):
        fin = d.gxi[s] < 0
        assert R._bits_equal(got.carry_after[s][fin], got.carry_after[s + 1][fin]), "%s step %d: the carry of a finished sequence changed" % (what, s)
    first = (d.gxi[0] >= 0) if steps else np.zeros((d.ndir, d.B), bool)
    assert R._bits_equal(got.dh0[~first], ic.dh0_0[~first]), "%s: dh0 written where gxi[0] < 0" % what
    if not steps:
        return
    assert np.isfinite(got.dh0[first]).all(), "%s: dh0 of an active sequence was not written" % what
    if d.kind == "exact":
        ref = evaluate_init(ic)
        bad = np.argwhere((got.dgx != ref.dgx) & used4)
        assert bad.shape[0] == 0, "%s: %d dgx elements differ, first at %s: got %r expected %r" % (
            what, bad.shape[0], tuple(bad[0]), got.dgx[tuple(bad[0])], ref.dgx[tuple(bad[0])])
        for s in range(steps):
            lstmref.check_exact(got.carry_after[s], _f64(ref.carry_after[s]), "%s carry after step %d" % (what, s))
        lstmref.check_exact(got.dh0[first], _f64(ref.dh0)[first], "%s dh0" % what)
        return
    grown = _grow(got.dgx, extra)
    for s in range(steps - 1, -1, -1):
        ref = R.bwd_step(a, s + 1, grown, _f64(got.carry_after[s + 1]))
        e32 = R.bwd_step(a, s + 1, grown, _f64(got.carry_after[s + 1]), f32=True)
        for dd in range(d.ndir):
            r = ref.rows[dd]
            if not len(r):
                continue
            tol, err32 = rowref.tolerance(ref.val[dd], e32.val[dd], ref.sa_dgx[dd], bf16_out=True)
            lstmref._share("lstm_seq_bwd_init (dgx, bf16)", "%s step %d dir %d" % (what, s, dd),
                           np.abs(_f64(got.dgx[r, dd * K:(dd + 1) * K]) - ref.val[dd]), tol, err32, True, stats, log)
        act = d.gxi[s] >= 0
        if act.any():
            tol, err32 = rowref.tolerance(ref.carry[act], e32.carry[act], ref.sa_carry[act])
            lstmref._share("lstm_seq_bwd_init (dc_carry)", "%s step %d" % (what, s), np.abs(_f64(got.carry_after[s]) - ref.carry)[act],
                           tol, err32, False, stats, log)
    val, sa = dh0_reference(d, got.dgx)
    e32, _ = dh0_reference(d, got.dgx, f32_eval=True)
    tol, err32 = rowref.tolerance(val[first], e32[first], sa[first])
    lstmref._share("lstm_seq_bwd_init (dh0)", what, np.abs(_f64(got.dh0) - val)[first], tol, err32, False, stats, log)


def check_h0_saved(hprev_step0, h0, what=""):
    """the forward's hprev rows of step 0 [*, Hp] (float32 values of the stored bf16) against h_0 [*, Hp]: the state the recurrence
    starts from is bf16(h_0), bit for bit"""
    assert R._bits_equal(hprev_step0, rowref.bf16_round(_f64(h0))), "%s: hprev of step 0 is not bf16(h_0)" % what
