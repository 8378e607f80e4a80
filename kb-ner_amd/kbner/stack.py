"""Engine of BASELINE config 5 (ACE-style stacked embeddings -> BiLSTM -> linear -> CRF): inference, and training of the BiLSTM
-> linear -> CRF head on frozen features (BiLSTMHead.enable_training / loss_backward, StackOptimizer), all arithmetic in
libkbner_hip.so.

Reference path (restated): FastSequenceTagger.forward with `use_rnn` (flair/models/sequence_tagger_model.py:844-1052):
    sentence_tensor = cat([features[name] * selection[idx] for idx, name in enumerate(sorted(features))], -1)   (:879-891)
    packed BiLSTM (torch.nn.LSTM(D, hidden, rnn_layers, bidirectional, dropout 0.5 between layers), optionally started from the trained
    lstm_init_h / lstm_init_c, :317-357, :969-994) -> linear(2 * hidden -> T) (:1027)
and the feature producers: TransformerWordEmbeddings (frozen, first-sub-token pooling, optionally `use_internal_doc`:
embeddings.py:3116-3117,3283-3284) and FlairEmbeddings (character LM hidden state at each token's end,
embeddings.py:2469-2543, flair/models/language_model.py:71-138).

Layout: ONE bf16 matrix X [rows = B * n padded to 128, D_total padded to 64] is the concatenation; every producer writes its own
column block in place (transformers: kbner_gather_rows_ld from the encoder's hidden states; character LMs: the LSTM step
kernel stores h_t at the token-end steps straight into X), so torch.cat never happens.  The BiLSTM's input half is one MFMA
GEMM over all time steps, its recurrent half one launch per time step for both directions (csrc/lstm.hip).  While the head trains, the
features are constants: FeatureStore keeps each sentence's rows of X after their first computation (embeddings_storage_mode)."""
import numpy as np
import torch

from . import lib as L_
from . import ops
from .lib import EPI_ATOMIC32, EPI_BIAS, GEMM_NN, GEMM_NT, GEMM_TN

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _round_up(x, m):
    return (x + m - 1) // m * m


class LSTMGroup:
    """`ndir` single-layer LSTMs of one hidden width run in lockstep (the two directions of the tagger's BiLSTM; one character
    LM).  Holds Whh as bf16 [ndir, 4Hp, Hp] (hidden zero-padded to a multiple of 64: a padded unit has zero weights, so its c
    and h stay exactly 0) and runs the recurrence given pre-activations and per-step row tables."""

    def __init__(self, w_hh_list, hidden, device):
        self.H = int(hidden)
        self.Hp = _round_up(self.H, 64)   # kbner_lstm_seq: a wave's k slice is 64 wide (whole 128-byte lines of Whh)
        self.ndir = len(w_hh_list)
        self.device = torch.device(device)
        whh = torch.zeros((self.ndir, 4 * self.Hp, self.Hp), dtype=F32)
        for d, w in enumerate(w_hh_list):
            w = torch.as_tensor(w, dtype=F32)
            assert tuple(w.shape) == (4 * self.H, self.H)
            for q in range(4):
                whh[d, q * self.Hp:q * self.Hp + self.H, :self.H] = w[q * self.H:(q + 1) * self.H]
        self.whh = whh.to(BF16).to(self.device).contiguous()

    def pad_gates(self, t, axis=0):
        """[4H, ...] gate-major (i|f|g|o) tensor -> [4Hp, ...] with every gate block zero-padded"""
        t = torch.as_tensor(t, dtype=F32)
        out = torch.zeros((4 * self.Hp,) + tuple(t.shape[1:]), dtype=F32)
        for q in range(4):
            out[q * self.Hp:q * self.Hp + self.H] = t[q * self.H:(q + 1) * self.H]
        return out

    def _state0(self, B, h0, c0):
        """the state a recurrence starts from: zeros, or h0 bf16 / c0 f32 [ndir, Hp] broadcast over the batch
        -> h bf16 [2, ndir, B, Hp] (h[0] = h_0), c f32 [ndir, B, Hp]"""
        h = torch.zeros((2, self.ndir, B, self.Hp), dtype=BF16, device=self.device)
        c = torch.zeros((self.ndir, B, self.Hp), dtype=F32, device=self.device)
        if h0 is not None:
            h[0] = h0.view(self.ndir, 1, self.Hp)
        if c0 is not None:
            c += c0.view(self.ndir, 1, self.Hp)
        return h, c

    def run(self, gx, gxi, outi, out, out_dir_stride, B, col=0, out_cols=None, h0=None, c0=None):
        """gx bf16 [rows, ndir*4Hp]; gxi / outi int32 [steps, ndir, B] (device); out bf16 [rows_out, ld]; col: first column of
        direction 0's h inside `out`, direction d at col + d * out_dir_stride -- or out_cols: one first column per direction.
        h0 bf16 / c0 f32 [ndir, Hp]: the initial state of every sequence (default zeros).
        The whole recurrence is ONE call into the library (kbner_lstm_seq: one launch per time step, enqueued back to back)."""
        steps = gxi.shape[0]
        if out_cols is None:
            out_cols = [col + d * out_dir_stride for d in range(self.ndir)]
        if len(out_cols) != self.ndir or any(int(x) % 4 for x in out_cols):
            raise L_.KbnerError("LSTM output column offsets: one per direction, each a multiple of 4")
        h, c = self._state0(B, h0, c0)
        oc = torch.tensor([int(x) for x in out_cols], dtype=I32, device=self.device)
        gxi, outi = gxi.contiguous(), outi.contiguous()
        L_.call("kbner_lstm_seq", L_.ptr(gx), gx.shape[-1], L_.ptr(gxi), L_.ptr(self.whh), L_.ptr(h), L_.ptr(c), L_.ptr(out),
                out.shape[-1], L_.ptr(oc), L_.ptr(outi), steps, B, self.Hp, self.ndir, L_.stream_ptr())
        return h[steps & 1]

    def whh_t(self):
        """Whh of every direction transposed, bf16 [ndir, Hp, 4Hp]: what kbner_lstm_seq_bwd reads (made once per optimizer step)"""
        return self.whh.transpose(1, 2).contiguous()

    def run_train(self, gx, gxi_host, out, B, out_cols, h0=None, c0=None):
        """The recurrence from h_0 = c_0 = 0 (or h0 bf16 / c0 f32 [ndir, Hp], broadcast over the batch) through
        kbner_lstm_seq_train.  gxi_host int32 [steps, ndir, B] (numpy; used as outi too), checked against the training contract
        before upload.  -> the saved state for run_bwd."""
        gxi_host = check_prefix_active(gxi_host, gx.shape[0], self.ndir, B)
        if len(out_cols) != self.ndir or any(int(x) % 4 for x in out_cols):
            raise L_.KbnerError("LSTM output column offsets: one per direction, each a multiple of 4")
        steps, rows, Hp, nd = gxi_host.shape[0], gx.shape[0], self.Hp, self.ndir
        tab = torch.from_numpy(gxi_host).to(self.device)
        h, c = self._state0(B, h0, c0)
        oc = torch.tensor([int(x) for x in out_cols], dtype=I32, device=self.device)
        # zero-filled: the weight-gradient GEMMs read every row, consumed or not
        saved = dict(c0=None if c0 is None else c.clone(),      # (the kernel advances c in place)
                     gates=torch.zeros((rows, nd * 4 * Hp), dtype=BF16, device=self.device),
                     cs=torch.zeros((rows, nd * Hp), dtype=F32, device=self.device),
                     hprev=torch.zeros((rows, nd * Hp), dtype=BF16, device=self.device), tab=tab, oc=oc, steps=steps, B=B)
        L_.call("kbner_lstm_seq_train", L_.ptr(gx), gx.shape[-1], L_.ptr(tab), L_.ptr(self.whh), L_.ptr(h), L_.ptr(c), L_.ptr(out),
                out.shape[-1], L_.ptr(oc), L_.ptr(tab), steps, B, Hp, nd, L_.ptr(saved["gates"]), L_.ptr(saved["cs"]),
                L_.ptr(saved["hprev"]), L_.stream_ptr())
        return saved

    def run_bwd(self, dout, saved, whh_t, state_grads=False):
        """dout bf16 [rows_out, ld]: the gradient of run_train's `out` -> dgx bf16 [rows, ndir*4Hp] (zero where nothing was consumed).
        state_grads: through kbner_lstm_seq_bwd_init, which reads the c_0 run_train started from
        -> (dgx, d c_0 f32 [ndir, B, Hp], d h_0 f32 [ndir, B, Hp])"""
        rows, Hp, nd, B = saved["gates"].shape[0], self.Hp, self.ndir, saved["B"]
        dgx = torch.zeros((rows, nd * 4 * Hp), dtype=BF16, device=self.device)
        carry = torch.zeros((nd, B, Hp), dtype=F32, device=self.device)
        if state_grads:
            dh0 = torch.zeros((nd, B, Hp), dtype=F32, device=self.device)
            L_.call("kbner_lstm_seq_bwd_init", L_.ptr(dout), dout.shape[-1], L_.ptr(saved["oc"]), L_.ptr(saved["tab"]),
                    L_.ptr(saved["tab"]), L_.ptr(whh_t), L_.ptr(saved["gates"]), L_.ptr(saved["cs"]), L_.ptr(saved["c0"]), L_.ptr(carry),
                    L_.ptr(dgx), dgx.shape[-1], L_.ptr(dh0), saved["steps"], B, Hp, nd, L_.stream_ptr())
            return dgx, carry, dh0
        L_.call("kbner_lstm_seq_bwd", L_.ptr(dout), dout.shape[-1], L_.ptr(saved["oc"]), L_.ptr(saved["tab"]), L_.ptr(saved["tab"]),
                L_.ptr(whh_t), L_.ptr(saved["gates"]), L_.ptr(saved["cs"]), L_.ptr(carry), L_.ptr(dgx), dgx.shape[-1], saved["steps"], B,
                Hp, nd, L_.stream_ptr())
        return dgx

    def run_stepwise(self, gx, gxi, outi, out, out_dir_stride, B, col=0):
        """the same recurrence through the one-wave-per-tile step kernel, one library call per time step (kept as the A/B and
        cross-check of kbner_lstm_seq)"""
        steps = gxi.shape[0]
        h = [torch.zeros((self.ndir, B, self.Hp), dtype=BF16, device=self.device) for _ in range(2)]
        c = torch.zeros((self.ndir, B, self.Hp), dtype=F32, device=self.device)
        if col % 4:
            raise L_.KbnerError("LSTM output column offset must be a multiple of 4")
        for s in range(steps):
            self._step(gx, gxi[s], h[s & 1], h[(s + 1) & 1], c, out, col, outi[s], out_dir_stride)
        return h[steps & 1]

    def _step(self, gx, gxi, h_in, h_out, c, out, col, outi, out_dir_stride):
        ndir, B, Hp = h_in.shape
        L_.call("kbner_lstm_step", L_.ptr(gx), gx.shape[-1], L_.ptr(gxi), L_.ptr(self.whh), L_.ptr(h_in), L_.ptr(h_out), L_.ptr(c),
                L_.c_void_p(out.data_ptr() + 2 * col), out.shape[-1], out_dir_stride, L_.ptr(outi), B, Hp, ndir, L_.stream_ptr())


def step_tables(lengths, n, bidirectional=True):
    """row tables of a packed (variable-length) pass over token-major rows b*n + t: forward direction consumes t = s, the
    backward direction t = len_b - 1 - s; finished sequences get -1 (torch pack_padded_sequence / pad_packed_sequence: state
    frozen, padded outputs stay zero).  -> int32 [steps, ndir, B]"""
    lengths = np.asarray(lengths, np.int64)
    B = len(lengths)
    steps = int(lengths.max()) if B else 0
    s = np.arange(steps)[:, None]
    base = (np.arange(B) * n)[None, :]
    live = s < lengths[None, :]
    fwd = np.where(live, base + s, -1)
    if not bidirectional:
        return fwd[:, None, :].astype(np.int32)
    bwd = np.where(live, base + (lengths[None, :] - 1 - s), -1)
    return np.stack([fwd, bwd], 1).astype(np.int32)


def check_prefix_active(gxi, rows, ndir, B):
    """The training contract of kbner_lstm_seq_train / kbner_lstm_seq_bwd, which the library cannot check (the tables live in
    device memory): int [steps, ndir, B], entries -1 or a row of [0, rows), every (direction, sequence) active for steps
    0 .. len - 1 and finished after, no (direction, row) consumed twice.  -> the table as contiguous int32."""
    t = np.asarray(gxi)
    if t.ndim != 3 or t.shape[1] != ndir or t.shape[2] != B or not np.issubdtype(t.dtype, np.integer):
        raise L_.KbnerError("LSTM training row table: int [steps, %d, %d]" % (ndir, B))
    if t.size and (t.min() < -1 or t.max() >= rows):
        raise L_.KbnerError("LSTM training row table: entries are -1 or a row below %d" % rows)
    act = t >= 0
    if (act[1:] & ~act[:-1]).any():
        raise L_.KbnerError("LSTM training row table: a sequence is active after it finished (the table must be prefix-active)")
    for d in range(ndir):
        r = t[:, d][act[:, d]]
        if len(np.unique(r)) != len(r):
            raise L_.KbnerError("LSTM training row table: a row is consumed twice by one direction")
    return np.ascontiguousarray(t, np.int32)


class _Block:
    """A parameter block beside the head's one-layer arena: a flat fp32 arena of `_FIELDS` (each padded to 4 floats), a gradient
    buffer once training is enabled, and a bf16 shadow of the first `n_shadow` floats (the GEMM / recurrence operands)."""
    _FIELDS = ()

    def _alloc(self, shapes, n_shadow_before, device):
        self.device = torch.device(device)
        self.shapes, self.offsets, off = shapes, {}, 0
        for k in self._FIELDS:
            self.offsets[k] = off
            off += _round_up(int(np.prod(shapes[k])), 4)
        self.n = off
        self.n_shadow = self.offsets[n_shadow_before] if n_shadow_before else 0
        self.arena = torch.zeros(self.n, dtype=F32, device=self.device)
        self.shadow = torch.zeros(self.n_shadow, dtype=BF16, device=self.device) if self.n_shadow else None
        self.g = None

    def enable_training(self):
        if self.g is None:
            self.g = torch.zeros(self.n, dtype=F32, device=self.device)

    def param(self, name, buf=None):
        buf = self.arena if buf is None else buf
        o, shp = self.offsets[name], self.shapes[name]
        return buf[o:o + int(np.prod(shp))].view(shp)

    def grad(self, name):
        return self.param(name, self.g)


class UpperLayer(_Block):
    """Layer k >= 1 of the head's BiLSTM (torch.nn.LSTM(num_layers > 1): it reads the two-direction output of layer k - 1):
    [ Wih [8Hp, 2Hp] | Whh [2, 4Hp, Hp] | bias_ih [8Hp] | bias_hh [8Hp] ], shadow: Wih, Whh.  Wih's 2H input columns sit at [0, H) and
    [Hp, Hp + H) -- where the recurrence writes the two directions, the placement linear.weight uses.  All at lr * lr_rate."""
    _FIELDS = ("wih", "whh", "bias_ih", "bias_hh")
    _KEYS = ("weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d")

    def __init__(self, k, rnn_state, hidden, Hp, device):
        self.k, self.H, self.Hp = int(k), int(hidden), int(Hp)
        self._alloc({"wih": (8 * Hp, 2 * Hp), "whh": (2, 4 * Hp, Hp), "bias_ih": (8 * Hp,), "bias_hh": (8 * Hp,)}, "bias_ih", device)
        self.grp = LSTMGroup.__new__(LSTMGroup)
        self.grp.H, self.grp.Hp, self.grp.ndir, self.grp.device = self.H, self.Hp, 2, self.device
        self.load_state(rnn_state)

    def keys(self, sfx=""):
        return [key % self.k + sfx for key in self._KEYS]

    def load_state(self, rnn):
        H, Hp = self.H, self.Hp
        pad = self.grp.pad_gates
        self.arena.zero_()
        wih, whh = torch.zeros(self.shapes["wih"], dtype=F32), torch.zeros(self.shapes["whh"], dtype=F32)
        bih, bhh = torch.zeros(8 * Hp, dtype=F32), torch.zeros(8 * Hp, dtype=F32)
        for d, sfx in enumerate(("", "_reverse")):
            kw, kh, kbi, kbh = self.keys(sfx)
            w = pad(rnn[kw])
            if tuple(w.shape) != (4 * Hp, 2 * H):
                raise ValueError("%s is %s, layer %d of a %d-unit BiLSTM reads [%d, %d]" % (kw, tuple(rnn[kw].shape), self.k, H, 4 * H, 2 * H))
            blk = slice(d * 4 * Hp, (d + 1) * 4 * Hp)
            wih[blk, :H], wih[blk, Hp:Hp + H] = w[:, :H], w[:, H:]
            whh[d, :, :H] = pad(rnn[kh])
            bih[blk], bhh[blk] = pad(rnn[kbi]), pad(rnn[kbh])
        for name, v in (("wih", wih), ("whh", whh), ("bias_ih", bih), ("bias_hh", bhh)):
            self.param(name).copy_(v.to(self.device))
        self.shadow.copy_(self.arena[:self.n_shadow])
        if self.g is not None:
            self.g.zero_()
        self._refresh()

    def state(self, buf=None):
        """the block (or a buffer laid out like it) under torch.nn.LSTM's names for layer k (host float32)"""
        H, Hp = self.H, self.Hp
        unpad = lambda t: torch.cat([t[q * Hp:q * Hp + H] for q in range(4)], 0)   # noqa: E731
        p = {name: self.param(name, buf).detach().cpu() for name in self._FIELDS}
        out = {}
        for d, sfx in enumerate(("", "_reverse")):
            kw, kh, kbi, kbh = self.keys(sfx)
            blk = slice(d * 4 * Hp, (d + 1) * 4 * Hp)
            w = unpad(p["wih"][blk])
            out[kw] = torch.cat([w[:, :H], w[:, Hp:Hp + H]], 1).contiguous()
            out[kh] = unpad(p["whh"][d])[:, :H].contiguous()
            out[kbi], out[kbh] = unpad(p["bias_ih"][blk]).contiguous(), unpad(p["bias_hh"][blk]).contiguous()
        return out

    def _refresh(self):
        Hp = self.Hp
        self.wih = self.shadow[:8 * Hp * 2 * Hp].view(8 * Hp, 2 * Hp)
        self.grp.whh = self.shadow[self.offsets["whh"]:self.n_shadow].view(2, 4 * Hp, Hp)
        self.bias = self.param("bias_ih") + self.param("bias_hh")
        self._whht = None


class InitState(_Block):
    """The trained initial state of the head's BiLSTM (train_initial_hidden_state: lstm_init_h / lstm_init_c, [2L, H] in torch's
    (layer, direction) order, row 2k + d; sequence_tagger_model.py:346-357): [ h [2L, Hp] | c [2L, Hp] ] in fp32, no shadow -- the
    recurrence starts from bf16(h) (its state type) and the fp32 c.  At lr * lr_rate."""
    _FIELDS = ("h", "c")

    def __init__(self, state, layers, hidden, Hp, device):
        self.L, self.H, self.Hp = int(layers), int(hidden), int(Hp)
        self._alloc({"h": (2 * self.L, Hp), "c": (2 * self.L, Hp)}, None, device)
        self.load_state(state)

    def load_state(self, state):
        self.arena.zero_()
        for name in self._FIELDS:
            v = torch.as_tensor(state["lstm_init_" + name]).detach().float().cpu()
            if tuple(v.shape) != (2 * self.L, self.H):
                raise ValueError("lstm_init_%s is %s, a %d-layer BiLSTM of %d units has [%d, %d]"
                                 % (name, tuple(v.shape), self.L, self.H, 2 * self.L, self.H))
            self.param(name)[:, :self.H] = v.to(self.device)
        if self.g is not None:
            self.g.zero_()
        self._refresh()

    def state(self, buf=None):
        return {"lstm_init_" + name: self.param(name, buf)[:, :self.H].detach().cpu().contiguous() for name in self._FIELDS}

    def _refresh(self):
        self.h16 = self.param("h").to(BF16)

    def of_layer(self, k):
        """-> (h_0 bf16 [2, Hp], c_0 f32 [2, Hp]) of layer k"""
        return self.h16[2 * k:2 * k + 2], self.param("c")[2 * k:2 * k + 2]


def rnn_layer_count(rnn_state):
    """the number of layers a torch.nn.LSTM state dict holds"""
    k = 0
    while "weight_ih_l%d" % k in rnn_state:
        k += 1
    return k


class BiLSTMHead:
    """BiLSTM(D -> hidden, L layers) + linear(2*hidden -> T) on the concatenated features (sequence_tagger_model.py:317-357,969-1027).
    Layer 0 and the linear / CRF parameters are the one-layer head's arena, unchanged; every layer above it (UpperLayer) and the
    trained initial state (InitState) are parameter blocks of their own beside it."""

    def __init__(self, rnn_state, linear_w, linear_b, blocks, hidden, device, transitions=None, trainable=False, rnn_layers=1,
                 init_state=None):
        """rnn_state: torch.nn.LSTM state dict (weight_ih_l{k}, weight_hh_l{k}, bias_ih_l{k}, bias_hh_l{k} and *_reverse, k < rnn_layers);
        init_state: None (the recurrences start from zeros) or {"lstm_init_h", "lstm_init_c"}, each [2 * rnn_layers, hidden];
        trainable (off by default: nothing more is allocated): enable_training() on this state and `transitions`;
        blocks: the widths D_i of the concatenated feature blocks in the reference's order (sorted embedding names).  Inside X
        every block starts at a multiple of 32 columns (`self.cols[i]`), so a producer whose width is padded (a 1000-unit LM
        writes 1024 columns, the last 24 zero) never touches its neighbour; Wih's columns are placed to match."""
        self.device = torch.device(device)
        self.blocks = [int(w) for w in blocks]
        self.D, self.H = sum(self.blocks), int(hidden)
        self.cols, off = [], 0
        for w in self.blocks:
            self.cols.append(off)
            off += _round_up(w, 32)
        self.Dp = _round_up(max(off, 1), 64)
        self.grp = LSTMGroup([rnn_state["weight_hh_l0"], rnn_state["weight_hh_l0_reverse"]], hidden, device)
        Hp = self.Hp = self.grp.Hp
        wih = torch.zeros((8 * Hp, self.Dp), dtype=F32)
        bias = torch.zeros(8 * Hp, dtype=F32)
        for d, sfx in enumerate(("", "_reverse")):
            w = self.grp.pad_gates(rnn_state["weight_ih_l0" + sfx])
            assert w.shape[1] == self.D, (w.shape, self.D)
            ref = 0
            for width, xc in zip(self.blocks, self.cols):
                wih[d * 4 * Hp:(d + 1) * 4 * Hp, xc:xc + width] = w[:, ref:ref + width]
                ref += width
            bias[d * 4 * Hp:(d + 1) * 4 * Hp] = self.grp.pad_gates(torch.as_tensor(rnn_state["bias_ih_l0" + sfx], dtype=F32)
                                                                   + torch.as_tensor(rnn_state["bias_hh_l0" + sfx], dtype=F32))
        self.wih = wih.to(BF16).to(self.device).contiguous()
        self.bias = bias.to(self.device)
        lw = torch.as_tensor(linear_w, dtype=F32)
        T = lw.shape[0]
        wl = torch.zeros((T, 2 * Hp), dtype=F32)
        wl[:, :self.H] = lw[:, :self.H]
        wl[:, Hp:Hp + self.H] = lw[:, self.H:2 * self.H]
        self.lin_w = wl.to(self.device).contiguous()
        self.lin_b = torch.as_tensor(linear_b, dtype=F32).to(self.device).contiguous()
        self.T = T
        self.arena = None
        self.training = False
        self.L = int(rnn_layers)
        if self.L < 1:
            raise ValueError("rnn_layers must be at least 1 (got %r)" % (rnn_layers,))
        if rnn_layer_count(rnn_state) != self.L:
            raise ValueError("the BiLSTM state holds %d layer(s), this head has rnn_layers=%d" % (rnn_layer_count(rnn_state), self.L))
        self.upper = [UpperLayer(k, rnn_state, self.H, Hp, self.device) for k in range(1, self.L)]
        self.init = None if init_state is None else InitState(init_state, self.L, self.H, Hp, self.device)
        self.rnn_dropout = 0.5 if self.L > 1 else 0.0      # torch.nn.LSTM(dropout=...) as the reference hard-codes it (:341-344)
        if trainable:
            self.enable_training(rnn_state, linear_w, linear_b, transitions)

    def rows(self, B, n):
        return _round_up(max(B * n, 1), 128)

    def new_input(self, B, n):
        """zeroed X bf16 [rows, Dp] the feature producers fill"""
        return torch.zeros((self.rows(B, n), self.Dp), dtype=BF16, device=self.device)

    def emissions(self, X, lengths, B, n):
        """X bf16 [rows, Dp] (token-major rows b*n + t, zero rows at padding) -> emissions f32 [B, n, T]"""
        with L_.stream_scope():
            Mp, Hp = X.shape[0], self.Hp
            gx = torch.empty((Mp, 8 * Hp), dtype=BF16, device=self.device)
            ops.gemm(GEMM_NT, X, self.wih, Mp, 8 * Hp, self.Dp, C=gx, bias=self.bias, epi=EPI_BIAS)
            tab = torch.from_numpy(step_tables(lengths, n)).to(self.device)
            out = torch.zeros((Mp, 2 * Hp), dtype=BF16, device=self.device)
            h0, c0 = self._init_of(0)
            self.grp.run(gx, tab, tab, out, Hp, B, h0=h0, c0=c0)
            for lay in self.upper:      # (no dropout between the layers outside training)
                gx = torch.empty((Mp, 8 * Hp), dtype=BF16, device=self.device)
                ops.gemm(GEMM_NT, out, lay.wih, Mp, 8 * Hp, 2 * Hp, C=gx, bias=lay.bias, epi=EPI_BIAS)
                out = torch.zeros((Mp, 2 * Hp), dtype=BF16, device=self.device)
                h0, c0 = self._init_of(lay.k)
                lay.grp.run(gx, tab, tab, out, Hp, B, h0=h0, c0=c0)
            em = ops.head_fwd(out[:B * n], self.lin_w, self.lin_b)
        return em.view(B, n, self.T)

    def _init_of(self, k):
        """(h_0 bf16, c_0 f32), each [2, Hp], of layer k -- (None, None) without a trained initial state: zeros"""
        return (None, None) if self.init is None else self.init.of_layer(k)

    def blocks_extra(self):
        """the parameter blocks beside the one-layer arena, in the order the optimizer steps them: upper layers, initial state"""
        return list(self.upper) + ([self.init] if self.init is not None else [])


    # ------------------------------------------------------------------ training (opt-in)
    # One flat fp32 arena p with a gradient buffer g and a bf16 shadow of the two GEMM / recurrence operands, in the padded device
    # layouts.  The reference's two parameter groups (finetune_trainer.py:552-571) are two contiguous ranges:
    #   [ Wih [8Hp, Dq] | Whh [2, 4Hp, Hp] | bias_ih [8Hp] | bias_hh [8Hp] | transitions [T, T] ]  at lr * lr_rate   (shadow: Wih, Whh)
    #   [ linear.weight [T, 2Hp] | linear.bias [T] ]                                                at lr
    # Dq = Dp rounded up to 128: the weight-gradient GEMM dWih = dgx^T X takes N in multiples of 128, so the TRAINING side pads X and
    # Wih (zero columns); the inference layout (Dp, new_input) is as it was.  dWhh comes from one GEMM against the two-direction-wide
    # hprev [rows, 2Hp] whose cross blocks are discarded.  bias_ih and bias_hh stay two parameters (the reference trains both; they
    # receive the same gradient, so under AdamW their sum moves twice); the forward adds them.  Padded entries have zero weights and
    # receive exactly zero gradients (a padded unit's gates see dh = 0 and carry 0), so they stay zero.
    _FIELDS = ("wih", "whh", "bias_ih", "bias_hh", "transitions", "linear.weight", "linear.bias")

    def enable_training(self, rnn_state, linear_w, linear_b, transitions):
        Hp, T = self.Hp, self.T
        self.Dq = _round_up(self.Dp, 128)
        shapes = {"wih": (8 * Hp, self.Dq), "whh": (2, 4 * Hp, Hp), "bias_ih": (8 * Hp,), "bias_hh": (8 * Hp,), "transitions": (T, T),
                  "linear.weight": (T, 2 * Hp), "linear.bias": (T,)}
        self.shapes, self.offsets, off = shapes, {}, 0
        for k in self._FIELDS:
            self.offsets[k] = off
            off += _round_up(int(np.prod(shapes[k])), 4)
        self.n = off
        self.n_shadow = self.offsets["bias_ih"]
        self.split = self.offsets["linear.weight"]
        dev = self.device
        self.arena = torch.zeros(self.n, dtype=F32, device=dev)
        self.g = torch.zeros(self.n, dtype=F32, device=dev)
        self.shadow = torch.zeros(self.n_shadow, dtype=BF16, device=dev)
        self.dropout = self.word_dropout = self.locked_dropout = 0.0
        self._drop_rng = np.random.default_rng(0)
        self.last_drop = None
        for blk in self.blocks_extra():     # (a one-layer head without an initial state has none)
            blk.enable_training()
        self.load_state({"rnn": rnn_state, "linear.weight": linear_w, "linear.bias": linear_b, "transitions": transitions},
                        _extra=False)

    def param(self, name, buf=None):
        buf = self.arena if buf is None else buf
        o, shp = self.offsets[name], self.shapes[name]
        return buf[o:o + int(np.prod(shp))].view(shp)

    def grad(self, name):
        return self.param(name, self.g)

    def load_state(self, state, _extra=True):
        """the reference-layout dict load_stack_state takes -> the arena (padded layouts) and, of a deeper head or one with a trained
        initial state, the blocks beside it; the inverse of state()"""
        Hp, H, T = self.Hp, self.H, self.T
        rnn = state["rnn"]
        if rnn_layer_count(rnn) != self.L:
            raise ValueError("the state holds a BiLSTM of %d layer(s), this head has rnn_layers=%d" % (rnn_layer_count(rnn), self.L))
        if _extra:
            if ("lstm_init_h" in state) != (self.init is not None):
                raise ValueError("the state %s a trained initial state (lstm_init_h / lstm_init_c), this head %s"
                                 % (("carries", "has none") if "lstm_init_h" in state else ("carries no", "has one")))
            for lay in self.upper:
                lay.load_state(rnn)
            if self.init is not None:
                self.init.load_state(state)
        self.arena.zero_()
        wih, whh = torch.zeros(self.shapes["wih"], dtype=F32), torch.zeros(self.shapes["whh"], dtype=F32)
        bih, bhh = torch.zeros(8 * Hp, dtype=F32), torch.zeros(8 * Hp, dtype=F32)
        for d, sfx in enumerate(("", "_reverse")):
            w = self.grp.pad_gates(rnn["weight_ih_l0" + sfx])
            ref = 0
            for width, xc in zip(self.blocks, self.cols):
                wih[d * 4 * Hp:(d + 1) * 4 * Hp, xc:xc + width] = w[:, ref:ref + width]
                ref += width
            whh[d, :, :H] = self.grp.pad_gates(rnn["weight_hh_l0" + sfx])
            bih[d * 4 * Hp:(d + 1) * 4 * Hp] = self.grp.pad_gates(rnn["bias_ih_l0" + sfx])
            bhh[d * 4 * Hp:(d + 1) * 4 * Hp] = self.grp.pad_gates(rnn["bias_hh_l0" + sfx])
        lw = torch.as_tensor(state["linear.weight"], dtype=F32)
        wl = torch.zeros((T, 2 * Hp), dtype=F32)
        wl[:, :H], wl[:, Hp:Hp + H] = lw[:, :H], lw[:, H:2 * H]
        for k, v in (("wih", wih), ("whh", whh), ("bias_ih", bih), ("bias_hh", bhh), ("linear.weight", wl),
                     ("linear.bias", torch.as_tensor(state["linear.bias"], dtype=F32)),
                     ("transitions", torch.as_tensor(state["transitions"], dtype=F32))):
            self.param(k).copy_(v.to(self.device))
        self.shadow.copy_(self.arena[:self.n_shadow])
        self.g.zero_()
        self._refresh()

    def state(self, buf=None):
        """the arena (or a buffer laid out like it) in the reference's layout: {"rnn": torch.nn.LSTM state dict, "linear.weight",
        "linear.bias", "transitions"} (host float32).  load_state(state()) reproduces the arena bit for bit."""
        Hp, H = self.Hp, self.H
        unpad = lambda t: torch.cat([t[q * Hp:q * Hp + H] for q in range(4)], 0)   # noqa: E731
        p = {k: self.param(k, buf).detach().cpu() for k in self._FIELDS}
        rnn = {}
        for d, sfx in enumerate(("", "_reverse")):
            w = unpad(p["wih"][d * 4 * Hp:(d + 1) * 4 * Hp])
            rnn["weight_ih_l0" + sfx] = torch.cat([w[:, xc:xc + width] for width, xc in zip(self.blocks, self.cols)], 1).contiguous()
            rnn["weight_hh_l0" + sfx] = unpad(p["whh"][d])[:, :H].contiguous()
            rnn["bias_ih_l0" + sfx] = unpad(p["bias_ih"][d * 4 * Hp:(d + 1) * 4 * Hp]).contiguous()
            rnn["bias_hh_l0" + sfx] = unpad(p["bias_hh"][d * 4 * Hp:(d + 1) * 4 * Hp]).contiguous()
        lw = p["linear.weight"]
        out = {"rnn": rnn, "linear.weight": torch.cat([lw[:, :H], lw[:, Hp:Hp + H]], 1).contiguous(),
               "linear.bias": p["linear.bias"].clone(), "transitions": p["transitions"].clone()}
        if buf is None:     # (a buffer is laid out like the one-layer arena: the blocks beside it have buffers of their own)
            for lay in self.upper:
                rnn.update(lay.state())
            if self.init is not None:
                out.update(self.init.state())
        return out

    def state_of(self, buf):
        """a buffer laid out like the arena (the gradient, an optimizer moment) in the reference's layout"""
        return self.state(buf)

    def grad_state(self):
        """every gradient in the reference's layout: state_of(g) with the upper layers' and the initial state's"""
        out = self.state(self.g)
        for lay in self.upper:
            out["rnn"].update(lay.state(lay.g))
        if self.init is not None:
            out.update(self.init.state(self.init.g))
        return out

    def zero_grad(self):
        self.g.zero_()
        for blk in self.blocks_extra():
            blk.g.zero_()

    def _refresh(self):
        """after the arena changed (optimizer step, load_state): what emissions() and loss_backward() read"""
        Hp = self.Hp
        sh = self.shadow
        self.wih_t = sh[:8 * Hp * self.Dq].view(8 * Hp, self.Dq)
        self.wih = self.wih_t if self.Dq == self.Dp else self.wih_t[:, :self.Dp].contiguous()
        self.grp.whh = sh[self.offsets["whh"]:self.n_shadow].view(2, 4 * Hp, Hp)
        self.bias = self.param("bias_ih") + self.param("bias_hh")
        self.lin_w, self.lin_b = self.param("linear.weight"), self.param("linear.bias")
        self._whht = None
        for blk in self.blocks_extra():
            blk._refresh()

    def seed_dropout(self, seed):
        self._drop_rng = np.random.default_rng(int(seed))

    def train(self, mode=True):
        self.training = bool(mode) and self.arena is not None
        return self

    def _draw_dropout(self, n):
        """one training forward's dropout sites, drawn from the head's counter-based stream: (word-dropped positions bool [n] or
        None, pre-RNN (element, locked) sites, post-RNN (element, locked) sites), each site a (seed, thresh) pair.  A head of L > 1
        layers draws, after these, the L - 1 element sites between its layers (rate rnn_dropout) as a fourth item -- also when the
        three rates above are 0; a one-layer head draws exactly what it always drew."""
        if not self.training or not (self.dropout or self.word_dropout or self.locked_dropout or self.L > 1):
            return None
        word = (self._drop_rng.random(n) < self.word_dropout) if self.word_dropout > 0.0 else None
        sd = self._drop_rng.integers(0, 2 ** 32, size=4, dtype="uint64")
        te, tl = ops.drop_thresh(self.dropout), ops.drop_thresh(self.locked_dropout)
        sites = word, ((int(sd[0]), te), (int(sd[1]), tl)), ((int(sd[2]), te), (int(sd[3]), tl))
        if self.L > 1:
            si = self._drop_rng.integers(0, 2 ** 32, size=self.L - 1, dtype="uint64")
            sites += (tuple((int(x), ops.drop_thresh(self.rnn_dropout)) for x in si),)
        return sites

    def loss_backward(self, X, lengths, B, n, batch, start, stop, loss_scale=1.0, weights=None, drop="draw", source=None, char=None):
        """One micro-batch of head training on constant features: forward, CRF NLL, and loss_scale * its gradient ADDED to self.g.
        X bf16 [rows, Dp] as new_input() lays it out -- or None with `source`, a FeatureStore.source() of the batch: the first stage
        (the pre-RNN dropouts and the padding to Dq) is then one kbner_gather_rows_blocks_drop from the stored rows; batch: the device dict of kbner.batch (ctags i32 [B, nc], clens i32 [B],
        cfeat_idx i32 [B * nc]: the S-X compaction of the emissions); weights f32 [B] replace the 1 / B of the batch mean.
        Sequence (sequence_tagger_model.py:959-964,969-994,1027 and the CRF loss): the three pre-RNN dropouts as one
        gather_rows_drop over X with an identity index (WordDropout: index -1), input GEMM, kbner_lstm_seq_train, the two post-RNN
        dropouts, head, compaction, CRF NLL forward / backward, and back through the same chain to kbner_lstm_seq_bwd and the weight
        gradients.  Nothing flows into X.  char: a CharStep (the trainable character BiLSTM's batch), or None: it writes its block
        into the matrix the input GEMM reads, after the first stage has produced it, applying the pre-RNN sites itself; after the
        recurrence's backward the block's window of dXt = dgx . Wih is handed to it.  -> the loss, a 0-d device tensor."""
        if self.arena is None:
            raise L_.KbnerError("this BiLSTMHead was not built for training (enable_training())")
        with L_.stream_scope():
            dev, Hp, T, R = self.device, self.Hp, self.T, B * n
            X_in = X
            Mp = self.rows(B, n) if source is not None else X.shape[0]
            sites = self._draw_dropout(n) if drop == "draw" else drop
            self.last_drop = sites
            ident = None
            inter = None       # the element sites between the layers (a fourth item of `sites`: heads of more than one layer)
            if sites is not None:
                word, pre, post = sites[:3]
                inter = sites[3] if len(sites) > 3 else None
                ident = torch.arange(R, dtype=I32, device=dev)
            if source is not None:
                # the whole first stage as ONE launch from the stored rows: Xt [Mp, Dq] written whole (padding rows and columns too)
                Xt = FeatureStore.launch(source, Mp, self.Dq, None if sites is None else (word, pre[0], pre[1]))
            else:
                if sites is not None:
                    idx = ident
                    if word is not None:
                        idx = torch.where(torch.from_numpy(np.tile(word, B)).to(dev), torch.full_like(ident, -1), ident)
                    Xd = torch.zeros((Mp, self.Dp), dtype=BF16, device=dev)
                    ops.gather_rows_drop(X, idx, n, pre[0], pre[1], out=Xd)
                    X = Xd
                if self.Dq != self.Dp:
                    Xt = torch.zeros((Mp, self.Dq), dtype=BF16, device=dev)
                    Xt[:, :self.Dp] = X
                else:
                    Xt = X
            if char is not None:
                if Xt is X_in:       # no site drawn and no Dq pad: the caller's X would receive the block -- it never lives in X
                    Xt = X_in.clone()
                char.forward(Xt, sites, n)
            gx = torch.empty((Mp, 8 * Hp), dtype=BF16, device=dev)
            ops.gemm(GEMM_NT, Xt, self.wih_t, Mp, 8 * Hp, self.Dq, C=gx, bias=self.bias, epi=EPI_BIAS)
            out = torch.zeros((Mp, 2 * Hp), dtype=BF16, device=dev)
            deep = self.L > 1 or self.init is not None      # (a one-layer head from zeros launches what it always launched)
            h0, c0 = self._init_of(0)
            saved = self.grp.run_train(gx, step_tables(lengths, n), out, B, [0, Hp], h0=h0, c0=c0)
            upper = []         # per upper layer: (layer, the matrix its input GEMM read, what its recurrence saved, its site)
            for lay in self.upper:
                site = inter[lay.k - 1] if inter is not None else ops.NO_DROP
                inp = out
                if site[1]:    # torch.nn.LSTM's dropout on the output of every layer but the last: element site only
                    inp = torch.zeros((Mp, 2 * Hp), dtype=BF16, device=dev)
                    ops.gather_rows_drop(out, ident, n, site, ops.NO_DROP, out=inp)
                gxk = torch.empty((Mp, 8 * Hp), dtype=BF16, device=dev)
                ops.gemm(GEMM_NT, inp, lay.wih, Mp, 8 * Hp, 2 * Hp, C=gxk, bias=lay.bias, epi=EPI_BIAS)
                out = torch.zeros((Mp, 2 * Hp), dtype=BF16, device=dev)
                h0, c0 = self._init_of(lay.k)
                upper.append((lay, inp, lay.grp.run_train(gxk, step_tables(lengths, n), out, B, [0, Hp], h0=h0, c0=c0), site))
            post_on = sites is not None and bool(post[0][1] or post[1][1])
            feat = ops.gather_rows_drop(out, ident, n, post[0], post[1]) if post_on else out[:R]
            em = ops.head_fwd(feat, self.lin_w, self.lin_b)
            self.last_out, self.last_feat = out, feat      # (tests read the dropout sites back from these)
            nc = batch["ctags"].shape[1]
            comp = ops.gather_rows_f32(em, batch["cfeat_idx"]).view(B, nc, T)
            trans = self.param("transitions")
            logz, gold, alpha = ops.crf_nll_fwd(comp, trans, batch["ctags"], batch["clens"], start, stop)
            w = torch.full((B,), 1.0 / B, dtype=F32, device=dev) if weights is None else torch.as_tensor(
                weights, dtype=F32, device=dev).contiguous()
            if w.numel() != B:
                raise ValueError("weights must hold one value per sentence")
            loss = torch.empty((1,), dtype=F32, device=dev)
            ops.wdiff_sum(logz, gold, w, loss)
            self.last_emissions = em.view(B, n, T)
            # ---- backward
            dcomp = ops.crf_nll_bwd(comp, trans, batch["ctags"], batch["clens"], alpha, logz, w * float(loss_scale), start, stop,
                                    self.grad("transitions"))
            dem = torch.zeros((R, T), dtype=F32, device=dev)
            # (kbner_scatter_rows_f32 moves float4s: tag counts that are no multiple of 4 take the adding scatter onto the zeros)
            (ops.scatter_rows_f32 if T % 4 == 0 else ops.scatter_add_rows_f32)(dcomp.view(B * nc, T), batch["cfeat_idx"], dem)
            dfeat = ops.head_bwd(dem, feat, self.lin_w, self.grad("linear.weight"), self.grad("linear.bias"))
            if post_on:
                dout = torch.zeros((R, 2 * Hp), dtype=BF16, device=dev)
                ops.scatter_rows_drop(dfeat, ident, dout, n, post[0], post[1])
            else:
                dout = dfeat
            # the layers above the first, last one first: each hands the gradient of its input to the layer below
            for lay, inp, sv, site in reversed(upper):
                if lay._whht is None:
                    lay._whht = lay.grp.whh_t()
                dgxk = self._recurrence_bwd(lay.grp, lay.k, dout, sv, lay._whht, True)
                self._weight_grads(dgxk, inp, 2 * Hp, sv["hprev"], Mp, lay.grad)
                dinp = torch.empty((Mp, 2 * Hp), dtype=BF16, device=dev)
                ops.gemm(GEMM_NN, dgxk, lay.wih, Mp, 2 * Hp, 8 * Hp, C=dinp)
                if site[1]:
                    dout = torch.zeros((Mp, 2 * Hp), dtype=BF16, device=dev)
                    ops.scatter_rows_drop(dinp, ident, dout, n, site, ops.NO_DROP)
                else:
                    dout = dinp
            if self._whht is None:
                self._whht = self.grp.whh_t()
            dgx = self._recurrence_bwd(self.grp, 0, dout, saved, self._whht, deep)
            self._weight_grads(dgx, Xt, self.Dq, saved["hprev"], Mp, self.grad)
            if char is not None:
                # the one window of dXt = dgx . Wih anything reads: the character block's columns.  The GEMM takes N in multiples of
                # 128, so the window is CHAR_WINDOW columns of wih_t (leading dimension Dq) that contain the block.
                assert self.Dq >= CHAR_WINDOW and self.Dq % CHAR_WINDOW == 0      # (Dq is Dp rounded up to 128: enable_training)
                c0 = min(char.col, self.Dq - CHAR_WINDOW)
                dwin = torch.empty((Mp, CHAR_WINDOW), dtype=BF16, device=dev)
                ops.gemm(GEMM_NN, dgx, self.wih_t.reshape(-1)[c0:], Mp, CHAR_WINDOW, 8 * Hp, C=dwin, lda=8 * Hp, ldb=self.Dq)
                char.backward(dwin, char.col - c0, n)
        return loss[0]

    def _recurrence_bwd(self, grp, k, dout, saved, whh_t, deep):
        """layer k's walk back through time -> dgx.  deep: through kbner_lstm_seq_bwd_init; with a trained initial state the
        gradients of c_0 and h_0, summed over the batch, are added to rows 2k, 2k + 1 of its gradient"""
        if not deep:
            return grp.run_bwd(dout, saved, whh_t)
        dgx, dc0, dh0 = grp.run_bwd(dout, saved, whh_t, state_grads=True)
        if self.init is not None:
            B = saved["B"]
            for d in range(2):
                ops.colsum_rows_f32(dc0[d], B, self.init.grad("c")[2 * k + d])
                ops.colsum_rows_f32(dh0[d], B, self.init.grad("h")[2 * k + d])
        return dgx

    def _weight_grads(self, dgx, inp, W, hprev, Mp, grad):
        """one layer's dWih = dgx^T inp ([8Hp, W]), dWhh from dgx^T hprev and both bias gradients, ADDED to grad(name): fp32 atomic
        accumulation on the 128x128 kernel (lda given: it takes N in multiples of 128), the row (reduction) dimension split until
        the launch has enough workgroups"""
        Hp, dev = self.Hp, self.device
        sk = 1
        while (8 * Hp // 128) * (W // 128) * sk < 768 and Mp % (128 * sk) == 0 and sk < 64:
            sk *= 2
        ops.gemm(GEMM_TN, dgx, inp, 8 * Hp, W, Mp, C32=grad("wih"), epi=EPI_ATOMIC32, splitk=sk, lda=8 * Hp)
        cross = torch.zeros((8 * Hp, 2 * Hp), dtype=F32, device=dev)
        sk = 1
        while (8 * Hp // 128) * (2 * Hp // 128) * sk < 768 and Mp % (128 * sk) == 0 and sk < 64:
            sk *= 2
        ops.gemm(GEMM_TN, dgx, hprev, 8 * Hp, 2 * Hp, Mp, C32=cross, epi=EPI_ATOMIC32, splitk=sk, lda=8 * Hp)
        gw = grad("whh")
        gw[0] += cross[:4 * Hp, :Hp]
        gw[1] += cross[4 * Hp:, Hp:]
        ops.colsum(dgx, grad("bias_ih"))
        ops.colsum(dgx, grad("bias_hh"))


CHAR_WINDOW = 128       # columns of the dXt window computed for the character block (the GEMM's N granule)


class CharBiLSTM:
    """The trainable parameters of FastCharacterEmbeddings on the device (flair/embeddings.py:670-758: char_embedding, char_layer): one
    flat fp32 arena with a gradient buffer, in torch's layouts -- kbner_char_lstm_fwd / _bwd read them as they are, so there is no
    shadow copy.  [ emb [V, E] | wih [2, 4Hc, E] | whh [2, 4Hc, Hc] | bias_ih [2, 4Hc] | bias_hh [2, 4Hc] ], all at the plain learning
    rate (names containing 'embedding', finetune_trainer.py:552-553)."""
    _FIELDS = ("emb", "wih", "whh", "bias_ih", "bias_hh")
    _KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

    def __init__(self, state, device):
        """state: {"char_embedding.weight", "char_layer.weight_ih_l0", ... "_reverse"} (FastCharacterEmbeddings.state_dict())"""
        self.device = torch.device(device)
        V, E = state["char_embedding.weight"].shape
        Hc = state["char_layer.weight_hh_l0"].shape[1]
        self.V, self.E, self.Hc = int(V), int(E), int(Hc)
        self.shapes = {"emb": (V, E), "wih": (2, 4 * Hc, E), "whh": (2, 4 * Hc, Hc), "bias_ih": (2, 4 * Hc), "bias_hh": (2, 4 * Hc)}
        self.offsets, off = {}, 0
        for k in self._FIELDS:
            self.offsets[k] = off
            off += _round_up(int(np.prod(self.shapes[k])), 4)
        self.n = off
        self.arena = torch.zeros(self.n, dtype=F32, device=self.device)
        self.g = torch.zeros(self.n, dtype=F32, device=self.device)
        self.load_state(state)

    def param(self, name, buf=None):
        buf = self.arena if buf is None else buf
        o, shp = self.offsets[name], self.shapes[name]
        return buf[o:o + int(np.prod(shp))].view(shp)

    def grad(self, name):
        return self.param(name, self.g)

    def load_state(self, state):
        f = lambda k: torch.as_tensor(state[k]).detach().float().cpu()   # noqa: E731
        parts = {"emb": f("char_embedding.weight")}
        for name, key in zip(self._FIELDS[1:], self._KEYS):
            parts[name] = torch.stack([f("char_layer." + key), f("char_layer." + key + "_reverse")])
        for k, v in parts.items():
            if tuple(v.shape) != tuple(self.shapes[k]):
                raise ValueError("character state: %s is %s, this embedding's is %s" % (k, tuple(v.shape), tuple(self.shapes[k])))
            self.param(k).copy_(v.to(self.device))
        self.g.zero_()

    def state(self, buf=None):
        """the arena (or a buffer laid out like it) under the reference's parameter names (host float32)"""
        p = {k: self.param(k, buf).detach().cpu() for k in self._FIELDS}
        out = {"char_embedding.weight": p["emb"].clone()}
        for name, key in zip(self._FIELDS[1:], self._KEYS):
            out["char_layer." + key] = p[name][0].clone()
            out["char_layer." + key + "_reverse"] = p[name][1].clone()
        return out


class CharStep:
    """One batch of the character BiLSTM inside a step of the head: the host word tables (FastCharacterEmbeddings.char_batch), the
    block's column, and what the forward saved for the backward.  The placement rule: the block is written into the matrix the input
    GEMM reads -- Xt while training (its columns arrive there as zeros), X itself in a forward-only pass -- never into the stored
    features; the kernel applies the pre-RNN masks itself."""

    def __init__(self, net, chars, lens, rows, col):
        self.net, self.col = net, int(col)
        self.chars, self.lens, self.rows = chars, lens, np.asarray(rows)
        self.tab = self.ws = self.sites = None

    def _params(self):
        return [self.net.param(k) for k in CharBiLSTM._FIELDS]

    def forward(self, Xt, sites, n, save=True):
        """sites: None or (word: WordDropout positions bool [n] or None, (element site, locked site), ...) as the head draws them"""
        rows, se, sl = self.rows, ops.NO_DROP, ops.NO_DROP
        if sites is not None:
            word, (se, sl) = sites[0], sites[1]
            if word is not None:
                live = rows >= 0
                rows = np.where(live & np.asarray(word, bool)[np.where(live, rows, 0) % n], -1, rows)
        self.tab = ops.CharTables(self.chars, self.lens, rows, self.net.V, Xt.shape[0], Xt.device)
        self.sites = (se, sl)
        self.ws = ops.char_lstm_ws(self.tab, self.net.Hc, Xt.device) if save and self.tab.W else None
        ops.char_lstm_fwd(*self._params(), self.tab, Xt, self.col, n, se, sl, ws=self.ws)

    def backward(self, dwin, col, n):
        """dwin bf16 [rows, *]: the gradient of the matrix the forward wrote into, its block at column `col` of dwin"""
        net = self.net
        p = self._params()
        tab = self.tab
        if dwin.shape[0] < tab.n_rows:
            raise L_.KbnerError("CharStep.backward: the gradient window holds fewer rows than the forward's matrix")
        ops.char_lstm_bwd(dwin, col, p[0], p[1], p[2], tab, self.ws, *[net.grad(k) for k in CharBiLSTM._FIELDS], n, self.sites[0],
                          self.sites[1], key_col=self.col)


class FeatureStore:
    """The frozen features of the stacked tagger, computed once (flair's `embeddings_storage_mode`, training_utils.store_embeddings:
    the reference keeps every embedding's vectors on the tokens after their first computation; here they are rows of ONE matrix).
    Compact bf16 rows [tokens, Dp] in the head's column layout, one contiguous run of len(sentence) rows per sentence, keyed by the
    sentence object (the store holds a reference, so an id is never reused).  A stored sentence's features are the bits of its FIRST
    computation, in the batch it was first seen in.

        mode "gpu": one device matrix, grown in steps of CHUNK_ROWS rows (growing copies the rows in use: old and new matrix exist
                    together for the length of that copy); budget MAX_FRACTION of the free device memory at opening
        mode "cpu": pinned host chunks of CHUNK_ROWS rows (budget: MAX_FRACTION of the free host memory); a batch's rows are gathered
                    on the host into one pinned staging buffer and copied to the device on the current stream (non-blocking)

    Reading is ONE launch of kbner_gather_rows_blocks_drop: padding rows (index -1), the embedding selection (block_on) and the
    head's pre-RNN dropouts on the way out, into the padded matrix the consumer asks for.  The store remembers which column blocks
    were computed when it was filled (`have`: the embedding selection in force then); a later selection that is a subset is served
    by block_on, one that needs a missing block empties the store.  A batch with any sentence missing is not served (the caller
    recomputes it whole); at the budget the store stops accepting sentences."""
    MAX_FRACTION = 0.5
    CHUNK_ROWS = 16384

    def __init__(self, mode, Dp, block_col, device, budget_bytes=None):
        if mode not in ("gpu", "cpu"):
            raise ValueError("FeatureStore mode must be 'gpu' or 'cpu' (got %r; 'none' is: no store)" % (mode,))
        self.mode, self.Dp, self.device = mode, int(Dp), torch.device(device)
        self.block_col_host = ops.check_block_cols(block_col, self.Dp)
        self.nblk = len(self.block_col_host) - 1
        self.block_col = torch.tensor(self.block_col_host, dtype=I32, device=self.device)
        if budget_bytes is None:
            if mode == "gpu":
                budget_bytes = self.MAX_FRACTION * torch.cuda.mem_get_info(self.device)[0]
            else:
                import os
                budget_bytes = self.MAX_FRACTION * os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
        self.budget_rows = int(budget_bytes) // (2 * self.Dp)
        self.pin = self.device.type == "cuda"
        self.hits = self.misses = 0
        self._staging = self._staged = None
        self._warned = set()
        self.want = [True] * self.nblk
        self.block_on = torch.ones(self.nblk, dtype=torch.uint8, device=self.device)
        self.clear()

    # ---- bookkeeping
    def clear(self):
        self.index = {}            # id(sentence) -> (sentence, chunk, first row, rows)
        self.chunks = []           # "gpu": at most one matrix [capacity, Dp]; "cpu": pinned host chunks [>= CHUNK_ROWS, Dp]
        self.rows = 0              # rows stored
        self._used = 0             # rows in use in the last chunk
        self.have = None
        self.full = False

    close = clear

    @property
    def nbytes(self):
        return self.rows * self.Dp * 2

    def __len__(self):
        return len(self.index)

    def _log_once(self, key, msg, *args):
        if key not in self._warned:
            self._warned.add(key)
            import logging
            logging.getLogger("flair").info(msg, *args)

    def select(self, on):
        """the embedding selection of the next reads and writes: one bool per block.  A block the store lacks empties it."""
        on = [bool(x) for x in on]
        if len(on) != self.nblk:
            raise ValueError("FeatureStore.select: one switch per block (%d)" % self.nblk)
        if self.have is not None and any(o and not h for o, h in zip(on, self.have)):
            import logging
            logging.getLogger("flair").info("feature store: the selection needs a block that was not stored; %d sentences dropped, "
                                            "the store refills", len(self.index))
            self.clear()
        if on != self.want:
            self.want = on
            self.block_on = torch.tensor([1 if o else 0 for o in on], dtype=torch.uint8, device=self.device)

    def lookup(self, sentences):
        """-> [(chunk, first row, rows)] per sentence, or None when any of them is missing"""
        out = []
        for s in sentences:
            e = self.index.get(id(s))
            if e is None:
                self.misses += 1
                return None
            out.append(e[1:])
        self.hits += 1
        return out

    # ---- writing
    def _room(self, rows):
        """-> (chunk, first row) of `rows` free contiguous rows, or None at the budget"""
        if self.mode == "gpu":
            cap = self.chunks[0].shape[0] if self.chunks else 0
            if self.rows + rows > cap:
                new = min(_round_up(self.rows + rows, self.CHUNK_ROWS), self.budget_rows)
                if new < self.rows + rows:
                    return None
                grown = torch.empty((new, self.Dp), dtype=BF16, device=self.device)
                if self.rows:
                    grown[:self.rows] = self.chunks[0][:self.rows]
                self.chunks = [grown]
            return 0, self.rows
        if not self.chunks or self._used + rows > self.chunks[-1].shape[0]:
            # a batch's rows never straddle two chunks: the rest of the last one stays unused
            size = max(self.CHUNK_ROWS, rows)
            if sum(c.shape[0] for c in self.chunks) + size > self.budget_rows:
                return None
            self.chunks.append(torch.empty((size, self.Dp), dtype=BF16, pin_memory=self.pin))
            self._used = 0
        return len(self.chunks) - 1, self._used

    def add(self, sentences, X, lengths, n):
        """pack the real-token rows of a freshly computed X bf16 [rows, Dp] (token-major rows b * n + t) into the store: one
        kbner_gather_rows_ld per batch.  Only whole batches computed under the selection the store was filled with are taken."""
        if self.full:
            return False
        if self.have is not None and self.want != self.have:
            self._log_once("subset", "feature store: a batch computed under a narrower selection than the stored one is not stored")
            return False
        new = [(b, s) for b, s in enumerate(sentences) if id(s) not in self.index]
        total = sum(int(lengths[b]) for b, _ in new)
        if not new or total == 0:
            return False
        at = self._room(total)
        if at is None:
            self.full = True
            self._log_once("full", "feature store (%s): budget of %d rows reached at %d sentences; later sentences are recomputed",
                           self.mode, self.budget_rows, len(self.index))
            return False
        chunk, r0 = at
        src = np.concatenate([b * n + np.arange(int(lengths[b])) for b, _ in new]).astype(np.int32)
        idx = torch.from_numpy(src).to(self.device)
        if self.mode == "gpu":
            ops.gather_rows_into(X, idx, self.chunks[0][r0:r0 + total], 0, self.Dp)
        else:
            packed = torch.empty((total, self.Dp), dtype=BF16, device=self.device)
            ops.gather_rows_into(X, idx, packed, 0, self.Dp)
            self.chunks[chunk][r0:r0 + total].copy_(packed)      # (blocking: the first visit of a sentence only)
        off = r0
        for b, s in new:
            self.index[id(s)] = (s, chunk, off, int(lengths[b]))
            off += int(lengths[b])
        self._used = off
        self.rows += total
        self.have = list(self.want)
        return True

    # ---- reading
    def source(self, sentences, n):
        """what one launch of kbner_gather_rows_blocks_drop reads for this batch: {"store": bf16 [*, Dp] on the device, "idx": host
        int32 [B * n] (-1 at padding positions), "block_col", "block_on", "n"} -- or None when a sentence is missing"""
        found = self.lookup(sentences)
        if found is None:
            return None
        B = len(found)
        idx = np.full((B, n), -1, np.int32)
        if self.mode == "gpu":
            for b, (_, r0, rows) in enumerate(found):
                idx[b, :rows] = np.arange(r0, r0 + rows)
            store = self.chunks[0]
        else:
            total = sum(rows for _, _, rows in found)
            if self._staging is None or self._staging.shape[0] < total:
                cap = _round_up(max(total, 1), 1024)
                self._staging = torch.empty((cap, self.Dp), dtype=BF16, pin_memory=self.pin)
                self._staged = None
            if self._staged is not None:
                self._staged.synchronize()      # the previous batch's copy has left the staging buffer
            off = 0
            for b, (chunk, r0, rows) in enumerate(found):
                self._staging[off:off + rows] = self.chunks[chunk][r0:r0 + rows]
                idx[b, :rows] = np.arange(off, off + rows)
                off += rows
            store = torch.empty((max(total, 1), self.Dp), dtype=BF16, device=self.device)
            store[:total].copy_(self._staging[:total], non_blocking=True)
            if self.pin:
                self._staged = torch.cuda.Event()
                self._staged.record()
        return {"store": store, "idx": idx.reshape(-1), "block_col": self.block_col, "block_on": self.block_on, "n": int(n)}

    @staticmethod
    def launch(source, R_out, ld_out, drop=None):
        """one kbner_gather_rows_blocks_drop over a source -> bf16 [R_out, ld_out], every element written.  drop: None or (word: the
        WordDropout positions, bool [n] or None -- folded into the index as -1 --, element site, locked site)"""
        idx, n = source["idx"], source["n"]
        site_e = site_l = ops.NO_DROP
        if drop is not None:
            word, site_e, site_l = drop
            if word is not None:
                idx = np.where(np.tile(np.asarray(word, bool), idx.size // n), np.int32(-1), idx).astype(np.int32)
        store = source["store"]
        return ops.gather_rows_blocks_drop(store, torch.from_numpy(idx).to(store.device), source["block_col"], source["block_on"], n,
                                           R_out=R_out, ld_out=ld_out, drop_e=site_e, drop_l=site_l)

    def assemble(self, sentences, n, out_ld, drop=None):
        """the batch's matrix bf16 [B * n padded to 128, out_ld] from the store, or None when a sentence is missing"""
        src = self.source(sentences, n)
        if src is None:
            return None
        return self.launch(src, _round_up(max(len(sentences) * n, 1), 128), out_ld, drop)


class StackOptimizer:
    """The optimizer of a trainable BiLSTMHead over its arena ranges: `linear.*` at lr, `rnn.*`, `lstm_init_*` and `transitions` at lr * lr_rate
    (the reference's two parameter groups, finetune_trainer.py:552-571), clip_grad_norm_(max_norm) from kbner_grad_sqnorm, then
    kbner_adamw_hf (HF AdamW: eps 1e-6, weight decay 0, bias correction) or kbner_sgd.  lr_scale multiplies both rates (the
    trainer's schedule)."""

    def __init__(self, head, name="AdamW", lr=5e-3, lr_rate=1.0, betas=(0.9, 0.999), eps=1e-6, max_norm=5.0):
        if name not in ("AdamW", "SGD"):
            raise NotImplementedError("optimizer %r: the stacked tagger trains with AdamW or SGD" % (name,))
        if head.arena is None:
            raise L_.KbnerError("StackOptimizer needs a trainable BiLSTMHead (enable_training())")
        self.head, self.name, self.lr, self.lr_rate, self.betas, self.eps, self.max_norm = head, name, lr, lr_rate, betas, eps, max_norm
        self.t = 0
        self.lr_scale = 1.0
        self.ws = torch.zeros(L_.load().kbner_sqnorm_ws_floats(), dtype=F32, device=head.device)
        self.norm_sq = torch.zeros(1, dtype=F32, device=head.device)
        self.reset()

    @property
    def char(self):
        """the head's character BiLSTM (CharBiLSTM) or None: its arena is one more range of the plain-learning-rate group"""
        return getattr(self.head, "char", None)

    def groups(self):
        """[(name, parameters, learning rate)]: what step() updates, in order"""
        h = self.head
        out = [("rnn+transitions", h.split, self.lr * self.lr_rate * self.lr_scale), ("linear", h.n - h.split, self.lr * self.lr_scale)]
        if self.char is not None:
            out.append(("char", self.char.n, self.lr * self.lr_scale))
        # rnn.*_l{k}, lstm_init_h and lstm_init_c: neither 'embedding' in the name nor linear.* (finetune_trainer.py:552-553)
        for blk in h.blocks_extra():
            out.append(("rnn layer %d" % blk.k if hasattr(blk, "k") else "lstm_init", blk.n, self.lr * self.lr_rate * self.lr_scale))
        return out

    def reset(self):
        """drop the moments (a new state was loaded into the head)"""
        h = self.head
        self.m = torch.zeros(h.n, dtype=F32, device=h.device) if self.name == "AdamW" else None
        self.v = torch.zeros(h.n, dtype=F32, device=h.device) if self.name == "AdamW" else None
        c = self.char
        self.cm = torch.zeros(c.n, dtype=F32, device=h.device) if (c is not None and self.name == "AdamW") else None
        self.cv = torch.zeros(c.n, dtype=F32, device=h.device) if (c is not None and self.name == "AdamW") else None
        # one pair of moments per parameter block beside the arena (upper layers, initial state)
        self.xm = [torch.zeros(b.n, dtype=F32, device=h.device) if self.name == "AdamW" else None for b in h.blocks_extra()]
        self.xv = [torch.zeros(b.n, dtype=F32, device=h.device) if self.name == "AdamW" else None for b in h.blocks_extra()]
        self.t = 0

    def step(self, grad_scale=1.0):
        """clip, update, zero the gradient, refresh the head's shadow views -> the squared gradient norm (device, before scaling)"""
        h = self.head
        with L_.stream_scope():
            ops.grad_sqnorm(h.g, self.ws, self.norm_sq)
            c = self.char
            if c is not None:      # ONE clip norm over head and character gradients (clip_grad_norm_(model.parameters()))
                ops.grad_sqnorm(c.g, self.ws, self.norm_sq, accumulate=True)
            extra = h.blocks_extra()
            for blk in extra:
                ops.grad_sqnorm(blk.g, self.ws, self.norm_sq, accumulate=True)
            self.t += 1
            b1, b2 = self.betas
            bc = (1.0 - b2 ** self.t) ** 0.5 / (1.0 - b1 ** self.t)
            for lo, hi, lr in ((0, h.split, self.lr * self.lr_rate * self.lr_scale), (h.split, h.n, self.lr * self.lr_scale)):
                nsh = h.n_shadow if lo == 0 else 0
                sh = h.shadow if nsh else None
                if self.name == "AdamW":
                    ops.adamw(h.arena[lo:hi], h.g[lo:hi], self.m[lo:hi], self.v[lo:hi], sh, nsh, lr * bc, 0.0, b1, b2, self.eps,
                              self.norm_sq, self.max_norm, grad_scale, True)
                else:
                    ops.sgd(h.arena[lo:hi], h.g[lo:hi], sh, nsh, lr, self.norm_sq, self.max_norm, grad_scale, True)
            if c is not None:
                lr = self.lr * self.lr_scale
                if self.name == "AdamW":
                    if self.cm is None or self.cm.numel() != c.n:
                        self.cm, self.cv = torch.zeros_like(c.g), torch.zeros_like(c.g)
                    ops.adamw(c.arena, c.g, self.cm, self.cv, None, 0, lr * bc, 0.0, b1, b2, self.eps, self.norm_sq, self.max_norm,
                              grad_scale, True)
                else:
                    ops.sgd(c.arena, c.g, None, 0, lr, self.norm_sq, self.max_norm, grad_scale, True)
            for blk, m, v in zip(extra, self.xm, self.xv):
                lr = self.lr * self.lr_rate * self.lr_scale
                if self.name == "AdamW":
                    ops.adamw(blk.arena, blk.g, m, v, blk.shadow, blk.n_shadow, lr * bc, 0.0, b1, b2, self.eps, self.norm_sq,
                              self.max_norm, grad_scale, True)
                else:
                    ops.sgd(blk.arena, blk.g, blk.shadow, blk.n_shadow, lr, self.norm_sq, self.max_norm, grad_scale, True)
            h._refresh()
        return self.norm_sq


class CharLM:
    """FlairEmbeddings' character language model at inference: embedding(chars) -> 1-layer LSTM -> hidden state at chosen steps
    (flair/models/language_model.py:71-138; projection `nout` unsupported: the shipped big LMs have none).
    The input half is a lookup table: table[ch] = Wih emb[ch] + bih + bhh, one row per dictionary character, built once."""

    def __init__(self, state_dict, hidden, device):
        self.device = torch.device(device)
        self.grp = LSTMGroup([state_dict["rnn.weight_hh_l0"]], hidden, device)
        emb = torch.as_tensor(state_dict["encoder.weight"], dtype=F32)
        wih = torch.as_tensor(state_dict["rnn.weight_ih_l0"], dtype=F32)
        b = torch.as_tensor(state_dict["rnn.bias_ih_l0"], dtype=F32) + torch.as_tensor(state_dict["rnn.bias_hh_l0"], dtype=F32)
        table = emb @ wih.t() + b                                   # [chars, 4H] fp32, host, once per model load
        self.table = self.grp.pad_gates(table.t().contiguous()).t().contiguous().to(BF16).to(self.device).contiguous()
        self.H, self.Hp = self.grp.H, self.grp.Hp

    def run(self, char_ids, out_rows, X, col):
        """char_ids int [steps, B] (every sequence padded to the same length, as the reference pads with blanks);
        out_rows int [steps, B]: row of X that receives h after that step, -1 = not needed.  Writes X[row, col:col+Hp]."""
        steps, B = char_ids.shape
        gxi = torch.from_numpy(np.ascontiguousarray(char_ids, np.int32)[:, None, :]).to(self.device)
        outi = torch.from_numpy(np.ascontiguousarray(out_rows, np.int32)[:, None, :]).to(self.device)
        with L_.stream_scope():
            self.grp.run(self.table, gxi, outi, X, 0, B, col=col)


class CharLMGroup:
    """All character LMs of one hidden width run as ONE recurrence (LSTMGroup with ndir = number of models): one launch per
    character step for all of them instead of one per model -- the step of a 2048-unit LM is a 33.5 MB stream of Whh, and a
    single model's launch cannot keep enough of it in flight.  Tables are stacked along the columns ([chars, ndir * 4Hp], the
    shorter dictionaries zero-padded), every model keeps its own character ids (forward / backward LMs read the text in opposite
    orders) and its own column block of X."""

    def __init__(self, lms):
        lms = list(lms)
        if not lms or len({lm.Hp for lm in lms}) != 1:
            raise ValueError("a CharLMGroup takes character LMs of one (padded) hidden width")
        self.lms = lms
        self.device = lms[0].device
        self.H, self.Hp = lms[0].H, lms[0].Hp
        self.grp = LSTMGroup.__new__(LSTMGroup)
        self.grp.H, self.grp.Hp, self.grp.ndir, self.grp.device = self.H, self.Hp, len(lms), self.device
        self.grp.whh = torch.cat([lm.grp.whh for lm in lms], 0).contiguous()
        rows = max(lm.table.shape[0] for lm in lms)
        table = torch.zeros((rows, len(lms) * 4 * self.Hp), dtype=BF16, device=self.device)
        for d, lm in enumerate(lms):
            table[:lm.table.shape[0], d * 4 * self.Hp:(d + 1) * 4 * self.Hp] = lm.table
        self.table = table

    def run(self, char_ids, out_rows, X, cols):
        """char_ids / out_rows: one int [steps, B] array per model (same steps and B); cols: its first column in X"""
        gxi = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(c, np.int32) for c in char_ids], 1))).to(self.device)
        outi = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(r, np.int32) for r in out_rows], 1))).to(self.device)
        B = gxi.shape[2]
        with L_.stream_scope():
            self.grp.run(self.table, gxi, outi, X, 0, B, out_cols=list(cols))
