#!/usr/bin/env python
"""One optimizer step of the stacked tagger's head at the ACE shape (32 sentences, hidden_size 800), with and without the character
BiLSTM (FastCharacterEmbeddings, 25 / 25), in alternating rounds of one process; and the two character kernels on their own.

    python tools/char_bench.py [--rounds 7] [--steps 20] [--tokens 24]

The head is the same in both arms (input blocks 1024 + 50, so the input GEMM and the weight-gradient GEMMs are the same launches): an arm
with the embedding adds kbner_char_lstm_fwd, the 128-column window GEMM of dXt, kbner_char_lstm_bwd, and the character range of the
clip norm and the optimizer.  Times are device events around `steps` back-to-back steps, per round; printed: median and minimum over the
rounds, one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kb-ner_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sentences", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--hidden", type=int, default=800)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("char_bench.py measures on the GPU; there is none here")
    from kbner import batch as kb
    from kbner import ops
    from kbner import stack as K
    rng = np.random.default_rng(0)
    B, n, H, T, D0 = args.sentences, args.tokens, args.hidden, 17, 1024
    D = D0 + 50
    k = 1.0 / np.sqrt(H)
    rnn = {}
    for s in ("", "_reverse"):
        rnn["weight_ih_l0" + s] = torch.from_numpy(rng.uniform(-k, k, (4 * H, D)).astype(np.float32))
        rnn["weight_hh_l0" + s] = torch.from_numpy(rng.uniform(-k, k, (4 * H, H)).astype(np.float32))
        rnn["bias_ih_l0" + s] = torch.from_numpy(rng.uniform(-k, k, 4 * H).astype(np.float32))
        rnn["bias_hh_l0" + s] = torch.from_numpy(rng.uniform(-k, k, 4 * H).astype(np.float32))
    tr = rng.standard_normal((T, T)).astype(np.float32)
    tr[T - 2, :] = -1e12
    tr[:, T - 1] = -1e12
    head = K.BiLSTMHead(rnn, rng.standard_normal((T, 2 * H)).astype(np.float32) * 0.05, np.zeros(T, np.float32), [D0, 50], H, "cuda",
                        transitions=tr, trainable=True)
    head.dropout, head.locked_dropout, head.word_dropout = 0.0, 0.5, 0.05          # the ACE YAMLs' head dropouts
    head.train(True)
    lengths = rng.integers(n // 2, n + 1, size=B)
    lengths[0] = n
    X = head.new_input(B, n)
    for b in range(B):
        X[b * n:b * n + lengths[b], :D0] = torch.randn((int(lengths[b]), D0), device="cuda").to(torch.bfloat16)
    tags = rng.integers(0, T - 2, (B, n)).astype(np.int64)
    db = kb.to_device(kb.assemble(np.zeros((B, 1), np.int64), np.ones((B, 1), np.int64), np.full((B, n), -1, np.int64), tags,
                                  lengths.astype(np.int64), None), "cuda")
    cemb = torch.nn.Embedding(90, 25)
    clstm = torch.nn.LSTM(25, 25, num_layers=1, bidirectional=True)
    state = {"char_embedding.weight": cemb.weight.detach()}
    state.update({"char_layer." + kk: v.detach() for kk, v in clstm.named_parameters()})
    net = K.CharBiLSTM(state, "cuda")
    rows = np.concatenate([b * n + np.arange(lengths[b]) for b in range(B)]).astype(np.int32)
    W = rows.size
    lens = np.clip(rng.poisson(5.0, W), 1, 16).astype(np.int32)
    chars = rng.integers(1, 90, (W, int(lens.max()))).astype(np.int32)
    for w in range(W):
        chars[w, lens[w]:] = 0
    opt = K.StackOptimizer(head, name="SGD", lr=0.01)

    def step(with_char):
        head.char = net if with_char else None
        char = K.CharStep(net, chars, lens, rows, head.cols[1]) if with_char else None
        if char is None:
            head.loss_backward(X, lengths, B, n, db, T - 2, T - 1)
        else:
            head.loss_backward(X, lengths, B, n, db, T - 2, T - 1, char=char)
        opt.step()

    for arm in (False, True, False, True):
        step(arm)
    torch.cuda.synchronize()
    res = {False: [], True: []}
    for _ in range(args.rounds):
        for arm in (False, True):
            res[arm].append(timed(lambda: step(arm), args.steps))
    # the two kernels alone, on the same tables
    Mp = head.rows(B, n)
    Xt = torch.zeros((Mp, head.Dq), dtype=torch.bfloat16, device="cuda")
    tab = ops.CharTables(chars, lens, rows, net.V, Mp, "cuda")
    ws = ops.char_lstm_ws(tab, net.Hc, "cuda")
    par = [net.param(f) for f in K.CharBiLSTM._FIELDS]
    grads = [net.grad(f) for f in K.CharBiLSTM._FIELDS]
    site = ((5, ops.drop_thresh(0.0)), (6, ops.drop_thresh(0.5)))
    dwin = torch.randn((Mp, 128), device="cuda").to(torch.bfloat16)
    fwd = lambda: ops.char_lstm_fwd(*par, tab, Xt, head.cols[1], n, site[0], site[1], ws=ws)                       # noqa: E731
    bwd = lambda: ops.char_lstm_bwd(dwin, 0, par[0], par[1], par[2], tab, ws, *grads, n, site[0], site[1], key_col=head.cols[1])   # noqa: E731
    kt = {"fwd": [], "bwd": []}
    for f in (fwd, bwd, fwd, bwd):
        f()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        kt["fwd"].append(timed(fwd, 50))
        kt["bwd"].append(timed(bwd, 50))
    out = {"sentences": B, "tokens": n, "words": int(W), "chars": int(lens.sum()), "hidden": H, "rounds": args.rounds, "steps": args.steps}
    for name, v in (("step_without_us", res[False]), ("step_with_us", res[True]), ("char_fwd_us", kt["fwd"]), ("char_bwd_us", kt["bwd"])):
        out[name + "_median"], out[name + "_min"] = round(float(np.median(v)), 1), round(float(np.min(v)), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
