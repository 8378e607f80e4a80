"""What the feature store saves a training run of the stacked tagger (kbner.stack.FeatureStore, embeddings_storage_mode): the wall time
of one epoch AFTER the first over a synthetic corpus, with the store off ("none": every batch runs its frozen feature producers again),
in pinned host memory ("cpu") and in device memory ("gpu").

Shape: the ACE YAML's head (B 32, n 64 with lengths 32-64, H 1000, D 5120, T 21) behind random-weight producers of the real sizes that add
up to D: three XLM-R-large-sized frozen encoders reading 512 sub-tokens per sentence and one 2048-unit character LM (~7 characters per
token); word_dropout 0.05 and locked_dropout 0.5 (flair's defaults, which the YAML leaves alone), dropout 0.  A batch is: features
(computed, or one kbner_gather_rows_blocks_drop from the store) -> BiLSTMHead.loss_backward -> StackOptimizer.step.  The corpus is
`--batches` batches of distinct sentence objects (all batches share one set of sub-token ids: the producers' time does not depend on them).

Method: one fill pass (the first epoch: computes and stores every batch in both stores), then alternating rounds in one process -- each
round runs one epoch per mode, host clock around the epoch ending in a device synchronise -- `--warmup` rounds first, the median of
`--rounds` timed ones.  Second table: the new kernel alone against the launches it replaces in loss_backward (the zero-fill of Xd,
kbner_gather_rows_drop with an identity index, and -- where Dq != Dp -- the zero-fill of Xt and the slice copy), device events around
`--kreps` repetitions.  Prints one JSON line (and writes it to --out).  No threshold: the numbers go into DESIGN.md section 3 as measured.

    python tools/stack_store_bench.py [--batches 64 --rounds 5 --warmup 2 --out profiles/stack_store_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kb-ner_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


class Sent:
    """a sentence as the store sees it: a length and an identity"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def kernel_table(ops, B, n, widths, reps):
    """the store read against the first stage of loss_backward it replaces, both dropout sites and WordDropout on -> rows of microseconds"""
    dev = "cuda"
    rows = []
    R, Mp = B * n, (B * n + 127) // 128 * 128
    rng = np.random.default_rng(1)
    word = rng.random(n) < 0.05
    de, dl = (12345, ops.drop_thresh(0.1)), (54321, ops.drop_thresh(0.5))
    for Dp in widths:
        Dq = (Dp + 127) // 128 * 128
        X = torch.randn((Mp, Dp), device=dev).to(torch.bfloat16)
        ident = torch.arange(R, dtype=torch.int32, device=dev)
        idx_old = torch.where(torch.from_numpy(np.tile(word, B)).to(dev), torch.full_like(ident, -1), ident)
        idx_new = idx_old.clone()
        cols = torch.tensor([0, Dp], dtype=torch.int32, device=dev)
        ops.check_block_cols([0, Dp], Dp)
        on = torch.ones(1, dtype=torch.uint8, device=dev)

        def old():
            Xd = torch.zeros((Mp, Dp), dtype=torch.bfloat16, device=dev)
            ops.gather_rows_drop(X, idx_old, n, de, dl, out=Xd)
            if Dq != Dp:
                Xt = torch.zeros((Mp, Dq), dtype=torch.bfloat16, device=dev)
                Xt[:, :Dp] = Xd
                return Xt
            return Xd

        def new():
            return ops.gather_rows_blocks_drop(X, idx_new, cols, on, n, R_out=Mp, ld_out=Dq, drop_e=de, drop_l=dl)
        assert torch.equal(old().view(torch.int16), new().view(torch.int16))
        us = {}
        for name, fn in (("replaced_launches", old), ("gather_rows_blocks_drop", new)) * 2:
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.setdefault(name, []).append(e0.elapsed_time(e1) / reps * 1e3)
        rows.append({"rows": Mp, "Dp": Dp, "Dq": Dq, "launches_replaced": 4 if Dq != Dp else 2,
                     "us": {k_: round(min(v), 2) for k_, v in us.items()},
                     "bytes_moved_new": 2 * (R * Dp + Mp * Dq)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("B", 32), ("n", 64), ("H", 1000), ("T", 21), ("batches", 64), ("rounds", 5), ("warmup", 2), ("encoders", 3), ("lm_hidden", 2048),
                 ("kreps", 50)):
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kbner import batch as kb
    from kbner import engine, ops
    from kbner import stack as K
    dev = "cuda"
    B, n, H, T = a.B, a.n, a.H, a.T
    start, stop = T - 2, T - 1
    cfg = engine.EncoderConfig.large(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    blocks = [a.lm_hidden] + [cfg.hidden_size] * a.encoders      # sorted embedding names: FlairEmbeddings before TransformerWordEmbeddings
    D = sum(blocks)
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(3)
    # ---- the producers
    encs = []
    for i in range(a.encoders):
        e = engine.Tagger(cfg, T, start, stop, device=dev, inference=True)
        e.init_random(seed=kb.SEED + i)
        encs.append(e)
    kk = 1.0 / a.lm_hidden ** 0.5
    lm = K.CharLMGroup([K.CharLM({"encoder.weight": torch.rand(300, 100, generator=g) * 0.2 - 0.1,
                                  "rnn.weight_ih_l0": (torch.rand(4 * a.lm_hidden, 100, generator=g) * 2 - 1) * kk,
                                  "rnn.weight_hh_l0": (torch.rand(4 * a.lm_hidden, a.lm_hidden, generator=g) * 2 - 1) * kk,
                                  "rnn.bias_ih_l0": torch.zeros(4 * a.lm_hidden), "rnn.bias_hh_l0": torch.zeros(4 * a.lm_hidden)},
                                 a.lm_hidden, dev)])
    hb = kb.synthetic_batch(B, 512, vocab=cfg.vocab_size, T=29, x_idx=9, start=27, stop=28, n_real=n, seed=kb.SEED + 9)
    eb = kb.to_device(hb, dev)
    n_tok = hb["first_idx"].shape[1]
    assert n_tok >= n, "the synthetic 512-sub-token batch has %d word tokens per sentence, fewer than n = %d" % (n_tok, n)
    first_rows = np.ascontiguousarray(hb["row_idx"].reshape(B, n_tok)[:, :n])
    # ---- the head
    k = 1.0 / np.sqrt(H)
    rnn = {}
    for s in ("", "_reverse"):
        rnn["weight_ih_l0" + s] = torch.from_numpy(rng.uniform(-k, k, (4 * H, D)).astype(np.float32))
        rnn["weight_hh_l0" + s] = torch.from_numpy(rng.uniform(-k, k, (4 * H, H)).astype(np.float32))
        rnn["bias_ih_l0" + s] = torch.from_numpy(rng.uniform(-k, k, 4 * H).astype(np.float32))
        rnn["bias_hh_l0" + s] = torch.from_numpy(rng.uniform(-k, k, 4 * H).astype(np.float32))
    tr = rng.standard_normal((T, T)).astype(np.float32)
    tr[start, :] = -1e4
    tr[:, stop] = -1e4
    head = K.BiLSTMHead(rnn, (rng.uniform(-1, 1, (T, 2 * H)) / np.sqrt(2 * H)).astype(np.float32), np.zeros(T, np.float32), blocks, H, dev,
                        transitions=tr, trainable=True)
    head.word_dropout, head.locked_dropout, head.dropout = 0.05, 0.5, 0.0
    head.train(True)
    opt = K.StackOptimizer(head, name="AdamW", lr=1e-4, lr_rate=1.0)
    # ---- the corpus
    corpus = []
    for bi in range(a.batches):
        lengths = rng.integers(n // 2, n + 1, size=B)
        lengths[0] = n
        sents = [Sent(int(x)) for x in lengths]
        tags = rng.integers(0, T - 2, (B, n))
        idx = np.where(np.arange(n)[None, :] < lengths[:, None], first_rows, -1).reshape(-1).astype(np.int32)
        steps = 2 + n * 7
        out_rows = np.full((steps, B), -1, np.int32)
        for b in range(B):
            t = np.arange(int(lengths[b]))
            out_rows[(t + 1) * 7, b] = b * n + t
        db = kb.to_device(kb.assemble(np.zeros((B, 1), np.int64), np.ones((B, 1), np.int64), np.full((B, n), -1, np.int64), tags.astype(np.int64),
                                      lengths.astype(np.int64), None), dev)
        corpus.append(dict(sents=sents, lengths=lengths.astype(np.int64), idx=torch.from_numpy(idx).to(dev), db=db,
                           char_ids=rng.integers(1, 290, size=(steps, B)).astype(np.int32), out_rows=out_rows))
    block_col = list(head.cols) + [head.Dp]
    stores = {"none": None, "cpu": K.FeatureStore("cpu", head.Dp, block_col, dev), "gpu": K.FeatureStore("gpu", head.Dp, block_col, dev)}

    def produce(c):
        X = head.new_input(B, n)
        lm.run([c["char_ids"]], [c["out_rows"]], X, [head.cols[0]])
        for i, e in enumerate(encs):
            hid = e.encoder_forward(eb["ids"], eb["pos_ids"], eb["maskbias"], B, 512, need_grad=False)
            ops.gather_rows_into(hid, c["idx"], X, head.cols[1 + i], cfg.hidden_size)
        return X

    def epoch(mode):
        store = stores[mode]
        for c in corpus:
            src = store.source(c["sents"], n) if store is not None else None
            X = None
            if src is None:
                X = produce(c)
                if store is not None:
                    store.add(c["sents"], X, c["lengths"], n)
            head.loss_backward(X, c["lengths"], B, n, c["db"], start, stop, source=src)
            opt.step()

    def timed_epoch(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        epoch(mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    fill = {m: timed_epoch(m) for m in ("cpu", "gpu")}           # the first epoch of a run with a store: compute + store
    for m in ("cpu", "gpu"):
        assert len(stores[m]) == a.batches * B and not stores[m].full, (m, len(stores[m]))
    times = {m: [] for m in stores}
    for r in range(a.warmup + a.rounds):
        for m in stores:
            t = timed_epoch(m)
            if r >= a.warmup:
                times[m].append(t)
    for m in ("cpu", "gpu"):
        assert stores[m].misses == a.batches, "an epoch after the first recomputed a batch"
    med = {m: float(np.median(v)) for m, v in times.items()}
    out = {"shape": {"B": B, "n": n, "H": H, "D": D, "T": T, "blocks": blocks, "batches": a.batches,
                     "producers": "%d XLM-R-large-sized encoders at 512 sub-tokens + 1 character LM of %d units" % (a.encoders, a.lm_hidden)},
           "rounds": a.rounds, "warmup": a.warmup,
           "second_epoch_ms": {m: round(v, 1) for m, v in med.items()},
           "per_batch_ms": {m: round(v / a.batches, 3) for m, v in med.items()},
           "speedup_vs_none": {m: round(med["none"] / med[m], 2) for m in ("cpu", "gpu")},
           "all_ms": {m: [round(t, 1) for t in v] for m, v in times.items()},
           "first_epoch_with_store_ms": {m: round(v, 1) for m, v in fill.items()},
           "store": {"rows": stores["gpu"].rows, "bytes": stores["gpu"].nbytes},
           "kernel": kernel_table(ops, B, n, [head.Dp, head.Dp + 64], a.kreps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
