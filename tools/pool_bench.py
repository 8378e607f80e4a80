"""What sub-token pooling costs the producer stage of one stack batch (kbner_pool_rows_layers): one frozen
XLM-R-large-sized encoder (hidden 1024, 24 layers) reading 32 sentences of 512 sub-tokens, then the token features of n = 64 word
positions (sentence lengths 32-64, drawn as tools/stack_store_bench.py draws them) written into a 4096-column block of the stack's
input matrix X (row stride 8192, block at column 2048):

    pool     encoder_forward + ONE ops.pool_rows_layers: pooling_operation 'mean' over layers -1,-2,-3,-4 (host checks of the two
             tables and their upload included -- that is what a batch pays)
    gather   encoder_forward + FOUR kbner_gather_rows_ld: 'first' over the same four layers with one launch per layer (the scheme the
             stack had for BertEmbeddings; the index is on the device already)

Method: the two stages alternate inside every round; a round times `--reps` stages of each kind with the host clock around work that
ends in a device synchronise; `--warmup` rounds first (the third forward-only pass over a shape is captured into a graph), then the
median over `--rounds` rounds.  Second table: the launches alone, device events around `--kreps` repetitions, alternating, medians --
`pool_rows_layers` through kbner.ops (tables checked and uploaded per call), `pool_kernel` the library call with the tables already on
the device, `gather_ld_x4` the four launches.  Before anything is timed 'first' over the four layers through the new kernel is
compared bit for bit with the four gathers.  Prints one JSON line (and writes it to --out).  A record, no threshold.

    python tools/pool_bench.py [--rounds 7 --warmup 3 --reps 10 --out profiles/pool_bench.json]
"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("B", 32), ("n", 64), ("rounds", 7), ("warmup", 3), ("reps", 10), ("kreps", 200)):
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kbner import batch as kb
    from kbner import engine, ops
    from kbner import lib as L
    dev = "cuda"
    B, n, S, T = a.B, a.n, 512, 21
    cfg = engine.EncoderConfig.large(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    H, LAYERS = cfg.hidden_size, (-1, -2, -3, -4)
    enc = engine.Tagger(cfg, T, T - 2, T - 1, device=dev, inference=True)
    enc.init_random(seed=kb.SEED)
    hb = kb.synthetic_batch(B, S, vocab=cfg.vocab_size, T=29, x_idx=9, start=27, stop=28, n_real=n, seed=kb.SEED + 9)
    eb = kb.to_device(hb, dev)
    first = hb["first_idx"]
    assert first.shape[1] > n, "the synthetic batch has %d word tokens per sentence, n + 1 = %d are needed" % (first.shape[1], n + 1)
    rng = np.random.default_rng(0)
    lengths = rng.integers(n // 2, n + 1, size=B)
    lengths[0] = n
    # the tables: word t of sentence b owns the sub-tokens from its first piece up to the next word's
    span_ptr, rows, idx = [0], [], np.full((B, n), -1, np.int64)
    for b in range(B):
        for t in range(n):
            if t < lengths[b]:
                rows += [b * S + p for p in range(int(first[b, t]), int(first[b, t + 1]))]
                idx[b, t] = b * S + first[b, t]
            span_ptr.append(len(rows))
    span_ptr, rows = np.asarray(span_ptr, np.int64), np.asarray(rows, np.int64)
    idx_d = torch.from_numpy(idx.reshape(-1).astype(np.int32)).to(dev)
    R, ld, col, W = B * n, 8192, 2048, len(LAYERS) * H
    X = torch.zeros((R, ld), dtype=torch.bfloat16, device=dev)
    Y = torch.zeros((R, ld), dtype=torch.bfloat16, device=dev)

    def forward():
        enc.encoder_forward(eb["ids"], eb["pos_ids"], eb["maskbias"], B, S, need_grad=False)
        states = enc.acts(B, S).x
        return [states[li] for li in LAYERS]

    def pool(srcs, op="mean", out=X):
        ops.pool_rows_layers(srcs, span_ptr, rows, out, col, op)

    def gather(srcs, out=X):
        for j, s_ in enumerate(srcs):
            ops.gather_rows_into(s_, idx_d, out, col + j * H, H)

    srcs = forward()
    pool(srcs, "first", X)
    gather(srcs, Y)
    torch.cuda.synchronize()
    assert torch.equal(X.view(torch.int16), Y.view(torch.int16)), "'first' through the new kernel differs from the four gathers"

    stages = {"pool": lambda: pool(forward()), "gather": lambda: gather(forward())}
    times = {k: [] for k in stages}
    for r in range(a.warmup + a.rounds):
        for name, fn in stages.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append((time.perf_counter() - t0) / a.reps * 1e3)
    # ---- the launches alone
    sp_d, sr_d = torch.from_numpy(span_ptr.astype(np.int32)).to(dev), torch.from_numpy(rows.astype(np.int32)).to(dev)
    ptrs = (ctypes.c_void_p * len(srcs))(*[s_.data_ptr() for s_ in srcs])

    def pool_kernel():
        L.call("kbner_pool_rows_layers", ptrs, len(srcs), 0, ops.POOL_OPS["mean"], L.ptr(sp_d), L.ptr(sr_d),
               ctypes.c_void_p(X.data_ptr() + 2 * col), ld, R, H, L.stream_ptr())

    launches = {"pool_rows_layers": lambda: pool(srcs), "pool_kernel": pool_kernel, "gather_ld_x4": lambda: gather(srcs)}
    us = {k: [] for k in launches}
    for r in range(2 + 5):
        for name, fn in launches.items():
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.kreps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                us[name].append(e0.elapsed_time(e1) / a.kreps * 1e3)
    m = np.diff(span_ptr)
    out = {"shape": {"B": B, "S": S, "n": n, "hidden": H, "encoder_layers": cfg.num_hidden_layers, "layers": list(LAYERS), "rows": R,
                     "block": [col, col + W], "ld": ld, "word_tokens": int((m > 0).sum()), "sub_tokens_pooled": int(rows.size),
                     "longest_span": int(m.max())},
           "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "producer_stage_ms": {k: round(float(np.median(v)), 3) for k, v in times.items()},
           "producer_stage_all_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
           "launch_us": {k: round(float(np.median(v)), 2) for k, v in us.items()},
           "launch_all_us": {k: [round(t, 2) for t in v] for k, v in us.items()},
           "bytes_moved": {"pool_mean_x4": int(2 * H * (len(LAYERS) * rows.size + len(LAYERS) * R)), "gather_ld_x4": int(2 * 2 * W * R)}}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
