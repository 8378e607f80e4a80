"""Times the layer-selection kernels (csrc/rows.hip) -- the figures of DESIGN.md section 3, "Encoder layer selection".

  python tools/layers_bench.py [--out FILE.json] [--steps]

Kernels, at R = 131 072 rows, H = 1024, k = 4 (a 256-sentence step's kept tokens, layers='-1,-2,-3,-4'):
  gather_rows_layers, concatenation and mean, without and with both dropout sites, against k launches of kbner_gather_rows_ld into
  the same [R, k * H] matrix (how the block matrix could be built before this kernel existed);
  scatter_add_rows_ld of one H-wide block of a [R, 4 H] gradient; head_bwd_dx at W = 4096, T = 29.
Every configuration is timed in `--rounds` alternating rounds of `--reps` back-to-back launches between two device events (one round
of each configuration, then the next round) after a warm-up of all of them; the figure is the median round with the spread, in us
and in TB/s of the bytes the operation has to move.
--steps: the optimizer step of the engine (forward_loss with backward + FusedAdamW.step) with layers (-1,-2,-3,-4) against (-1,) on
XLM-R-large dimensions, at 256 x 1 sentences of 128 sub-tokens and at 4 sentences, in alternating rounds in one process.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kb-ner_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda"
BF16 = torch.bfloat16


def time_rounds(configs, rounds, reps):
    """configs: {name: zero-argument launcher} -> {name: [us per launch, one entry per round]}"""
    for f in configs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in configs}
    for _ in range(rounds):
        for name, f in configs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1000.0 / reps)
    return out


def kernels(args):
    from kbner import ops
    R, H, k, T, n = args.rows, 1024, 4, 29, 512
    g = torch.Generator(device=DEV).manual_seed(1)
    srcs = [torch.randn((R, H), generator=g, device=DEV).to(BF16) for _ in range(k)]
    idx = torch.randperm(R, generator=g, device=DEV).to(torch.int32)
    cat = torch.empty((R, k * H), dtype=BF16, device=DEV)
    avg = torch.empty((R, H), dtype=BF16, device=DEV)
    dst = torch.zeros((R, H), dtype=BF16, device=DEV)
    de = torch.randn((R, T), generator=g, device=DEV)
    w = torch.randn((T, k * H), generator=g, device=DEV) * 0.02
    dw, db = torch.zeros_like(w), torch.zeros(T, device=DEV)
    se, sl = (11, ops.drop_thresh(0.1)), (12, ops.drop_thresh(0.5))

    def by_ld():
        for j in range(k):
            ops.gather_rows_into(srcs[j], idx, cat, j * H, H)

    from kbner import lib as L
    st = L.stream_ptr

    def dx_only():
        L.call("kbner_head_bwd_dx", L.ptr(de), L.ptr(w), L.ptr(cat), R, k * H, T, st())

    configs = {
        "gather_rows_ld x4 (concat)": by_ld,
        "gather_rows_layers concat": lambda: ops.gather_rows_layers(srcs, idx, n, out=cat),
        "gather_rows_layers concat +drop": lambda: ops.gather_rows_layers(srcs, idx, n, drop_e=se, drop_l=sl, out=cat),
        "gather_rows_layers mean": lambda: ops.gather_rows_layers(srcs, idx, n, mean=True, out=avg),
        "gather_rows_layers mean +drop": lambda: ops.gather_rows_layers(srcs, idx, n, mean=True, drop_e=se, drop_l=sl, out=avg),
        "scatter_add_rows_ld": lambda: ops.scatter_add_rows_ld(cat, H, idx, dst, n),
        "scatter_add_rows_ld +drop": lambda: ops.scatter_add_rows_ld(cat, H, idx, dst, n, 1.0, se, sl),
        "head_bwd_dx W=4096 T=29": dx_only,
    }
    row = 2 * H
    nbytes = {"gather_rows_ld x4 (concat)": 2 * k * R * row, "gather_rows_layers concat": 2 * k * R * row,
              "gather_rows_layers concat +drop": 2 * k * R * row, "gather_rows_layers mean": (k + 1) * R * row,
              "gather_rows_layers mean +drop": (k + 1) * R * row, "scatter_add_rows_ld": 3 * R * row, "scatter_add_rows_ld +drop": 3 * R * row,
              "head_bwd_dx W=4096 T=29": R * (4 * T + 2 * k * H)}
    t = time_rounds(configs, args.rounds, args.reps)
    res = {}
    for name, us in t.items():
        med = statistics.median(us)
        res[name] = {"us": round(med, 1), "min": round(min(us), 1), "max": round(max(us), 1), "TBps": round(nbytes[name] / med * 1e-6, 2)}
        print("%-34s %9.1f us  (%.1f .. %.1f)  %.2f TB/s" % (name, med, min(us), max(us), nbytes[name] / med * 1e-6))
    return res


def steps(args):
    from kbner import batch as kb
    from kbner import engine
    res = {}
    for label, B in (("256x1", 256), ("4x1", 4)):
        cfg = engine.EncoderConfig.large()
        T, start, stop = 29, 27, 28
        b = kb.synthetic_batch(B, 128, vocab=cfg.vocab_size, T=T, x_idx=9, start=start, stop=stop, n_real=24, seed=3)
        bd = kb.to_device(b, DEV)
        runs = {}
        for name, layers in (("-1", (-1,)), ("-1,-2,-3,-4", (-1, -2, -3, -4))):
            tg = engine.Tagger(cfg, T, start, stop, device=DEV, layers=layers)
            tg.init_random(seed=1)
            opt = engine.FusedAdamW(tg.arena, lr=5e-6, t_total=1000)

            def step(tg=tg, opt=opt):
                tg.forward_loss(bd, backward=True)
                opt.step()
            runs[name] = step
        t = time_rounds(runs, args.rounds, max(1, args.reps // 4))
        res[label] = {k: {"ms": round(statistics.median(v) / 1000.0, 3), "min": round(min(v) / 1000.0, 3), "max": round(max(v) / 1000.0, 3)}
                      for k, v in t.items()}
        print(label, res[label])
        del runs
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"kernels": kernels(args)}
    if args.steps:
        res["steps"] = steps(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
