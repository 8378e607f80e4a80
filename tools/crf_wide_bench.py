"""Times the wide CRF entry points (csrc/crf_wide.hip) next to the single-wave ones (csrc/crf.hip) -- the figures of DESIGN.md
section 3, "Tag sets of 65 to 192 tags".

  python tools/crf_wide_bench.py [--out FILE.json]

Shapes: (B, n, T) = (32, 128, 137) wide, (32, 128, 64) wide and narrow on the same device buffers.  Every (kernel, family, shape)
is timed in `--rounds` alternating rounds of `--reps` back-to-back launches between two device events (a round of each
configuration, then the next round), after a warm-up of every configuration; the figure is the median round, with the spread.
Also: the CRF part (nll_fwd + nll_bwd) of a 4-sentence training step at T = 137 on the tiny model's compacted shape, and that
whole step (forward_loss with backward + FusedAdamW.step) on the tiny model, for the share it takes.
"""
import argparse
import ctypes
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


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def make(B, n, T, seed):
    rng = np.random.default_rng(seed)
    start, stop = T - 2, T - 1
    trans = rng.standard_normal((T, T)).astype(np.float32)
    trans[start, :] = -1e12
    trans[:, stop] = -1e12
    emit = (rng.standard_normal((B, n, T)) * 2).astype(np.float32)
    lens = rng.integers(n // 2, n + 1, size=B).astype(np.int32)
    lens[0] = n
    tags = rng.integers(0, T - 2, size=(B, n)).astype(np.int32)
    d = lambda a: torch.from_numpy(a).to(DEV)
    return {"B": B, "n": n, "T": T, "start": start, "stop": stop, "emit": d(emit), "trans": d(trans), "lens": d(lens), "tags": d(tags),
            "steps": int(lens.sum()), "max_len": int(lens.max()),
            "otags": torch.empty((B, n), dtype=torch.int32, device=DEV), "conf": torch.empty((B, n), device=DEV),
            "logz": torch.empty(B, device=DEV), "gold": torch.empty(B, device=DEV), "alpha": torch.empty((B, n + 1, T), device=DEV),
            "demit": torch.empty((B, n, T), device=DEV), "dtrans": torch.zeros((T, T), device=DEV),
            "dloss": torch.full((B,), 1.0 / B, device=DEV), "marg": torch.empty((B, n, T), device=DEV)}


def calls(lib, x, wide):
    """name -> zero-argument launcher of the family's entry point on the buffers of x"""
    pre = "kbner_crf_wide_" if wide else "kbner_crf_"
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, n, T, s, e = x["B"], x["n"], x["T"], x["start"], x["stop"]
    f = lambda name: getattr(lib, pre + name)
    if wide:
        x["ws"] = torch.empty(max(16, int(lib.kbner_crf_wide_viterbi_ws_bytes(B, n, T))), dtype=torch.uint8, device=DEV)
        vit = lambda: f("viterbi")(P(x["emit"]), P(x["trans"]), P(x["lens"]), B, n, T, s, e, P(x["otags"]), P(x["conf"]), None, P(x["ws"]), st)
    else:
        vit = lambda: f("viterbi")(P(x["emit"]), P(x["trans"]), P(x["lens"]), B, n, T, s, e, P(x["otags"]), P(x["conf"]), None, st)
    return {
        "viterbi": vit,
        "nll_fwd": lambda: f("nll_fwd")(P(x["emit"]), P(x["trans"]), P(x["tags"]), P(x["lens"]), B, n, T, s, e, P(x["logz"]), P(x["gold"]),
                                        P(x["alpha"]), st),
        "nll_bwd": lambda: f("nll_bwd")(P(x["emit"]), P(x["trans"]), P(x["tags"]), P(x["lens"]), P(x["alpha"]), P(x["logz"]), P(x["dloss"]),
                                        B, n, T, s, e, P(x["demit"]), P(x["dtrans"]), st),
        "posterior": lambda: f("posterior")(P(x["emit"]), P(x["trans"]), P(x["lens"]), P(x["alpha"]), P(x["logz"]), B, n, T, s, e,
                                            P(x["marg"]), st),
    }


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        rc = fn()
        assert rc == 0, rc
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps      # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from kbner import lib as L
    lib = L.load()
    x137, x64 = make(32, 128, 137, 1), make(32, 128, 64, 2)
    x4 = make(4, 24, 137, 3)
    configs = {}
    for name, fn in calls(lib, x137, True).items():
        configs[(name, "wide", "32x128x137")] = (fn, x137)
    for name, fn in calls(lib, x64, True).items():
        configs[(name, "wide", "32x128x64")] = (fn, x64)
    for name, fn in calls(lib, x64, False).items():
        configs[(name, "narrow", "32x128x64")] = (fn, x64)
    for name, fn in calls(lib, x4, True).items():
        if name in ("nll_fwd", "nll_bwd"):
            configs[(name, "wide", "4x24x137")] = (fn, x4)
    order = sorted(configs, key=lambda k: (k[0] != "nll_fwd", k))      # nll_fwd first: it writes the alpha / logz the others read
    for k in order:
        window(configs[k][0], 20)
    torch.cuda.synchronize()
    samples = {k: [] for k in order}
    for _ in range(args.rounds):
        for k in order:
            samples[k].append(window(configs[k][0], args.reps))
    res = {}
    for k in order:
        x = configs[k][1]
        med = statistics.median(samples[k])
        res["%s %s %s" % k] = {"us": round(med, 2), "min_us": round(min(samples[k]), 2), "max_us": round(max(samples[k]), 2),
                               "us_per_scan_step": round(med / x["max_len"], 3)}
    for name in ("viterbi", "nll_fwd", "nll_bwd", "posterior"):
        res["ratio wide/narrow at T=64 %s" % name] = round(res["%s wide 32x128x64" % name]["us"] / res["%s narrow 32x128x64" % name]["us"], 3)
    # ---- the tiny model's 4-sentence step at T = 137
    import selftest
    from kbner import batch as kb
    from kbner.engine import FusedAdamW
    cfg, tg, b, _ = selftest.tiny_setup(B=4, T=137)
    bd = kb.to_device(b, DEV)
    tg.train(True)
    opt = FusedAdamW(tg.arena, lr=1e-5, lr_rate=50.0, t_total=100000, warmup=0)

    def step():
        tg.forward_loss(bd, loss_scale=1.0, backward=True)
        opt.step()
        return 0

    window(step, 10)
    tiny = [window(step, 50) for _ in range(args.rounds)]
    Bc, nc = b["ctags"].shape
    xt = make(Bc, nc, 137, 4)
    ct = calls(lib, xt, True)
    for k in ("nll_fwd", "nll_bwd"):
        window(ct[k], 20)
    crf_t = [window(ct["nll_fwd"], args.reps) + window(ct["nll_bwd"], args.reps) for _ in range(args.rounds)]
    res["tiny 4-sentence step us (L2 H128 S64, T=137)"] = round(statistics.median(tiny), 1)
    res["tiny step CRF part us (nll_fwd + nll_bwd at %dx%dx137)" % (Bc, nc)] = round(statistics.median(crf_t), 1)
    res["tiny step CRF share"] = round(statistics.median(crf_t) / statistics.median(tiny), 4)
    full = res["nll_fwd wide 4x24x137"]["us"] + res["nll_bwd wide 4x24x137"]["us"]
    res["full-size 4-sentence CRF part us (nll_fwd + nll_bwd at 4x24x137)"] = round(full, 1)
    res["share of a 10 ms full-size step"] = round(full / 10000.0, 4)
    for k, v in res.items():
        print(k, v)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
