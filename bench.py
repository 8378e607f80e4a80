#!/usr/bin/env python
"""bench.py -- sentences/sec of XLM-R-large + CRF fine-tuning at seq_len 512 (BASELINE.json metric,
configs[1]) on N GPUs of one node; one process per GPU, RCCL all-reduce of gradients per optimizer step.

A "step" = one optimizer step = `accum` micro-batches of `micro_batch` synthetic 512-token sentences
(encoder fwd + gather + head + CRF NLL + full backward) + [all-reduce] + grad-norm clip + fused AdamW.
Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0.

  python bench.py --gpus 1 --steps 5 --warmup 2
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
  python bench.py --gpus N ...        (no launcher: re-executes itself under torch.distributed.run with N ranks)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "kb-ner_amd"))

MFMA_BF16_DENSE_PEAK_TFLOPS = 2500.0  # /opt/skills/guides/MI355X_MICROARCH.md: ~2.5 PF dense bf16
SUSTAINED_MFMA_RANDOM_BF16_TFLOPS = 1993.0   # measured, profiles/round2_mfma_power.txt (v_mfma_f32_16x16x32_bf16, 2.03-2.16 GHz)
HBM_PEAK_GBS = 8000.0
# Sentences per micro-batch of the default workload (x accumulate 1).  configs[1] fixes the model, the sequence length and the
# precision, not the batch: rounds 1-4 ran 128 (52 GB of saved activations), round 5 runs 256 (104 GB of the 288 GB): the per-step
# costs that do not grow with the batch (optimizer 3.7 ms, launch tails, the tile-count rounding of every GEMM) are paid once per 256
# sentences.  `extra.micro_batch_x_accumulate` keeps the 128 x 1 point and BASELINE.md's {1, 4, 16, 32} x 4 next to it.
DEFAULT_MICRO_BATCH = 256


def encoder_flops_per_sentence(cfg, S):
    """matmul FLOPs only, forward; fwd+bwd = 3x (no recompute counted)."""
    H, L = cfg.hidden_size, cfg.num_hidden_layers
    return L * (6 * S * H * H + 2 * S * H * H + 16 * S * H * H + 4 * S * S * H)


def host_threads():
    """Threads for the CPU leg: the container's CPU quota (cgroup v2 cpu.max) when there is one -- the GPU box
    exposes 256 logical CPUs under a 16-CPU quota, where 256 threads run 100x slower than 32 -- else the affinity
    mask; 2 threads per quota CPU measured best for torch's GEMMs (tools/cpu_probe.py)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(2 * int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, 64))


def cpu_baseline(args, cfg_kw, T, tags):
    """The oracle's fp32 torch-CPU restatement of the same step, timed on this box's host cores on a
    bounded sample (kind 'port').  Only rank 0 at N=1."""
    import numpy as np
    import torch
    from kbner import batch as kb
    from oracle import encoder as oenc
    from oracle import train_step as ots
    start, stop, x_idx = tags
    ncores = host_threads()
    torch.set_num_threads(ncores)
    ocfg = oenc.EncoderConfig(**cfg_kw)
    Bc = args.cpu_sentences
    t0 = time.time()
    params = oenc.init_params(ocfg, seed=kb.SEED)
    g = torch.Generator().manual_seed(1)
    params["linear.weight"] = torch.empty(T, ocfg.hidden_size).uniform_(-0.03, 0.03, generator=g)
    params["linear.bias"] = torch.zeros(T)
    tr = torch.randn(T, T, generator=g)
    tr[start, :] = -1e12
    tr[:, stop] = -1e12
    params["transitions"] = tr
    trainer = ots.OracleTrainer(params, ocfg, start, stop, x_idx, accum=1, t_total=1000)
    del params
    b = kb.synthetic_batch(Bc, args.seq_len, vocab=ocfg.vocab_size, T=T, x_idx=x_idx, start=start, stop=stop)
    ob = dict(input_ids=torch.from_numpy(b["input_ids"]), attention_mask=torch.from_numpy(b["attention_mask"]),
              first_idx=torch.from_numpy(b["first_idx"]), tags=torch.from_numpy(b["tags"].astype(np.int64)),
              lengths=torch.from_numpy(b["lengths"].astype(np.int64)))
    setup = time.time() - t0
    tw = time.time()
    trainer.micro_batch(ob)          # untimed warm-up step: first-touch allocation of activations / Adam state, thread-pool start
    trainer.optimizer_step()
    warm = time.time() - tw
    nt = max(1, args.cpu_steps)
    t1 = time.time()
    for _ in range(nt):
        trainer.micro_batch(ob)
        trainer.optimizer_step()
    dt = (time.time() - t1) / nt
    return {"value": Bc / dt, "unit": "sentences/sec", "cores": ncores, "kind": "port",
            "sample": "%d timed optimizer steps (after 1 untimed warm-up) of %d synthetic 512-token sentences each (fwd+bwd+clip+"
                      "AdamW, fp32 torch-CPU oracle, %d threads; %.1fs per timed step, warm-up step %.1fs, %.1fs setup)"
                      % (nt, Bc, ncores, dt, warm, setup)}


def id_variants(mb, n, vocab, seed):
    """n copies of a device micro-batch that differ in their content sub-token ids (uniform in [5, vocab), <s> / </s> kept): a training
    run never sees the same ids twice in a row, and with FusedAdamW.lazy_rows what a step costs depends on WHICH embedding rows it
    looks up -- rows nobody has visited for k steps owe k optimizer updates (kbner/engine.py).  The structure of the batch (word
    boundaries, tags, lengths) is untouched."""
    import torch
    dev = mb["ids"].device
    g = torch.Generator(device=dev).manual_seed(int(seed))
    S = int(mb["S"])
    M = int(mb["R"]) * S
    col = torch.arange(M, device=dev) % S
    interior = (col != 0) & (col != S - 1)
    out = []
    for _ in range(n):
        ids = mb["ids"].clone()
        fresh = torch.randint(5, int(vocab), (M,), device=dev, generator=g, dtype=torch.int32)
        ids[:M] = torch.where(interior, fresh, ids[:M])
        v = dict(mb)
        v["ids"] = ids
        out.append(v)
    return out


def impose_row_debt(opt, tokens_per_step, seed=0):
    """FusedAdamW.lazy_rows defers the zero-gradient updates of embedding rows until they are looked up.  A short benchmark that
    starts with every row up to date would measure the cheap transient (nobody owes anything yet); a long run with uniform ids
    settles where a row is visited with probability p = distinct rows per step / rows and owes j steps with P(j) = p (1 - p)^j
    (mean 1/p - 1: 121 steps at the YAMLs' 2 048 sub-tokens per step, 1.4 at 131 072).  This writes that distribution into the
    lazy clock (row_t = t - j, every row live), so that the timed steps do the catch-up work of the steady state: per step as
    many row updates as the eager optimizer performs, in registers instead of through HBM.  The debt is IMPOSED, not earned: the
    rows receive j updates more than a real run would have given them -- irrelevant on random-init weights, the cost of an update
    does not depend on the data.  (`--warmup 600` earns it instead: DESIGN.md section 8 compares the two.)"""
    import math
    import torch
    a = opt.arena
    z = a.lazy
    if z is None:
        return None
    a.materialize_rows()
    V = a.emb_flags.numel()
    p = 1.0 - math.exp(-float(tokens_per_step) / V)          # a row is among a step's ids with this probability
    horizon = min(int(8.0 / p) + 1, opt.LAZY_FULL_EVERY - 1)
    if opt.t < horizon:     # the clock starts late enough for the oldest debt: steps 1..horizon get their step sizes
        t_keep = opt.t
        b1, b2 = opt.betas
        hist = torch.zeros(horizon + 1, dtype=torch.float32)
        for s in range(1, horizon + 1):
            opt.t = s - 1
            hist[s] = opt.lr * opt.lr_lambda() * math.sqrt(1.0 - b2 ** s) / (1.0 - b1 ** s)
        opt.t = horizon
        if opt.t_total is not None:
            opt.t_total += horizon - t_keep
        z["hist"][:horizon + 1].copy_(hist.to(z["hist"].device))
        z["clock"].fill_(opt.t)
        z["last_full"] = opt.t
    g = torch.Generator(device=a.p.device).manual_seed(int(seed) + 77)
    u = torch.rand(V, device=a.p.device, generator=g).clamp_(1e-12, 1.0)
    j = torch.floor(torch.log(u) / math.log1p(-p)).clamp_(0, min(horizon, opt.t - 1)).to(torch.int32)
    a.emb_flags.fill_(1)
    z["row_t"].copy_(opt.t - j)
    z["dirty"] = True
    return {"p_row_visited_per_step": round(p, 6), "mean_owed_steps": round(float(j.float().mean()), 2), "horizon": horizon}


DUMP_PARAM_SAMPLE = 8 << 20     # parameters in the sample of the arena (32 MB of float32)
DUMP_SEED = 20220711


def dump_outputs(out_dir, tg, opt, last_losses):
    """What the last timed step handed its caller, as float32 .npy files: the loss of each of its micro-batches, the emissions of
    the last micro-batch, the head (linear + transitions) whole and a fixed seeded sample of the updated fp32 parameter arena (the
    same indices in every run with the same arguments).  Lazy embedding rows are brought up to date first, as any reader of the
    parameters does.  Untimed: runs after the timed region."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    a = tg.arena
    opt.materialize()
    torch.cuda.synchronize()
    arrays = {"loss": torch.stack([l.reshape(()) for l in last_losses]),
              "emissions": tg.last_emissions,
              "grad_norm_sq": opt.norm_sq,
              "linear_weight": a.param("linear.weight"), "linear_bias": a.param("linear.bias"),
              "transitions": a.param("transitions")}
    rng = np.random.default_rng(DUMP_SEED)
    idx = np.unique(rng.integers(0, a.n, size=min(DUMP_PARAM_SAMPLE, a.n), dtype=np.int64))
    arrays["params_sample"] = a.p.index_select(0, torch.from_numpy(idx).to(a.p.device))
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--micro-batch", type=int, default=DEFAULT_MICRO_BATCH)
    ap.add_argument("--accum", type=int, default=1)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--model", default="large", choices=["large", "base"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sentences", type=int, default=4)
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--blocking-allreduce", action="store_true", help="N>1: no overlap, everything exchanged after backward (A/B)")
    ap.add_argument("--compress-embedding-grad", action="store_true",
                    help="N>1: all-reduce the word-embedding gradient as bf16 when it is not row-sparse (deviation from the fp32 mean)")
    ap.add_argument("--dynamic-tiles", action="store_true", help="N=1: run the GEMMs with the dynamic tile scheduler the N>1 runs use (A/B)")
    ap.add_argument("--static-tiles", action="store_true", help="N>1: keep the static tile walk (A/B)")
    ap.add_argument("--gemm-shapes", action="store_true", help="print a per-shape GEMM timing table to stderr")
    ap.add_argument("--gemm-variant", type=int, default=None, help="kbner_gemm_set_variant(<int>) before the run (include/kbner.h; A/B)")
    # N > 1 knobs the first multi-GPU run can A/B without a code change (all echoed in dp_exchange)
    ap.add_argument("--nccl-max-nchannels", type=int, default=None, help="N>1: NCCL_MAX_NCHANNELS for RCCL (fewer channels = fewer CUs "
                    "held by a collective's kernels while backward runs; profiles/round5_cu_contention.txt)")
    ap.add_argument("--nccl-min-nchannels", type=int, default=None, help="N>1: NCCL_MIN_NCHANNELS for RCCL")
    ap.add_argument("--bucket-layers", type=int, default=4, choices=[4, 8, 12, 24], help="N>1: layers per gradient bucket (4 = one per grouped "
                    "weight-gradient launch, 201 MB; 8 = two launches per all-reduce, 402 MB)")
    ap.add_argument("--exchange-delay", type=int, default=0, help="N>1: issue a bucket's all-reduce only when this many later buckets are ready")
    ap.add_argument("--splitk-finish-kernel", action="store_true",
                    help="A/B (small micro-batches): fold split-K slabs with kbner_splitk_finish instead of inside the LayerNorm kernels")
    ap.add_argument("--eager-rows", action="store_true",
                    help="A/B: every live word-embedding row through HBM in every optimizer step (round 5) instead of FusedAdamW.lazy_rows")
    ap.add_argument("--no-extras", action="store_true", help="skip the secondary measurements (small micro-batches, dropout)")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="train with this dropout probability at the encoder's three HF sites + WordDropout (default 0: "
                         "BASELINE.md's workload is 'dropout off', and so is the cpu_baseline leg)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last one computed as DIR/<name>.npy (float32, < 64 MB in all): the "
                         "loss, the emissions, the head parameters, a fixed seeded sample of every updated parameter")
    ap.add_argument("--launch-check", action="store_true",
                    help="only check the launch: every rank joins a gloo group on the CPU, all-reduces its rank and rank 0 prints "
                         "{launch_check, world, ranks_seen}; no GPU work (tests/test_bench_launch_cpu.py)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become N ranks (one process per GPU) under torch.distributed.run on
        # this node -- the same command line the driver uses -- and pass its exit code on.  (KBNER_BENCH_LAUNCH_DRYRUN: print the
        # command instead; tests/test_bench_launch_cpu.py.)
        import subprocess
        if os.environ.get("KBNER_BENCH_CHILD"):
            sys.exit("bench.py: a launched rank found no WORLD_SIZE in its environment -- refusing to launch again")
        # --standalone: torchrun picks (and holds) a free rendezvous port itself -- no bind-then-close race between picking a
        # port here and the launcher binding it, and concurrent bench launches on one box cannot collide
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
               "--nproc-per-node", str(args.gpus), os.path.abspath(__file__)] + sys.argv[1:]
        if os.environ.get("KBNER_BENCH_LAUNCH_DRYRUN"):
            print(json.dumps({"launch": cmd}))
            return
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env["KBNER_BENCH_CHILD"] = "1"
        sys.exit(subprocess.call(cmd, env=env))

    if args.launch_check:
        import torch
        import torch.distributed as dist
        w, r = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
        seen = torch.zeros(w)
        seen[r] = 1.0
        if w > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
            dist.all_reduce(seen)
            dist.destroy_process_group()
        if r == 0:
            print(json.dumps({"launch_check": True, "n_gpus": args.gpus, "world": w, "ranks_seen": int(seen.sum().item())}))
        return

    import torch
    import torch.distributed as dist
    from kbner import batch as kb
    from kbner import engine, ops

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # one process per GPU over RCCL ("nccl" IS RCCL on ROCm).  KBNER_DIST_BACKEND=gloo is a functional-test escape
        # hatch only (several ranks sharing one GPU on a 1-GPU box); never used for reported numbers.
        if args.nccl_max_nchannels is not None:
            os.environ["NCCL_MAX_NCHANNELS"] = str(args.nccl_max_nchannels)
        if args.nccl_min_nchannels is not None:
            os.environ["NCCL_MIN_NCHANNELS"] = str(args.nccl_min_nchannels)
        backend = os.environ.get("KBNER_DIST_BACKEND", "nccl")
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    if args.gemm_variant is not None:
        ops.gemm_variant(args.gemm_variant)
    T, start, stop, x_idx = 29, 27, 28, 9  # resources/taggers/EN-English_x.pkl layout
    cfg_kw = dict(vocab_size=250002, max_position_embeddings=514)
    if args.model == "base":
        cfg_kw.update(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
    cfg = engine.EncoderConfig(hidden_dropout_prob=args.dropout, attention_probs_dropout_prob=args.dropout, **cfg_kw)
    tg = engine.Tagger(cfg, T, start, stop, device=dev)
    tg.init_random(seed=kb.SEED)  # identical replicas on every rank
    if args.dropout > 0.0:
        tg.train(True)
        tg.word_dropout = args.dropout
        tg.seed_dropout(kb.SEED + 7919 * rank)
    if args.splitk_finish_kernel:
        tg.FUSE_SPLITK_LN = False
    B, S, accum = args.micro_batch, args.seq_len, args.accum
    # each rank gets its own shard of synthetic sentences (weak scaling: per-GPU work fixed)
    micro = [kb.to_device(kb.synthetic_batch(B, S, vocab=cfg.vocab_size, T=T, x_idx=x_idx, start=start, stop=stop,
                                              seed=kb.SEED + 1000 * rank + i), dev) for i in range(accum)]
    total_steps = args.steps + args.warmup + 1
    opt = engine.FusedAdamW(tg.arena, lr=5e-6, lr_rate=10000.0, t_total=max(total_steps, 100))
    losses = []
    # The optimizer skips word-embedding rows that never received a gradient (exact, see FusedAdamW.step).  The synthetic ids are
    # uniform over all 250 002 rows, so a LONG run touches every row: the headline is measured in that steady state (every row
    # live from the first step), not in the cheaper transient of a 5-step run.  `extra.corpus_vocabulary_30k` shows what a corpus
    # that uses 30 000 distinct sub-tokens gets.
    if tg.arena.emb_flags is not None:
        tg.arena.emb_flags.fill_(1)
    # N = 1: the trainer's optimizer settings (flair/trainers/finetune_trainer.py: lazy_rows) on ids that change from step to step,
    # starting from the steady state of the deferred row updates (impose_row_debt).  N > 1 keeps round 5's fixed batches and the
    # eager row update: the data-parallel exchange marks other ranks' rows touched, which the lazy update handles (tests), but that
    # path has never met RCCL.
    row_debt = None
    micro_variants = None
    if world == 1:
        n_var = min(args.warmup + args.steps + 2, 1024 if B * S * accum <= 65536 else 48)
        micro_variants = [id_variants(m, n_var, cfg.vocab_size, kb.SEED + 4242 + 17 * i) for i, m in enumerate(micro)]
        if not args.eager_rows:
            opt.lazy_rows_for(B * S * accum)   # what the trainer does: lazy when a step visits at most 1/8 of the table
        row_debt = impose_row_debt(opt, B * S * accum, seed=kb.SEED)
    rows_mode = "lazy" if opt.lazy_rows else "eager"    # (of the timed run: the secondary measurements choose per step size)
    step_no = [0]

    # data parallel: the gradient exchange of a step overlaps with its backward (kbner.dp.GradReducer): the GEMM-weight
    # gradients travel as 6 buckets of 4 layers, each all-reduced (RCCL, async) as soon as its grouped weight-gradient launch
    # is enqueued; only embeddings + vectors + head are exchanged after backward.  --blocking-allreduce restores round 1's
    # single 2.24 GB all-reduce for A/B.
    reducer = None
    if world > 1 or args.dynamic_tiles:
        # N > 1: dynamic from the first bucket's all-reduce to the end of backward; --dynamic-tiles (the N = 1 A/B): every launch
        tg.dynamic_tiles = False if args.static_tiles else ("always" if args.dynamic_tiles else True)
    if world > 1:
        from kbner import dp
        a = tg.arena
        lo = a.offsets["emb.word"]
        Vv, Hh = a.shapes["emb.word"]
        reducer = dp.GradReducer(a.g, emb_range=(lo, lo + Vv * Hh), emb_width=Hh, compress_embedding=args.compress_embedding_grad,
                                 emb_flags=a.emb_flags, coalesce=args.bucket_layers // 4, delay=args.exchange_delay,
                                 finalize=a.finalize_grads)
    touched = None
    if reducer is not None:
        import numpy as np
        touched = np.unique(np.concatenate([m["ids"].cpu().numpy().ravel() for m in micro]))
    exposed = []

    def one_step(time_exchange=False):
        if reducer is not None:
            reducer.begin(touched)
        k = step_no[0]
        step_no[0] += 1
        for i, mb in enumerate(micro):
            if micro_variants is not None:
                mb = micro_variants[i][k % len(micro_variants[i])]
            hook = reducer.bucket_ready if (reducer is not None and i == len(micro) - 1 and not args.blocking_allreduce) else None
            losses.append(tg.forward_loss(mb, loss_scale=1.0 / accum, backward=True, grad_ready=hook))
        scale = 1.0
        if reducer is not None:
            if time_exchange:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            scale = reducer.finish()   # sum over ranks; AdamW applies 1/world (mean gradient)
            if time_exchange:
                e1.record()
                exposed.append((e0, e1))
        opt.step(grad_scale=scale)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    dp_fallback = None
    if reducer is not None and not args.blocking_allreduce:
        # pre-flight (untimed): the overlapped / sparse exchange has only ever run over gloo on the builder's 1-GPU boxes.  If
        # its first step raises under RCCL, say so in the JSON and fall back to round 1's blocking dense all-reduce rather than
        # lose the scaling measurement.  (The failure is REPORTED -- dp_exchange.fallback -- never hidden.)
        try:
            one_step()
            torch.cuda.synchronize()
        except Exception as e:   # noqa: BLE001
            dp_fallback = "%s: %s" % (type(e).__name__, e)
            print("bench.py: overlapped gradient exchange failed (%s); falling back to --blocking-allreduce" % dp_fallback,
                  file=sys.stderr)
            args.blocking_allreduce = True
            touched = None
            tg.dynamic_tiles = False
            reducer = dp.GradReducer(a.g, emb_range=None, emb_flags=a.emb_flags, finalize=a.finalize_grads)
            tg.arena.g.zero_()
        losses.clear()
    for _ in range(args.warmup):
        one_step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tg, opt, losses[-accum:])
    sentences = world * B * accum * args.steps
    value = sentences / dt
    loss_first, loss_last = float(losses[0]), float(losses[-1])

    roofline = None
    if not args.no_roofline:
        # live per-launch timing of the dominant kernel family (gemm_kernel<*>): HIP events on the launch
        # stream around every GEMM launch of ONE extra step; algorithmic FLOPs = 2*M*N*K per launch.
        recs = []
        ops.GEMM_HOOK = recs
        one_step()
        torch.cuda.synchronize()
        ops.GEMM_HOOK = None
        tot_fl = sum(r[2] for r in recs)
        tot_ms = sum(r[0].elapsed_time(r[1]) for r in recs)
        by = {}
        for s_ev, e_ev, fl, layout, _shape in recs:
            d = by.setdefault(layout, [0.0, 0.0, 0])
            d[0] += fl
            d[1] += s_ev.elapsed_time(e_ev)
            d[2] += 1
        ach = tot_fl / (tot_ms * 1e-3) / 1e12
        if args.gemm_shapes and rank == 0:   # per-shape breakdown of the same launches (stderr; not part of the JSON contract)
            sh = {}
            for s_ev, e_ev, fl, layout, shape in recs:
                d = sh.setdefault((layout,) + shape, [0.0, 0.0, 0])
                d[0] += fl
                d[1] += s_ev.elapsed_time(e_ev)
                d[2] += 1
            for k, v in sorted(sh.items(), key=lambda kv: -kv[1][1]):
                print("gemm layout %d nprob %2d M %6d N %5d K %6d epi %3d : %3d launches %8.3f ms %7.1f TFLOP/s"
                      % (k + (v[2], v[1], v[0] / (v[1] * 1e-3) / 1e12)), file=sys.stderr)
        # HBM-side bytes per launch of the same kernel family, from the committed rocprofv3 PMC passes of THIS command at its
        # default configuration (FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE; tools/pmc_traffic.py); None otherwise
        traffic, traffic_src = None, None
        pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
        cands = sorted(f for f in (os.listdir(pdir) if os.path.isdir(pdir) else []) if f.endswith("_hbm_traffic.json"))
        tpath = os.path.join(pdir, cands[-1]) if cands else ""
        tj = json.load(open(tpath)) if tpath else {}
        # (a traffic file says which micro-batch it was profiled at; the files of rounds 1-4 carry no tag: 128)
        if args.model == "large" and B == int(tj.get("micro_batch", 128)) and S == 512 and tpath:
            ks = [v for k, v in tj["kernels"].items() if "gemm256f_kernel" in k or "gemm256_kernel" in k]
            n = sum(v["launches"] for v in ks)
            if n:
                traffic = round(sum(v["launches"] * v["hbm_bytes_per_launch"] for v in ks) / n)
                traffic_src = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, bytes per launch)" % cands[-1]
        roofline = {"bound": "mfma", "kernel": "gemm256f_kernel<A_KS,B_KS> (bf16 MFMA 16x16x32, 256x256x64 tiles, interleaved-ring K loop, all 3 layouts; "
                              "at N > 1 the same kernel with one workgroup per tile while a gradient bucket may be in flight)",
                    "achieved": round(ach, 2), "peak": MFMA_BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach / MFMA_BF16_DENSE_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_src,
                    "algorithmic_flops_per_launch": round(tot_fl / max(len(recs), 1)),
                    "launches_per_step": len(recs), "gemm_ms_per_step": round(tot_ms, 3),
                    # informational: what a register-only MFMA loop sustains on random bf16 operands under the 1400 W package
                    # cap (tools/micro/mfma_power.hip, profiles/round2_mfma_power.txt); `peak` / `frac` stay the data-sheet ones
                    "sustained_mfma_peak_random_bf16": SUSTAINED_MFMA_RANDOM_BF16_TFLOPS,
                    "frac_of_sustained": round(ach / SUSTAINED_MFMA_RANDOM_BF16_TFLOPS, 4),
                    "by_layout": {("NT_fwd", "NN_dgrad", "TN_wgrad")[k]: {"tflops": round(v[0] / (v[1] * 1e-3) / 1e12, 2),
                                                                              "ms": round(v[1], 3), "launches": v[2]}
                                  for k, v in sorted(by.items())}}

    # the HBM-bound kernels SURVEY.md section 8d assigns to the bandwidth roofline, timed live like the GEMMs: HIP events on the launch
    # stream around every launch of ONE extra step (every embedding row live); algorithmic bytes per the survey / DESIGN.md section 3
    roofline_hbm = None
    if not args.no_roofline:
        try:
            hrec = []
            was_lazy = opt.lazy_rows
            opt.lazy_rows = False             # the eager row kernels: every live row through HBM, the survey's 28 B per parameter
            if tg.arena.emb_flags is not None:
                tg.arena.emb_flags.fill_(3)   # LIVE | TOUCHED: the row kernels move their whole algorithmic bytes in this step
            ops.HBM_HOOK = hrec
            one_step()
            torch.cuda.synchronize()
            ops.HBM_HOOK = None
            opt.lazy_rows = was_lazy
            agg = {}
            for name, e0, e1, nb in hrec:
                d = agg.setdefault(name, [0.0, 0.0, 0])
                d[0] += nb
                d[1] += e0.elapsed_time(e1)
                d[2] += 1
            roofline_hbm = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "achievable_copy_GBs": 6290.0,
                            "note": "achieved = algorithmic bytes / live HIP-event time per kernel over one step; peak 8 TB/s data sheet, "
                                    "6.29 TB/s = the guide's measured float4 copy",
                            "kernels": {k: {"achieved": round(v[0] / (v[1] * 1e-3) / 1e9, 1), "frac": round(v[0] / (v[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                            "launches": v[2], "ms": round(v[1], 3), "algorithmic_bytes": round(v[0])}
                                        for k, v in sorted(agg.items()) if v[1] > 0}}
        except Exception as e:   # noqa: BLE001
            ops.HBM_HOOK = None
            roofline_hbm = {"error": "%s: %s" % (type(e).__name__, e)}

    # data parallel: how long the compute stream waits for / runs the part of the exchange backward could not hide
    # (HIP events around GradReducer.finish() on one extra step); None at N=1
    allreduce_ms_exposed, dp_stats = None, None
    if reducer is not None:
        one_step(time_exchange=True)
        torch.cuda.synchronize()
        allreduce_ms_exposed = round(max(a.elapsed_time(b) for a, b in exposed), 3)
        dp_stats = dict(reducer.stats)
        if dp_fallback is not None:
            dp_stats["fallback"] = dp_fallback
        # self-explaining SCALE line: what ran, with which knobs, and what each collective costs on its own.  Everything here is a
        # REPORT: nothing in this block may cost the scaling measurement (it has never run over RCCL on the builder's 1-GPU boxes)
        try:
            seen = torch.zeros(world, device=dev)
            seen[rank] = 1.0
            dist.all_reduce(seen)
            try:
                rccl = ".".join(str(x) for x in torch.cuda.nccl.version()) if dist.get_backend() == "nccl" else None
            except Exception as e:   # noqa: BLE001
                rccl = "unknown (%s)" % type(e).__name__
            dp_stats.update({"world": world, "ranks_seen": int(seen.sum().item()), "backend": dist.get_backend(), "rccl_version": rccl,
                             "NCCL_MAX_NCHANNELS": os.environ.get("NCCL_MAX_NCHANNELS"), "NCCL_MIN_NCHANNELS": os.environ.get("NCCL_MIN_NCHANNELS"),
                             "bucket_layers": args.bucket_layers, "exchange_delay": args.exchange_delay,
                             "blocking_allreduce": bool(args.blocking_allreduce),
                             "tile_schedule": "static" if args.static_tiles else "one workgroup per tile from the first bucket to the end of backward"})
            if not args.blocking_allreduce:
                # one more step with every bucket all-reduce BLOCKING and timed on the compute stream: the isolated cost of each collective
                reducer.time_buckets = True
                one_step()
                torch.cuda.synchronize()
                reducer.time_buckets = False
                dp_stats["bucket_allreduce_us_isolated"] = [round(e0.elapsed_time(e1) * 1e3, 1) for _, e0, e1 in reducer.bucket_events]
                dp_stats["bucket_bytes"] = [int(nb) for nb, _, _ in reducer.bucket_events]
                dp_stats["bucket_busbw_GBs"] = [round(2 * (world - 1) / world * nb / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
                                                for nb, e0, e1 in reducer.bucket_events if e0.elapsed_time(e1) > 0]
        except Exception as e:   # noqa: BLE001
            dp_stats["diagnostics_error"] = "%s: %s" % (type(e).__name__, e)
            reducer.time_buckets = False

    # secondary measurements of the SAME step at the other points BASELINE.md / SURVEY.md §8d name: micro-batch {1,4,16,32} x
    # accumulate 4 (the YAMLs run 1 x 4) and dropout 0.1 at every site -- N=1, default workload only, a few steps each
    extra = None
    if world == 1 and not args.no_extras and args.model == "large" and B == DEFAULT_MICRO_BATCH and accum == 1 and args.dropout == 0.0:
        extra = {"micro_batch_x_accumulate": {}, "unit": "sentences/sec"}

        def timed(tgx, optx, mbs, steps, warm=1):
            # like the main loop: fresh ids every step, from the steady state of the deferred row updates at THIS step size
            var = [id_variants(m, steps + warm, cfg.vocab_size, kb.SEED + 999 + 31 * i + sum(int(x["B"]) for x in mbs))
                   for i, m in enumerate(mbs)]
            if not args.eager_rows:
                optx.lazy_rows_for(sum(int(x["B"]) * int(x["S"]) for x in mbs))
            impose_row_debt(optx, sum(int(x["B"]) * int(x["S"]) for x in mbs), seed=kb.SEED + len(mbs))
            kk = [0]

            def st():
                for v in var:
                    tgx.forward_loss(v[kk[0]], loss_scale=1.0 / len(mbs), backward=True)
                kk[0] += 1
                optx.step()
            for _ in range(warm):
                st()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                st()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps

        for mbsz in (1, 4, 16, 32):
            mbs = [kb.to_device(kb.synthetic_batch(mbsz, S, vocab=cfg.vocab_size, T=T, x_idx=x_idx, start=start, stop=stop,
                                                   seed=kb.SEED + 50 + i), dev) for i in range(4)]
            sec = timed(tg, opt, mbs, steps=3 if mbsz >= 16 else 6)
            extra["micro_batch_x_accumulate"]["%dx4" % mbsz] = {"value": round(4 * mbsz / sec, 2), "ms_per_step": round(sec * 1e3, 3)}
        # the fused form the drop-in trainer uses for the YAMLs' 1 x 4 (one weighted batch of 4: same loss and gradient)
        mb4 = [kb.to_device(kb.synthetic_batch(4, S, vocab=cfg.vocab_size, T=T, x_idx=x_idx, start=start, stop=stop,
                                               seed=kb.SEED + 60), dev)]
        sec = timed(tg, opt, mb4, steps=40, warm=5)    # (0.45 s: six 10-ms steps were a noisy sample of the YAML regime's number)
        extra["micro_batch_x_accumulate"]["1x4_fused_by_trainer"] = {"value": round(4 / sec, 2), "ms_per_step": round(sec * 1e3, 3)}
        # rounds 1-4's headline point, 128 sentences per launch (52 GB of saved activations): the fixed per-step costs (optimizer,
        # launch tails) amortise over half the sentences -- kept for continuity with BENCH_r01..r04
        try:
            mb128 = [kb.to_device(kb.synthetic_batch(128, S, vocab=cfg.vocab_size, T=T, x_idx=x_idx, start=start, stop=stop,
                                                     seed=kb.SEED + 80), dev)]
            sec = timed(tg, opt, mb128, steps=4, warm=2)
            extra["micro_batch_x_accumulate"]["128x1"] = {"value": round(128 / sec, 2), "ms_per_step": round(sec * 1e3, 3),
                                                           "mfma_fraction_end_to_end": round(128 / sec * 3 * encoder_flops_per_sentence(cfg, S) / (MFMA_BF16_DENSE_PEAK_TFLOPS * 1e12), 4)}
            del mb128
            tg._acts.pop((128, S), None)
            torch.cuda.empty_cache()
        except Exception as e:
            extra["micro_batch_x_accumulate"]["128x1"] = {"error": repr(e)}
        tg.cfg.hidden_dropout_prob = tg.cfg.attention_probs_dropout_prob = 0.1
        tg.train(True)
        tg.word_dropout = 0.1
        sec = timed(tg, opt, micro, steps=3)
        tg.train(False)
        tg.cfg.hidden_dropout_prob = tg.cfg.attention_probs_dropout_prob = 0.0
        extra["dropout_0.1_all_sites_%dx1" % B] = {"value": round(B / sec, 2), "ms_per_step": round(sec * 1e3, 3)}
        # what a corpus that uses 30 000 distinct sub-tokens gets (ids uniform in [5, 30000) instead of the whole 250 002-row
        # table): fresh optimizer state, only rows that receive a gradient are live, the other 88 % of the word-embedding table
        # (40 % of all parameters) are skipped by the clip norm and by AdamW -- exactly, their g / m / v are zero
        if tg.arena.emb_flags is not None:
            was_lazy = opt.lazy_rows
            opt.lazy_rows = False      # (the optimizer state is rewritten by hand below: the lazy clock restarts from it)
            tg.arena.emb_flags.zero_()
            tg.arena.m.zero_()
            tg.arena.v.zero_()
            tg.arena.g.zero_()
            opt.lazy_rows = was_lazy
            cv = {}
            mb4c = [kb.to_device(kb.synthetic_batch(4, S, vocab=30000, T=T, x_idx=x_idx, start=start, stop=stop, seed=kb.SEED + 61 + i),
                                 dev) for i in range(8)]
            mbc = [kb.to_device(kb.synthetic_batch(B, S, vocab=30000, T=T, x_idx=x_idx, start=start, stop=stop, seed=kb.SEED + 70), dev)]

            def timed_seq(batches, steps, warm):
                k = 0
                for _ in range(warm):
                    tg.forward_loss(batches[k % len(batches)], loss_scale=1.0, backward=True)
                    opt.step()
                    k += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    tg.forward_loss(batches[k % len(batches)], loss_scale=1.0, backward=True)
                    opt.step()
                    k += 1
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / steps

            sec = timed_seq(mbc, steps=3, warm=2)     # the big batch first: it makes (nearly) all 30 000 rows live
            cv["%dx1" % B] = {"value": round(B / sec, 2), "ms_per_step": round(sec * 1e3, 3)}
            sec = timed_seq(mb4c, steps=8, warm=2)
            cv["1x4_fused_by_trainer"] = {"value": round(4 / sec, 2), "ms_per_step": round(sec * 1e3, 3)}
            cv["live_rows"] = int((tg.arena.emb_flags != 0).sum())
            extra["corpus_vocabulary_30k"] = cv
        # BASELINE.md section 2 row 5 / SURVEY.md section 8d cfg 5 (ACE-style stack, inference): Viterbi alone and encoder + Viterbi at
        # the four (B, n') points, the whole stack (3 XLM-R-large-sized encoders + 4 character LMs + BiLSTM + CRF) at B = 32, and
        # FastSequenceTagger.evaluate end to end -- secondary lines, measured by tools/bench_stack.py / tools/train_throughput.py
        try:
            import importlib.util

            def _tool(name):
                spec = importlib.util.spec_from_file_location("kbner_tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                return mod
            tg._acts.clear()          # the training step's activation buffers are not needed any more
            torch.cuda.empty_cache()
            extra["cfg5"] = _tool("bench_stack").measure(encoders=3, lms=4, reps=3)
            # SURVEY.md section 8d cfg 5 as specified: emissions f32[B, n', 29] ~ N(0, 1), transitions ~ N(0, 1) with the START row / STOP
            # column at -1e12, Viterbi ALONE at the four (B, n') points incl. the real (32, 512); bytes/s against HBM as the survey asks
            # (algorithmic bytes per sentence: 4 T n' emissions + 4 T^2 transitions + T n' backpointers + 8 n' outputs) -- a sequential
            # 29 x 29 max-plus scan per token: latency-bound by construction, the fraction says so
            gv = torch.Generator(device=dev).manual_seed(20220711)
            trv = torch.randn(T, T, device=dev, generator=gv)
            trv[start, :] = -1e12
            trv[:, stop] = -1e12
            va = {}
            for Bv, nv in ((32, 16), (32, 64), (256, 32), (32, 512)):
                emv = torch.randn(Bv, nv, T, device=dev, generator=gv)
                lnv = torch.full((Bv,), nv, dtype=torch.int32, device=dev)
                for _ in range(3):
                    ops.crf_viterbi(emv, trv, lnv, start, stop)
                torch.cuda.synchronize()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(50):
                    ops.crf_viterbi(emv, trv, lnv, start, stop)
                ev1.record()
                torch.cuda.synchronize()
                sec = ev0.elapsed_time(ev1) * 1e-3 / 50
                nbytes = Bv * (4 * T * nv + 4 * T * T + T * nv + 8 * nv)
                va["B%d_n%d" % (Bv, nv)] = {"us": round(sec * 1e6, 1), "sentences_per_s": round(Bv / sec), "tokens_per_s": round(Bv * nv / sec),
                                            "algorithmic_bytes": nbytes, "GBs": round(nbytes / sec / 1e9, 2),
                                            "frac_of_hbm_peak": round(nbytes / sec / 1e9 / HBM_PEAK_GBS, 6)}
            extra["cfg5_viterbi_alone_N01"] = va
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            extra["evaluate"] = _tool("train_throughput").evaluate_rate(sentences=512, batch=32, model="large")
        except Exception as e:  # secondary measurements never cost the headline number
            extra["cfg5_error"] = repr(e)

    if rank == 0:
        fl_sent = 3 * encoder_flops_per_sentence(cfg, S)
        out = {
            "metric": "sentences/sec XLM-R-%s+CRF fine-tune seq512" % args.model,
            "value": round(value, 2), "unit": "sentences/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "configs[1]: xlm-roberta-%s (random-init, L%d/H%d/A%d/F%d, V=250002) + linear head + CRF (T=29), "
                                   "seq_len=%d, bf16 MFMA GEMMs/attention, fp32 master weights + AdamW(HF) + clip 5.0, "
                                   "dropout %s" % (args.model, cfg.num_hidden_layers, cfg.hidden_size, cfg.num_attention_heads,
                                                   cfg.intermediate_size, S,
                                                   ("%.2f (embeddings, attention probabilities, sub-layer outputs, WordDropout)"
                                                    % args.dropout) if args.dropout > 0 else "off (BASELINE.md workload spec)"),
                       "micro_batch": B, "accumulate": accum, "global_batch": world * B * accum, "seq_len": S,
                       "parallelism": "dp%d" % world},
            "encoder_tflops_fwd_bwd_per_sentence": round(fl_sent / 1e12, 4),
            "mfma_fraction_end_to_end": round(value / world * fl_sent / (MFMA_BF16_DENSE_PEAK_TFLOPS * 1e12), 4),
            "loss_first": round(loss_first, 4), "loss_last": round(loss_last, 4),
            # N = 1: content ids are redrawn every step; with lazy embedding rows the run starts from the steady state of the deferred
            # row updates (impose_row_debt: as many row updates per step as the eager optimizer performs, done in registers)
            "optimizer": {"embedding_rows": rows_mode, "ids": "fresh per step" if micro_variants is not None else "fixed",
                          "row_debt": row_debt},
        }
        if roofline is not None:
            out["roofline"] = roofline
        if roofline_hbm is not None:
            out["roofline_hbm"] = roofline_hbm
        # rounds 1-4 quoted the headline at 128 sentences per launch: the same figure at top level, so that BENCH_r01..r06 compare
        # like for like (`value` itself is at config.micro_batch)
        r128 = (extra or {}).get("micro_batch_x_accumulate", {}).get("128x1", {})
        if "value" in r128:
            out["value_at_128x1"] = r128["value"]
            out["mfma_fraction_end_to_end_at_128x1"] = r128.get("mfma_fraction_end_to_end")
        out["allreduce_ms_exposed"] = allreduce_ms_exposed
        if dp_stats is not None:
            out["dp_exchange"] = dp_stats
        if extra is not None:
            out["extra"] = extra
        if world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args, cfg_kw if args.model == "base" else dict(cfg_kw), T, (start, stop, x_idx))
            except Exception as e:  # the baseline is a report, never a reason to lose the GPU number
                out["cpu_baseline"] = {"error": repr(e)}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
