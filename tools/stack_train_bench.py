"""One optimizer step of the stacked tagger's head alone -- input GEMM, BiLSTM recurrence forward and backward, linear head, CRF NLL,
weight gradients, optimizer -- on the HIP path (kbner.stack.BiLSTMHead.loss_backward + StackOptimizer) against stock PyTorch on the
same GPU (torch.nn.LSTM(D, H, bidirectional) + linear + a torch CRF NLL + torch.optim.AdamW, fp32 and bf16 autocast).

Shape: the ACE YAML's by default (B 32, n 64, H 1000, D 5120, T 21).  Method: alternating rounds in one process, warm-up first, the
median of `--rounds` timed steps per variant (HIP events around the step).  The two PyTorch variants share one set of parameters
(the second starts where the first's step left them: their first losses differ).  Prints one JSON line.  No threshold: the numbers go into
DESIGN.md section 3 as measured.

    python tools/stack_train_bench.py [--B 32 --n 64 --H 1000 --D 5120 --T 21 --rounds 5 --warmup 2]
"""
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


def crf_nll(em, tags, lens, trans, start, stop):
    """mean over sentences of logZ - gold score; em [B, n, T], trans[to, from]"""
    B, n, T = em.shape
    alpha = torch.full((B, T), -1e4, device=em.device, dtype=em.dtype)
    alpha[:, start] = 0.0
    for i in range(n):
        nxt = torch.logsumexp(em[:, i, :, None] + trans[None] + alpha[:, None, :], dim=2)
        live = (lens > i)[:, None]
        alpha = torch.where(live, nxt, alpha)
    final = alpha
    logz = torch.logsumexp(final + trans[stop][None], dim=1)
    mask = (torch.arange(n, device=em.device)[None] < lens[:, None]).to(em.dtype)
    prev = torch.cat([torch.full((B, 1), start, device=em.device, dtype=tags.dtype), tags[:, :-1]], 1)
    gold = ((em.gather(2, tags[:, :, None])[:, :, 0] + trans[tags, prev]) * mask).sum(1)
    last = tags.gather(1, (lens - 1).clamp(min=0)[:, None])[:, 0]
    gold = gold + trans[stop, last]
    return (logz - gold).mean()


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("B", 32), ("n", 64), ("H", 1000), ("D", 5120), ("T", 21), ("rounds", 5), ("warmup", 2)):
        ap.add_argument("--" + k, type=int, default=v)
    a = ap.parse_args()
    from kbner import batch as kb
    from kbner import stack as K
    B, n, H, D, T = a.B, a.n, a.H, a.D, a.T
    rng = np.random.default_rng(0)
    k = 1.0 / np.sqrt(H)
    st = {"rnn": {}}
    for s in ("", "_reverse"):
        st["rnn"]["weight_ih_l0" + s] = rng.uniform(-k, k, (4 * H, D)).astype(np.float32)
        st["rnn"]["weight_hh_l0" + s] = rng.uniform(-k, k, (4 * H, H)).astype(np.float32)
        st["rnn"]["bias_ih_l0" + s] = rng.uniform(-k, k, 4 * H).astype(np.float32)
        st["rnn"]["bias_hh_l0" + s] = rng.uniform(-k, k, 4 * H).astype(np.float32)
    st["linear.weight"] = (rng.uniform(-1, 1, (T, 2 * H)) / np.sqrt(2 * H)).astype(np.float32)
    st["linear.bias"] = np.zeros(T, np.float32)
    tr = rng.standard_normal((T, T)).astype(np.float32)
    tr[T - 2, :] = -1e4
    tr[:, T - 1] = -1e4
    st["transitions"] = tr
    lengths = rng.integers(n // 2, n + 1, size=B)
    lengths[0] = n
    tags = rng.integers(0, T - 2, (B, n))
    x = rng.standard_normal((B, n, D)).astype(np.float32)
    for b in range(B):
        x[b, lengths[b]:] = 0
    # ---- HIP
    head = K.BiLSTMHead({kk: torch.from_numpy(v) for kk, v in st["rnn"].items()}, st["linear.weight"], st["linear.bias"], [D], H, "cuda",
                        transitions=st["transitions"], trainable=True)
    opt = K.StackOptimizer(head, name="AdamW", lr=1e-3, lr_rate=1.0)
    X = head.new_input(B, n)
    X[:B * n, :D] = torch.from_numpy(x).view(B * n, D).to(torch.bfloat16).cuda()
    hb = kb.assemble(np.zeros((B, 1), np.int64), np.ones((B, 1), np.int64), np.full((B, n), -1, np.int64), tags.astype(np.int64),
                     lengths.astype(np.int64), None)
    db = kb.to_device(hb, "cuda")

    def hip_step():
        loss = head.loss_backward(X, lengths, B, n, db, T - 2, T - 1)
        opt.step()
        return loss

    # ---- stock PyTorch
    rnn = torch.nn.LSTM(D, H, 1, bidirectional=True, batch_first=True).cuda()
    with torch.no_grad():
        for kk, p in rnn.named_parameters():
            p.copy_(torch.from_numpy(st["rnn"][kk]))
    lin = torch.nn.Linear(2 * H, T).cuda()
    trans = torch.nn.Parameter(torch.from_numpy(tr).cuda())
    params = list(rnn.parameters()) + list(lin.parameters()) + [trans]
    topt = torch.optim.AdamW(params, lr=1e-3, eps=1e-6, weight_decay=0.0)
    xt = torch.from_numpy(x).cuda()
    lens_c = torch.from_numpy(lengths)
    lens_d, tags_d = lens_c.cuda(), torch.from_numpy(tags).cuda()

    def torch_step(autocast):
        topt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            packed = torch.nn.utils.rnn.pack_padded_sequence(xt, lens_c, batch_first=True, enforce_sorted=False)
            y, _ = rnn(packed)
            y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=n)
            em = lin(y)
        loss = crf_nll(em.float(), tags_d, lens_d, trans, T - 2, T - 1)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        topt.step()
        return loss

    variants = [("hip", hip_step), ("torch_fp32", lambda: torch_step(False)), ("torch_bf16_autocast", lambda: torch_step(True))]
    times = {name: [] for name, _ in variants}
    first = {}
    for r in range(a.warmup + a.rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            loss = fn()
            e1.record()
            torch.cuda.synchronize()
            if r == 0:
                first[name] = float(loss.detach())
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    out = {"shape": {"B": B, "n": n, "H": H, "D": D, "T": T}, "rounds": a.rounds, "first_loss": first,
           "median_ms": {k_: float(np.median(v)) for k_, v in times.items()}, "all_ms": {k_: [round(t, 3) for t in v] for k_, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
