"""TEST INFRASTRUCTURE: float64 references of the encoder layer selection -- kbner_gather_rows_layers / kbner_scatter_add_rows_ld
(include/kbner.h) and one tagger step whose token feature is the concatenation, or the mean, of several hidden states
(TransformerWordEmbeddings(layers=..., use_scalar_mix=...)).  numpy for the kernels (built on tests/headdropref.py's multiplier, which
is keyed by the global column already); torch autograd over oracle/encoder.py for the step.  No import of kbner except in
tiny_setup_layers, which builds the engine under test.

Rows are laid out [B, n] (R = B * n).  k sources x_j [rows_src, H]; W = k * H (concatenation) or H (mean).
    gather, concat: y[r, j * H + h] = idx[r] >= 0 ? x_j[idx[r], h] * M[r, j * H + h] : 0
    gather, mean  : y[r, h]         = idx[r] >= 0 ? (sum_j x_j[idx[r], h]) / k * M[r, h] : 0
    scatter-add   : dst[idx[r], h] += d[r, col0 + h] * M[r, col0 + h] * scale      for idx[r] >= 0 (unique), M of the ld-wide row

BOUNDS (per element, against the float64 reference; the kernels read bf16, compute in float32, store bf16):
    gather, concat  headdropref.real_bound: one bf16 rounding + the float32 roundings of the multiplier and the product.  Without
                    dropout the kernel copies: bit equality.
    gather, mean    2^-8 |ref| + (k + 4) * 2^-24 * (sum_j |x_j| / k) * |M|
                    k - 1 float32 additions of the running sum, each at most 2^-24 of a partial sum <= sum_j |x_j|; the rounded
                    constant 1 / k; its product with the sum; the multiplier's own product (scale_e * scale_l) and its product with
                    the value: (k - 1) + 1 + 1 + 2 = k + 3 roundings, one more for the compounding of the (1 + 2^-24) factors; all of
                    them relative to sum_j |x_j| / k * |M|, which bounds every intermediate.  Then one bf16 rounding of the result.
    scatter-add     2^-8 |ref| + 4 * 2^-24 * (|dst| + |d * M * scale|)
                    the multiplier's product, M * scale, the product with d (three roundings relative to the term), the addition
                    (relative to |dst| + |term|); then one bf16 rounding of the result.
    head_bwd_dx     rowref.tolerance(..., bf16_out=True), as tests/test_gpu_head_wide.py uses it."""
import numpy as np
import torch

import headdropref as hd
import mmaref

F32, F64 = np.float32, np.float64
NO_DROP = hd.NO_DROP


def gather_layers(xs64, idx, n, mean=False, drop_e=NO_DROP, drop_l=NO_DROP):
    """float64, unrounded; xs64: k arrays [rows_src, H]; idx [R] -> [R, k * H] (concatenation) or [R, H] (mean)"""
    xs = [np.asarray(x, F64) for x in xs64]
    idx = np.asarray(idx, np.int64)
    k, H, R = len(xs), xs[0].shape[1], idx.size
    feat = sum(xs[1:], xs[0].copy()) / k if mean else np.concatenate(xs, axis=1)
    W = feat.shape[1]
    assert W == (H if mean else k * H)
    M = hd.mult(R, W, n, drop_e, drop_l).astype(F64)
    y = np.zeros((R, W), F64)
    ok = idx >= 0
    y[ok] = feat[idx[ok]] * M[ok]
    return y


def gather_abs(xs64, idx, n, mean, drop_e=NO_DROP, drop_l=NO_DROP):
    """sum_j |x_j| / k * |M| at the gathered rows (mean), the quantity the mean bound is relative to"""
    return gather_layers([np.abs(np.asarray(x, F64)) for x in xs64], idx, n, mean, drop_e, drop_l)


def scatter_add_ld(dst64, d64, ld, col0, idx, scale, n, drop_e=NO_DROP, drop_l=NO_DROP):
    """-> (dst after the add, |dst before| + |term| per element: what the bound is relative to); float64, dst64 [rows, H], d64 [R, ld]"""
    dst = np.asarray(dst64, F64).copy()
    d = np.asarray(d64, F64)
    idx = np.asarray(idx, np.int64)
    R, H = idx.size, dst.shape[1]
    assert d.shape[1] == ld and col0 + H <= ld
    M = hd.mult(R, ld, n, drop_e, drop_l).astype(F64)[:, col0:col0 + H]
    ok = idx >= 0
    assert np.unique(idx[ok]).size == int(ok.sum()), "scatter_add_ld: indices must be unique"
    term = d[:R, col0:col0 + H][ok] * M[ok] * F64(F32(scale))
    mag = np.abs(dst)
    mag[idx[ok]] += np.abs(term)
    dst[idx[ok]] += term
    return dst, mag


def gather_mean_bound(ref64, abs64, k):
    return 2.0 ** -8 * np.abs(ref64) + (k + 4) * 2.0 ** -24 * np.abs(abs64)


def scatter_add_bound(ref64, mag64):
    return 2.0 ** -8 * np.abs(ref64) + 4 * 2.0 ** -24 * np.abs(mag64)


# ------------------------------------------------------------------ float32 restatements (tests/test_layers_cpu.py: the bounds hold
# for a plain float32 evaluation in the kernels' order of operations)
def gather_mean_f32(xs, idx, n, drop_e=NO_DROP, drop_l=NO_DROP):
    xs = [np.asarray(x, F32) for x in xs]
    idx = np.asarray(idx, np.int64)
    k, H, R = len(xs), xs[0].shape[1], idx.size
    acc = xs[0].copy()
    for x in xs[1:]:
        acc = (acc + x).astype(F32)
    acc = (acc * F32(F32(1.0) / F32(k))).astype(F32)
    M = hd.mult(R, H, n, drop_e, drop_l)
    y = np.zeros((R, H), F32)
    ok = idx >= 0
    y[ok] = (acc[idx[ok]] * M[ok]).astype(F32)
    return y


def scatter_add_f32(dst, d, ld, col0, idx, scale, n, drop_e=NO_DROP, drop_l=NO_DROP):
    dst = np.asarray(dst, F32).copy()
    d = np.asarray(d, F32)
    idx = np.asarray(idx, np.int64)
    R, H = idx.size, dst.shape[1]
    M = hd.mult(R, ld, n, drop_e, drop_l)[:, col0:col0 + H]
    ok = idx >= 0
    f = (M[ok] * F32(scale)).astype(F32)
    dst[idx[ok]] = (dst[idx[ok]] + (d[:R, col0:col0 + H][ok] * f).astype(F32)).astype(F32)
    return dst


def round_bf16(a):
    """float -> the nearest bf16 number (ties to even), as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).bfloat16().float().numpy().astype(F64)


# ------------------------------------------------------------------ the kernel case list (tests/test_gpu_layers_kernels.py runs it on the
# GPU, tests/test_layers_cpu.py checks the bounds on it in float32)
SHAPES = [(1, 1), (6, 3), (70, 7)]                     # (R, n)
WIDTHS = [8, 128, 520, 1024]                           # H
DROPS = {"none": (0.0, 0.0), "element": (0.1, 0.0), "locked": (0.0, 0.3), "both": (0.1, 0.3)}


def gather_cases():
    """(R, n, H, k, mean, drop): a pruned walk over the grid -- every value of every axis, H = 520 with k = 3 and both masks, R = 1"""
    cases = []
    i = 0
    for R, n in SHAPES:
        for H in WIDTHS:
            for k in (1, 2, 3, 4):
                for mean in (False, True):
                    for drop in DROPS:
                        i += 1
                        must = (H == 520 and k == 3 and drop == "both") or (R == 1 and H == 8 and drop in ("none", "both") and k in (1, 3))
                        if must or i % 9 == 0:
                            cases.append((R, n, H, k, mean, drop))
    return cases


GATHER_CASES = gather_cases()
SCATTER_CASES = [(R, n, H, c, scale, drop) for (R, n), H, c, scale, drop in
                 [((1, 1), 8, 0, 1.0, "none"), ((1, 1), 8, 3, 0.25, "both"), ((6, 3), 128, 1, 1.0, "element"), ((6, 3), 520, 3, 0.25, "both"),
                  ((6, 3), 1024, 0, 1.0, "locked"), ((70, 7), 8, 1, 0.25, "locked"), ((70, 7), 128, 3, 1.0, "both"),
                  ((70, 7), 520, 0, 0.25, "none"), ((70, 7), 520, 1, 1.0, "both"), ((70, 7), 1024, 3, 0.25, "element"),
                  ((1, 1), 1024, 1, 1.0, "both"), ((6, 3), 8, 0, 0.25, "element")]]        # c: col0 = c * H, ld = 4 * H


def sites(drop, salt):
    p_e, p_l = DROPS[drop]
    return ((0x9E3779B9 ^ (salt * 7919)) & 0xFFFFFFFF, mmaref.dropout_thresh(p_e)), ((0xC2B2AE35 + salt * 104729) & 0xFFFFFFFF,
                                                                                       mmaref.dropout_thresh(p_l))


def bf16_values(rng, shape):
    """Gaussian values that are bf16 numbers, none of them 0 (float64)"""
    t = torch.from_numpy(rng.standard_normal(shape).astype(F32)).bfloat16()
    t[t == 0] = 1.0
    return t.float().numpy().astype(F64)


def gather_inputs(R, n, H, k, salt=0):
    """k sources of 3 R rows, an unsorted index into them with -1 entries"""
    rng = np.random.default_rng(R * 131 + n * 17 + H + 1000 * k + salt)
    rows = 3 * R
    idx = rng.permutation(rows)[:R].astype(np.int64)
    idx[rng.random(R) < 0.25] = -1
    if R == 1:
        idx[0] = 2
    return [bf16_values(rng, (rows, H)) for _ in range(k)], idx


def scatter_inputs(R, n, H, salt=0):
    rng = np.random.default_rng(R * 37 + n * 5 + H + salt)
    rows = 3 * R
    idx = rng.permutation(rows)[:R].astype(np.int64)
    idx[rng.random(R) < 0.25] = -1
    if R == 1:
        idx[0] = 1
    return bf16_values(rng, (rows, H)), bf16_values(rng, (R, 4 * H)), idx


# ------------------------------------------------------------------ one tagger step with a layer selection
def normalize(layers, L):
    out = []
    for i in layers:
        assert -(L + 1) <= i <= L
        out.append(i + L + 1 if i < 0 else i)
    return out


def tagger_forward_loss_layers(params, cfg, batch, start, stop, x_idx, layers=(-1,), mean=False, bf16_points=False):
    """oracle.train_step.tagger_forward_loss with the token feature taken from the hidden states `layers` names (hs[0] = the embedding
    LayerNorm's output, hs[i] = layer i's): their first-sub-token rows concatenated in that order or, mean=True, averaged
    (torch.mean over the selected rows -- the reference's use_scalar_mix).  params['linear.weight'] is [T, W].  -> (loss, emissions)"""
    import torch.nn.functional as F
    from oracle import encoder as enc
    from oracle import train_step as ots
    _, hs = enc.encoder_forward(params, cfg, batch["input_ids"], batch["attention_mask"], return_all=True, bf16_points=bf16_points)
    sel = normalize(layers, cfg.num_hidden_layers)
    rows = [enc.gather_first_subtoken(hs[i], batch["first_idx"], batch.get("first_row")) for i in sel]
    pooled = torch.stack(rows, 0).mean(0) if mean else torch.cat(rows, dim=-1)
    if bf16_points:
        pooled = enc.round_bf16(pooled)
    emis = F.linear(pooled, params["linear.weight"], params["linear.bias"])
    tags, lengths = batch["tags"], batch["lengths"]
    B, n, T = emis.shape
    keep = (torch.arange(n)[None, :] < lengths[:, None])
    if x_idx is not None:
        keep = keep & (tags != x_idx)
    lens = keep.sum(1)
    nmax = int(lens.max())
    cf = emis.new_zeros(B, nmax, T)
    ct = torch.zeros(B, nmax, dtype=torch.int64)
    for b in range(B):
        idx = torch.nonzero(keep[b])[:, 0]
        cf[b, :len(idx)] = emis[b, idx]
        ct[b, :len(idx)] = tags[b, idx]
    nll = ots.crf_nll_torch(cf, ct, lens, params["transitions"], start, stop)
    return nll.mean(), emis


def tiny_setup_layers(layers=(-1,), mean=False, T=29, B=2, S=64, L=2, H=128, A=2, F_=256, V=512, seed=5, std=0.08, device="cuda"):
    """selftest.tiny_setup with the engine's layer selection: the same weights (the head's drawn for its own width), the same batch"""
    from kbner import batch as kb
    from kbner import engine
    cfg = engine.EncoderConfig(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=A, intermediate_size=F_,
                               max_position_embeddings=S + 2)
    start, stop, x_idx = 27, 28, 9
    tg = engine.Tagger(cfg, T, start, stop, device=device, layers=tuple(layers), layer_mean=mean)
    tg.init_random(seed=seed, std=std)
    b = kb.synthetic_batch(B, S, vocab=V, T=T, x_idx=x_idx, start=start, stop=stop, n_real=6, seed=seed)
    if B > 1:   # ragged, as selftest.tiny_setup makes it: the second sentence is shorter
        ids, am = b["input_ids"].copy(), b["attention_mask"].copy()
        cut = S - 9
        ids[1, cut - 1] = 2
        ids[1, cut:] = 0
        am[1, cut:] = 0
        fi = b["first_idx"].copy()
        fi[1][fi[1] >= cut - 1] = -1
        lengths = np.asarray([int((fi[r] >= 0).sum()) for r in range(B)])
        b = kb.assemble(ids, am, fi, b["tags"].copy(), lengths, x_idx)
    return cfg, tg, b, (start, stop, x_idx)
