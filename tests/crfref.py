"""TEST INFRASTRUCTURE: plain references of the linear-chain CRF operations behind csrc/crf.hip, written from the formulas in
include/kbner.h (numpy only, no kernel structure: no lanes, no padded tag width, no prefetch).  transitions[to, from];
START / STOP are tag ids anywhere in [0, T).

Every function takes a `dtype`: np.float64 is the reference, np.float32 is "the same formula in plain float32" that feeds
rowref.tolerance.  oracle/crf.py's float32 viterbi_batch / viterbi_nbest stay the bit-exact references of the tag indices
(the kernels reproduce exactly those float32 adds); this module is the float64 reference of everything smooth.

tests/test_crfref_cpu.py proves these functions against brute-force path enumeration, torch.autograd (float64) and
oracle/crf.py on the CPU; tests/test_gpu_crf_kernels.py compares the HIP kernels with them.

Also here, because both test modules need them: the input generators (real_case, tie_case), the case list of the shared
grid (GRID) with its inputs and references (grid_inputs, grid_reference) and the check that both modules apply to a set
of outputs (check_grid) -- the GPU module to what the kernels wrote, the CPU module to float32 evaluations with a defect
switched on, which the check has to refuse.
"""
import math

import numpy as np

import rowref

F64 = np.float64
NEG = -1e12
BIG = 1e11      # |value| above this: a -1e12 start / forbidden-transition score, not a finite log-domain quantity


def _sum(x, axis, dtype):
    """sum along `axis` in `dtype`; sequential in float32 (np.sum adds pairwise, a cumulative sum cannot)"""
    x = np.asarray(x, dtype=dtype)
    if dtype == F64:
        return x.sum(axis=axis)
    return np.take(np.cumsum(x, axis=axis, dtype=dtype), -1, axis=axis)


def _lse(x, axis, dtype):
    m = x.max(axis=axis, keepdims=True)
    s = _sum(np.exp(x - m), axis, dtype)
    return (np.squeeze(m, axis) + np.log(s)).astype(dtype)


def fin(x):
    """|x| where x is a finite-scale score, 0 where it is a -1e12 sentinel (or a sum containing one)"""
    a = np.abs(np.asarray(x, F64))
    return np.where(a < BIG, a, 0.0)


# ------------------------------------------------------------------ forward / gold / backward
def forward(emit, trans, lens, start, stop, dtype=F64):
    """alpha[b,0,t] = 0 at START else -1e12;  alpha[b,i+1,t] = lse_f((emit[b,i,t] + trans[t,f]) + alpha[b,i,f]);
    logz[b] = lse_t(alpha[b,lens[b],t] + trans[STOP,t]).  -> logz[B], alpha[B,n+1,T] (rows above lens[b] unspecified)"""
    e, tr = np.asarray(emit, dtype), np.asarray(trans, dtype)
    B, n, T = e.shape
    alpha = np.zeros((B, n + 1, T), dtype)
    alpha[:, 0, :] = NEG
    alpha[:, 0, start] = 0.0
    for i in range(n):
        x = (e[:, i, :, None] + tr[None, :, :]) + alpha[:, i, None, :]
        alpha[:, i + 1, :] = _lse(x, 2, dtype)
    last = alpha[np.arange(B), np.asarray(lens, np.int64), :]
    return _lse(last + tr[stop][None, :], 1, dtype), alpha


def gold(emit, trans, tags, lens, start, stop, dtype=F64):
    """gold[b] = sum_{k<len} (emit[b,k,tag_k] + trans[tag_k, tag_{k-1}]) + trans[STOP, tag_{len-1}], tag_{-1} = START"""
    e, tr = np.asarray(emit, dtype), np.asarray(trans, dtype)
    B = e.shape[0]
    out = np.zeros(B, dtype)
    for b in range(B):
        L = int(lens[b])
        tg = [int(t) for t in tags[b, :L]]
        prev = [start] + tg[:-1] if L else []
        terms = [e[b, k, tg[k]] + tr[tg[k], prev[k]] for k in range(L)]
        s = _sum(np.asarray(terms, dtype), 0, dtype) if L else dtype(0.0)
        out[b] = s + tr[stop, tg[-1] if L else start]
    return out


def backward(emit, trans, lens, start, stop, dtype=F64):
    """beta[b,len,t] = trans[STOP,t];  beta[b,i,f] = lse_t((emit[b,i,t] + trans[t,f]) + beta[b,i+1,t])  for i < len.
    -> beta[B,n+1,T] (rows above lens[b] zero): the log-sum over every continuation of a path that holds tag f at alpha-row i"""
    e, tr = np.asarray(emit, dtype), np.asarray(trans, dtype)
    B, n, T = e.shape
    beta = np.zeros((B, n + 1, T), dtype)
    for b in range(B):
        L = int(lens[b])
        beta[b, L] = tr[stop]
        for i in range(L - 1, -1, -1):
            x = (e[b, i, :, None] + tr) + beta[b, i + 1, :, None]      # [to, from]
            beta[b, i] = _lse(x, 0, dtype)
    return beta


def marginals(emit, trans, lens, start, stop, dtype=F64):
    """p[b,i,t] = exp(alpha[b,i+1,t] + beta[b,i+1,t] - logz[b]) for i < lens[b], zero at or past it.  -> [B,n,T]"""
    logz, alpha = forward(emit, trans, lens, start, stop, dtype)
    beta = backward(emit, trans, lens, start, stop, dtype)
    B, n, T = np.asarray(emit).shape
    out = np.zeros((B, n, T), dtype)
    for b in range(B):
        L = int(lens[b])
        out[b, :L] = np.exp(alpha[b, 1:L + 1] + beta[b, 1:L + 1] - logz[b])
    return out


def nll_grads(emit, trans, tags, lens, dloss, start, stop, dtype=F64):
    """gradients of sum_b dloss[b] (logz_b - gold_b):  with the pair marginals
         q[b,i,t,f] = exp(emit[b,i,t] + trans[t,f] + alpha[b,i,f] + beta[b,i+1,t] - logz[b])       (i < len)
       demit[b,i,t] = w_b (sum_f q[b,i,t,f] - [tag_i = t]);  dtrans[t,f] = sum_b w_b (sum_i q[b,i,t,f] - #gold uses of t<-f),
       row STOP also receives w_b (exp(alpha[b,len,f] + trans[STOP,f] - logz[b]) - [tag_{len-1} = f]).  -> demit[B,n,T], dtrans[T,T]"""
    e, tr = np.asarray(emit, dtype), np.asarray(trans, dtype)
    w = np.asarray(dloss, dtype)
    B, n, T = e.shape
    logz, alpha = forward(emit, trans, lens, start, stop, dtype)
    beta = backward(emit, trans, lens, start, stop, dtype)
    demit = np.zeros((B, n, T), dtype)
    dtrans = np.zeros((T, T), dtype)
    for b in range(B):
        L = int(lens[b])
        for i in range(L):
            q = np.exp(((e[b, i, :, None] + tr) + alpha[b, i, None, :]) + (beta[b, i + 1, :, None] - logz[b]))
            dtrans += w[b] * q
            demit[b, i] = w[b] * _sum(q, 1, dtype)
        dtrans[stop] += w[b] * np.exp(alpha[b, L] + tr[stop] - logz[b])
        prev = start
        for k in range(L):
            t = int(tags[b, k])
            demit[b, k, t] -= w[b]
            dtrans[t, prev] -= w[b]
            prev = t
        dtrans[stop, prev] -= w[b]
    return demit, dtrans


# ------------------------------------------------------------------ Viterbi
def viterbi(emit, trans, lens, start, stop, dtype=F64, with_scores=False):
    """v_0 = 0 at START else -1e12;  cand[t,f] = v[f] + trans[t,f];  bp[t] = FIRST maximal f;  v'[t] = cand[t,bp[t]] + emit[t]
    (in that order: in float32 this is the bit-exact specification);  terminal = v + trans[STOP,:] with the STOP and START
    entries set to -1e12, FIRST maximal index;  conf_i = max_t softmax_t(v'_i) = 1 / sum_t exp(v'_i[t] - max v'_i).
    -> tags int32[B,n] (-1 at or past lens), conf[B,n] (0 there), popped int32[B] (the tag the backtrace ends on; START for
    an empty sentence)  [, the scores v'[B,n,T]]"""
    e, tr = np.asarray(emit, dtype), np.asarray(trans, dtype)
    B, n, T = e.shape
    tags = np.full((B, n), -1, np.int32)
    conf = np.zeros((B, n), dtype)
    popped = np.full(B, start, np.int32)
    scores = np.zeros((B, n, T), dtype)
    ar = np.arange(T)
    for b in range(B):
        L = int(lens[b])
        v = np.full(T, NEG, dtype)
        v[start] = 0.0
        bps = np.zeros((L, T), np.int64)
        for i in range(L):
            cand = v[None, :] + tr
            bp = cand.argmax(axis=1)                       # numpy: the first maximal index
            v = cand[ar, bp] + e[b, i]
            bps[i] = bp
            scores[b, i] = v
            conf[b, i] = dtype(1.0) / _sum(np.exp(v - v.max()), 0, dtype)
        term = v + tr[stop]
        term[stop] = NEG
        term[start] = NEG
        best = int(term.argmax())
        for i in range(L - 1, -1, -1):
            tags[b, i] = best
            best = int(bps[i, best])
        if L:
            popped[b] = best
    return (tags, conf, popped, scores) if with_scores else (tags, conf, popped)


def tie_stats(emit, trans, lens, start, stop):
    """-> (share of the (sentence, step < len, to) cells whose maximal Viterbi candidate is attained by two or more `from`
    tags, number of sentences whose maximal terminal score is attained by two or more tags), float64"""
    e, tr = np.asarray(emit, F64), np.asarray(trans, F64)
    B, n, T = e.shape
    tied = cells = terminal = 0
    for b in range(B):
        L = int(lens[b])
        v = np.full(T, NEG)
        v[start] = 0.0
        for i in range(L):
            cand = v[None, :] + tr
            m = cand.max(axis=1)
            tied += int(((cand == m[:, None]).sum(axis=1) >= 2).sum())
            cells += T
            v = m + e[b, i]
        term = v + tr[stop]
        term[stop] = NEG
        term[start] = NEG
        terminal += int(L > 0 and (term == term.max()).sum() >= 2)
    return tied / max(cells, 1), terminal


# ------------------------------------------------------------------ input generators
def ragged_lens(rng, B, n, low=0):
    """ragged lengths that always contain n, 1 (B >= 2) and `low` = 0 (B >= 3; low = 1: no empty sentence)"""
    lens = rng.integers(1, n + 1, size=B).astype(np.int32)
    lens[0] = n
    if B >= 2:
        lens[1] = 1
    if B >= 3:
        lens[2] = low
    return lens


def real_case(rng, B, n, T, start, stop, scale, big=False):
    """Gaussian emissions (std `scale`) under oracle.crf.init_transitions; ragged lens (0 where B >= 3, 1, n); gold tags
    drawn from the ids other than START / STOP.  big: +30 / -30 on two tags, so that the max-subtraction has to work.
    -> emit f32[B,n,T], trans f32[T,T], tags i32[B,n], lens i32[B]"""
    from oracle import crf as ocrf
    trans = ocrf.init_transitions(T, start, stop, rng)
    emit = (rng.standard_normal((B, n, T)) * scale).astype(np.float32)
    valid = [t for t in range(T) if t not in (start, stop)]
    if big:
        emit[:, :, valid[len(valid) // 3]] += np.float32(30.0)
        emit[:, :, valid[-1]] -= np.float32(30.0)
    lens = ragged_lens(rng, B, n)
    tags = rng.choice(valid, size=(B, n)).astype(np.int32)
    return emit, trans, tags, lens


def tie_case(rng, B, n, T, start, stop):
    """integer emissions in [-2, 2], integer transitions in [-1, 1] with the START row and the STOP column at -1e12: every
    finite partial sum is a small integer, exact in float32, so float32 and float64 Viterbi agree and ties are everywhere.
    -> emit f32[B,n,T], trans f32[T,T], lens i32[B]"""
    emit = rng.integers(-2, 3, size=(B, n, T)).astype(np.float32)
    trans = rng.integers(-1, 2, size=(T, T)).astype(np.float32)
    trans[start, :] = NEG
    trans[:, stop] = NEG
    return emit, trans, ragged_lens(rng, B, n)


def dloss_mix(rng, B):
    """positive, zero and negative sentence weights (B = 1: one positive weight)"""
    w = rng.uniform(0.1, 1.0, size=B)
    w[1::3] = 0.0
    w[2::3] *= -1.0
    return w.astype(np.float32)


def dtrans_pattern(T):
    """the non-zero integer pattern kbner_crf_nll_bwd has to ADD its gradient to"""
    return (((np.arange(T)[:, None] * 7 + np.arange(T)[None, :] * 3) % 11) + 1).astype(np.float32)


# ------------------------------------------------------------------ the shared grid
def _placements(T):
    return {"last2": (T - 2, T - 1), "first2": (0, 1), "swapped": (1, 0), "ends": (T - 1, 0), "middle": (T // 2, T // 2 + 1)}


# (T, START / STOP placement, B, n, emission scale, +-30 outliers)
_GRID = [
    (3, "last2", 3, 7), (3, "swapped", 5, 1), (3, "ends", 1, 1),                       # one real tag: the path is forced
    (5, "first2", 16, 48), (5, "middle", 2, 130), (5, "swapped", 3, 7),
    (29, "last2", 16, 48), (29, "ends", 3, 7), (29, "first2", 5, 1),
    (31, "last2", 2, 130), (31, "middle", 16, 48),                                     # one padding lane
    (32, "last2", 16, 48), (32, "first2", 2, 130), (32, "swapped", 3, 7), (32, "ends", 1, 1), (32, "middle", 5, 1),
    (33, "last2", 3, 7), (33, "ends", 16, 48), (33, "first2", 2, 130), (33, "swapped", 5, 1), (33, "middle", 1, 1),
    (48, "last2", 3, 7), (48, "middle", 16, 48),
    (63, "swapped", 16, 48), (63, "ends", 2, 130),
    (64, "last2", 16, 48), (64, "first2", 3, 7), (64, "swapped", 2, 130), (64, "ends", 5, 1), (64, "middle", 1, 1),
]
GRID = [(T,) + _placements(T)[p] + (B, n, 2.0, False) for T, p, B, n in _GRID]
GRID += [(29, 27, 28, 3, 7, 8.0, True), (64, 17, 5, 16, 48, 8.0, True)]               # scale 8, +-30: the max-subtraction


# the tie condition is one on the inputs (tests/test_crfref_cpu.py asserts it: >= 25 % tied cells and a tied terminal for
# T >= 32); the one case whose first draw has no tied terminal takes the next generator
TIE_SALT = {"T63-s62-e0-B2-n130": 1}


def grid_id(case):
    T, start, stop, B, n, scale, big = case
    return "T%d-s%d-e%d-B%d-n%d%s" % (T, start, stop, B, n, "-big" if big else "")


def grid_inputs(case):
    T, start, stop, B, n, scale, big = case
    seed = 1000 * T + 37 * start + 11 * stop + B + n
    rng = np.random.default_rng(seed)
    emit, trans, tags, lens = real_case(rng, B, n, T, start, stop, scale, big)
    # tie inputs where a step can tie at all (at n = 1 the only finite predecessor is START), from a generator of their own
    tie_emit = tie_trans = tie_lens = None
    if n > 1:
        tie_emit, tie_trans, tie_lens = tie_case(np.random.default_rng([seed, TIE_SALT.get(grid_id(case), 0)]), B, n, T, start, stop)
    return {"T": T, "start": start, "stop": stop, "B": B, "n": n, "emit": emit, "trans": trans, "tags": tags, "lens": lens,
            "dloss": dloss_mix(rng, B), "pattern": dtrans_pattern(T), "tie_emit": tie_emit, "tie_trans": tie_trans,
            "tie_lens": tie_lens}


def _oracle_viterbi(emit, trans, lens, start, stop):
    """oracle.crf's float32 decoder: tags, conf and the popped start tag per sentence"""
    from oracle import crf as ocrf
    tags, conf = ocrf.viterbi_batch(emit, lens, trans, start, stop)
    popped = np.full(len(lens), start, np.int32)
    for b, L in enumerate(lens):
        if L:
            popped[b] = ocrf.viterbi_decode(emit[b, :L], trans, start, stop)[2]
    return tags, conf, popped


_REF_CACHE = {}


def grid_reference(case):
    """float64 reference, float32 evaluation and tolerance magnitudes of one grid case (computed once, shared, read-only)"""
    if case in _REF_CACHE:
        return _REF_CACHE[case]
    x = grid_inputs(case)
    a = (x["emit"], x["trans"])
    s = (x["start"], x["stop"])
    B, n, T = x["emit"].shape
    lens = x["lens"]
    ref = {"inputs": x}
    for name, dt in (("r64", F64), ("r32", np.float32)):
        r = {}
        r["logz"], r["alpha"] = forward(*a, lens, *s, dtype=dt)
        r["gold"] = gold(*a, x["tags"], lens, *s, dtype=dt)
        r["marg"] = marginals(*a, lens, *s, dtype=dt)
        r["demit"], r["dtrans"] = nll_grads(*a, x["tags"], lens, x["dloss"], *s, dtype=dt)
        r["dtrans"] = r["dtrans"] + x["pattern"].astype(dt)
        r["vtags"], r["conf"], r["vpopped"], r["vscores"] = viterbi(*a, lens, *s, dtype=dt, with_scores=True)
        ref[name] = r
    r64 = ref["r64"]
    beta = backward(*a, lens, *s, dtype=F64)
    # sum_abs, all from the float64 evaluation.  Log-domain outputs: the |emission| + |transition| accumulated along the scan
    step = np.abs(x["emit"].astype(F64)).max(axis=2) + fin(x["trans"]).max()                # [B,n]
    scan = np.concatenate([np.zeros((B, 1)), np.cumsum(step, axis=1)], axis=1) + fin(x["trans"]).max()   # [B,n+1]
    mag = {"alpha": np.repeat(scan[:, :, None], T, 2), "logz": scan[np.arange(B), lens] + fin(x["trans"]).max(),
           "conf": scan[:, 1:] * 2.0}
    g = np.zeros(B)
    for b in range(B):
        tg = [int(t) for t in x["tags"][b, :lens[b]]]
        prev = [s[0]] + tg
        g[b] = sum(abs(float(x["emit"][b, k, tg[k]])) + abs(float(x["trans"][tg[k], prev[k]])) for k in range(len(tg)))
        g[b] += abs(float(x["trans"][s[1], prev[-1]]))
    mag["gold"] = g
    # probabilities and gradients: |w| x the size of the exponent being cancelled, |alpha| + |beta| + |logz|
    size = fin(r64["alpha"][:, 1:]) + fin(beta[:, 1:]) + np.abs(r64["logz"])[:, None, None]   # [B,n,T]
    for b in range(B):
        size[b, lens[b]:] = 0.0
    w = np.abs(x["dloss"].astype(F64))
    mag["marg"] = size
    mag["demit"] = w[:, None, None] * (size + 1.0)
    mag["dtrans"] = float((w * (size.reshape(B, -1).max(axis=1) + np.abs(r64["logz"]) + 1.0)).sum()) + np.abs(x["pattern"].astype(F64))
    ref["mag"] = mag
    ref["oracle"] = _oracle_viterbi(*a, lens, *s)
    if x["tie_emit"] is not None:
        ref["tie_oracle"] = _oracle_viterbi(x["tie_emit"], x["tie_trans"], x["tie_lens"], *s)
        ref["tie64"] = viterbi(x["tie_emit"], x["tie_trans"], x["tie_lens"], *s, dtype=F64)
        ref["tie32"] = viterbi(x["tie_emit"], x["tie_trans"], x["tie_lens"], *s, dtype=np.float32)
    mag["tie_conf"] = 2.0 * 3.0 * (np.arange(n)[None, :] + 1.0)          # |emission| <= 2, |transition| <= 1 per step, twice
    _REF_CACHE[case] = ref
    return ref


class Stats:
    """worst figures per (kernel, output): kernel error, float32-numpy error, their ratio, share of the tolerance used"""

    def __init__(self, tag):
        self.tag, self.worst, self.cases = tag, {}, 0

    def add(self, key, case, kerr, err32, share, floor_bound=False):
        """floor_bound: the float32 evaluation came out (nearly) exact, so the tolerance is its floor 2 * 2^-24 * sum|terms| and
        the ratio to that evaluation's error says nothing; it is printed but not kept as a worst ratio"""
        ratio = kerr / err32 if err32 > 0 else (0.0 if kerr == 0 else float("inf"))
        print("[%s] %s %s: kernel_err %.3e  f32_numpy_err %.3e  ratio %.3f%s  tolerance_share %.3f"
              % (self.tag, key, case, kerr, err32, ratio, " (floor-bound)" if floor_bound else "", share))
        w = self.worst.setdefault(key, [0.0, 0.0, None, 0.0])
        w[0], w[1], w[3] = max(w[0], kerr), max(w[1], err32), max(w[3], share)
        if math.isfinite(ratio) and not floor_bound:
            w[2] = max(w[2] or 0.0, ratio)

    def table(self):
        print("\n[%s] worst per kernel output over %d cases (kernel error, float32-numpy error, ratio, share of the tolerance):" % (self.tag, self.cases))
        for k in sorted(self.worst):
            kerr, err32, ratio, share = self.worst[k]
            print("[%s]   %-22s kernel %.2e   f32 %.2e   ratio %7s   share %6.3f"
                  % (self.tag, k, kerr, err32, "-" if ratio is None else "%.3f" % ratio, share))


def check_close(stats, key, case, got, ref64, eval32, sum_abs, sel=None, scale=1.0):
    """|got - ref64| <= rowref.tolerance(ref64, eval32, sum_abs) on the elements `sel` (all of them when None)"""
    got, ref64, eval32 = np.asarray(got, F64), np.asarray(ref64, F64), np.asarray(eval32, F64)
    sum_abs = np.zeros_like(ref64) + np.asarray(sum_abs, F64)
    if sel is not None:
        got, ref64, eval32, sum_abs = got[sel], ref64[sel], eval32[sel], sum_abs[sel]
    if ref64.size == 0:
        return
    assert np.isfinite(got).all(), "%s %s: not finite" % (key, case)
    tol, err32 = rowref.tolerance(ref64, eval32, sum_abs, scale=scale)
    diff = np.abs(got - ref64)
    share = float((diff / np.maximum(tol, 1e-300)).max())
    stats.add(key, case, float(diff.max()), err32, share, floor_bound=8.0 * err32 < 2.0 * rowref.F32_EPS * float(sum_abs.max()))
    assert (diff <= tol).all(), "%s %s: worst error %.3e, tolerance share %.3f" % (key, case, float(diff.max()), share)


def check_grid(case, got, stats):
    """The assertions of the shared grid on one case's outputs `got` (numpy arrays by name):
      vtags, vconf, vpopped           kbner_crf_viterbi on the real-valued inputs
      tie_tags, tie_conf, tie_popped  kbner_crf_viterbi on the tie inputs (cases with n > 1)
      logz, gold, alpha               kbner_crf_nll_fwd
      demit, dtrans                   kbner_crf_nll_bwd (dtrans pre-filled with inputs['pattern'])
      marg                            kbner_crf_posterior"""
    ref = grid_reference(case)
    x, r64, r32, mag = ref["inputs"], ref["r64"], ref["r32"], ref["mag"]
    cid = grid_id(case)
    B, n, T = x["emit"].shape
    lens = x["lens"]
    below = np.arange(n)[None, :] < lens[:, None]                                       # [B,n]
    stats.cases += 1
    # ---- Viterbi: bit-exact tags and popped against the float32 oracle, no element excluded
    ties = x["tie_emit"] is not None
    for pre, orc, ln in (("v", ref["oracle"], lens),) + ((("tie_", ref["tie_oracle"], x["tie_lens"]),) if ties else ()):
        tags, popped = got[pre + "tags"], got[pre + "popped"]
        assert np.array_equal(tags, orc[0]), "%s %stags differ from oracle.crf.viterbi_batch" % (cid, pre)
        assert np.array_equal(popped, orc[2]), "%s %spopped differs" % (cid, pre)
        past = ~(np.arange(n)[None, :] < ln[:, None])
        assert (tags[past] == -1).all() and (got[pre + "conf"][past] == 0.0).all(), "%s %s: tags / conf past lens" % (cid, pre)
    assert np.array_equal(ref["oracle"][0], r64["vtags"]) and np.array_equal(ref["oracle"][2], r64["vpopped"])   # tie-free: fp64 agrees
    assert (got["vpopped"][lens == 0] == x["start"]).all()
    check_close(stats, "viterbi conf", cid, got["vconf"], r64["conf"], r32["conf"], mag["conf"])
    # the tie inputs are exact in float32: their confidences differ from float64 by the rounding of exp / sum only
    if ties:
        t64, t32 = ref["tie64"], ref["tie32"]
        assert np.array_equal(t64[0], ref["tie_oracle"][0]) and np.array_equal(t64[2], ref["tie_oracle"][2])
        check_close(stats, "viterbi conf (ties)", cid, got["tie_conf"], t64[1], t32[1], mag["tie_conf"])
    # ---- forward
    check_close(stats, "nll_fwd logz", cid, got["logz"], r64["logz"], r32["logz"], mag["logz"])
    check_close(stats, "nll_fwd gold", cid, got["gold"], r64["gold"], r32["gold"], mag["gold"])
    rows = np.arange(n + 1)[None, :] <= lens[:, None]                                    # alpha rows 0 .. lens[b]
    rows = np.repeat(rows[:, :, None], T, 2)
    small = np.abs(r64["alpha"]) < BIG
    check_close(stats, "nll_fwd alpha", cid, got["alpha"], r64["alpha"], r32["alpha"], mag["alpha"], sel=rows & small)
    big = rows & ~small                                                                 # -1e12 sentinels: relative, 4 float32 roundings
    assert (np.abs(got["alpha"].astype(F64)[big] - r64["alpha"][big]) <= 4 * 2.0 ** -24 * np.abs(r64["alpha"][big])).all(), cid
    a0 = np.full(T, np.float32(NEG))
    a0[x["start"]] = 0.0
    assert (got["alpha"][:, 0, :] == a0[None, :]).all(), "%s alpha row 0" % cid
    # ---- posterior and gradients
    check_close(stats, "posterior", cid, got["marg"], r64["marg"], r32["marg"], mag["marg"])
    check_close(stats, "nll_bwd demit", cid, got["demit"], r64["demit"], r32["demit"], mag["demit"])
    check_close(stats, "nll_bwd dtrans", cid, got["dtrans"], r64["dtrans"], r32["dtrans"], mag["dtrans"])
    assert (got["marg"][~below] == 0.0).all() and (got["demit"][~below] == 0.0).all(), "%s rows at or past lens" % cid
    rs = got["marg"].astype(F64).sum(axis=2)[below]
    ds = got["demit"].astype(F64).sum(axis=2)[below]
    print("[%s] %s: posterior row sums - 1 worst %.2e, demit row sums worst %.2e" % (
        stats.tag, cid, float(np.abs(rs - 1).max()) if rs.size else 0.0, float(np.abs(ds).max()) if ds.size else 0.0))
    # ---- an empty sentence
    for b in np.nonzero(lens == 0)[0]:
        tr = x["trans"].astype(F64)
        assert abs(float(got["gold"][b]) - tr[x["stop"], x["start"]]) <= 2.0 ** -23 * abs(tr[x["stop"], x["start"]]), cid
        z = _lse(r64["alpha"][b, 0] + tr[x["stop"]], 0, F64)
        assert abs(float(got["logz"][b]) - z) <= 4 * 2.0 ** -23 * max(1.0, abs(z)), cid
