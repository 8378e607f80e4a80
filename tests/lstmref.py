"""TEST INFRASTRUCTURE: plain float64 references of the LSTM recurrence behind csrc/lstm.hip (kbner_lstm_step,
kbner_lstm_seq), written from the formulas at the top of that file and the buffer contracts in include/kbner.h (numpy only, no
kernel structure: no tiles, no waves, no K slices, no ping-pong).

    pre[q] = gx[gxi[d,b], d*4Hp + q*Hp + j] + sum_k whh[d, q*Hp + j, k] h_in[d,b,k]          (gate order i | f | g | o)
    c' = sigmoid(f) c + sigmoid(i) tanh(g) ;  h' = sigmoid(o) tanh(c')
    gxi < 0: h and c carried, nothing written to `out` ;  outi < 0: the state advances, nothing written

tests/test_lstmref_cpu.py proves these functions against torch.nn.LSTM (float64), proves the conditions of the EXACT inputs for
every case below and proves that the comparison of this module refuses eleven defective evaluations;
tests/test_gpu_lstm_kernels.py runs the two entry points on the same cases and hands what they wrote to the same comparison.

Also here, because both test modules need them: the case list, the input and row-table generators, and the comparison
(check_case).  Arrays are host float64 holding values of the storage type (bf16: gx, whh, h, out; float32: c).

Two kinds of case.
EXACT (switchboard): whh = 65536 m with m a small integer (mostly 0), every gx entry that is read an odd multiple of 128, c0 a
small integer, h0 from the values h can take, {0, +-195/256, +-247/256, +-255/256, +-1} = {0, +-bf16(tanh k), +-1}.  Every
product w h is a multiple of 256 and every partial sum far below 2^31, so float32 addition is exact in any order; every
pre-activation is an odd multiple of 128, so sigmoid is exactly 0 or 1 and tanh exactly +-1 in float32 whatever the last bits of
the exponential (it overflows to inf or underflows to 0).  c stays an integer, h = o tanh(c) with tanh of an integer far from a
bf16 rounding midpoint.  The kernel's c must EQUAL the reference, its h and out rows the reference's bf16 rounding.  More than
half of the gates are decided by the product h Whh^T and not by gx (shares in test_lstmref_cpu.py), so a wrong h row, a dropped K slice
or a wrong Whh row flips gates.  (In float64 sigmoid(+-128) differs from 0 / 1 by 3e-56; the generator rounds the reference's c
to the integer it is next to and the CPU test asserts the distance.)
REAL: Gaussian gx and c0, whh ~ U(+-3 / sqrt(Hp)), h0 = bf16(U(-1, 1)), compared under rowref.tolerance with eval32 below as the
float32 evaluation and the first-order bound of the cell update as sum_abs.  Over several steps the reference is FORCED
(seq_forced): the matrix product of step t reads the h the kernel emitted at step t - 1, so a one-ulp bf16 difference in h is
never amplified through Whh into the comparison and the tolerance stays the single-step one.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

import rowref

F64 = np.float64
NAN = float("nan")


def _f64(a):
    return np.asarray(a, dtype=F64)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


# ------------------------------------------------------------------ one step
def _gather_gx(gx, gxi, Hp):
    """-> gx rows each (d, b) consumes, [ndir, B, 4Hp] (0 where gxi < 0), and the active mask [ndir, B]"""
    ndir, B = gxi.shape
    act = gxi >= 0
    g = np.zeros((ndir, B, 4 * Hp), gx.dtype)
    for d in range(ndir):
        g[d, act[d]] = gx[gxi[d, act[d]], d * 4 * Hp:(d + 1) * 4 * Hp]
    return g, act


def step(gx, gxi, whh, h_in, c, outi, out, out_cols, h_mm=None):
    """One time step of `ndir` directions, float64.  gx [rows, >= ndir*4Hp]; gxi / outi int [ndir, B]; whh [ndir, 4Hp, Hp];
    h_in / c [ndir, B, Hp]; out [rows_out, ldo]; out_cols: first column of direction d's h inside out.  h_mm (default h_in): the
    h the matrix product reads (seq_forced passes the kernel's).
    -> h (NOT rounded; h_in where carried), c, out (a copy with the rows of this step written), written (bool, shape of out),
       act [ndir, B], pre [ndir, B, 4, Hp], sum_abs (sum |terms| of pre, same shape), sum_abs_c / sum_abs_h [ndir, B, Hp]:
       the first-order bounds of the cell update."""
    gx, whh, h_in, c = _f64(gx), _f64(whh), _f64(h_in), _f64(c)
    gxi, outi = np.asarray(gxi), np.asarray(outi)
    ndir, B, Hp = h_in.shape
    hm = h_in if h_mm is None else _f64(h_mm)
    g, act = _gather_gx(gx, gxi, Hp)
    wt = whh.transpose(0, 2, 1)
    pre = (g + hm @ wt).reshape(ndir, B, 4, Hp)
    sum_abs = (np.abs(g) + np.abs(hm) @ np.abs(wt)).reshape(ndir, B, 4, Hp)
    si, sf, tg, so = _sigmoid(pre[:, :, 0]), _sigmoid(pre[:, :, 1]), np.tanh(pre[:, :, 2]), _sigmoid(pre[:, :, 3])
    c1 = sf * c + si * tg
    h1 = so * np.tanh(c1)
    # |d sigmoid| <= 1/4, |d tanh| <= 1: an error of pre_f passes into c' times |c| / 4, of pre_i times 1/4, of pre_g times 1
    sa_c = np.abs(sf * c) + np.abs(si * tg) + np.abs(c) / 4 * sum_abs[:, :, 1] + sum_abs[:, :, 0] / 4 + sum_abs[:, :, 2]
    sa_h = sa_c + sum_abs[:, :, 3] / 4
    a3 = act[:, :, None]
    h1, c1 = np.where(a3, h1, h_in), np.where(a3, c1, c)
    out = np.array(out, dtype=F64, copy=True)
    written = np.zeros(out.shape, bool)
    for d in range(ndir):
        for b in np.nonzero(act[d] & (outi[d] >= 0))[0]:
            out[outi[d, b], out_cols[d]:out_cols[d] + Hp] = h1[d, b]
            written[outi[d, b], out_cols[d]:out_cols[d] + Hp] = True
    return NS(h=h1, c=c1, out=out, written=written, act=act, pre=pre, sum_abs=sum_abs, sum_abs_c=sa_c, sum_abs_h=sa_h)


def eval32(gx, gxi, whh, h_mm, c, h_in=None):
    """The step formula in plain float32 numpy: sequential K sum (rowref.seq_dot32), sigmoid as 1 / (1 + exp(-x)), tanh as
    1 - 2 / (exp(2x) + 1), the kernels' documented forms.  -> h' (float32, not rounded to bf16), c' (float32); carried
    sequences return h_in (default h_mm) and c."""
    f = np.float32
    gxi = np.asarray(gxi)
    whh, hm, c = np.asarray(whh, f), np.asarray(h_mm, f), np.asarray(c, f)
    hin = hm if h_in is None else np.asarray(h_in, f)
    ndir, B, Hp = hm.shape
    g, act = _gather_gx(np.asarray(gx, f), gxi, Hp)
    pre = np.stack([g[d] + rowref.seq_dot32(hm[d], whh[d]) for d in range(ndir)]).reshape(ndir, B, 4, Hp)
    one, two = f(1), f(2)
    with np.errstate(over="ignore"):
        sig = lambda x: one / (one + np.exp(-x))                 # noqa: E731
        tnh = lambda x: one - two / (np.exp(two * x) + one)      # noqa: E731
        c1 = sig(pre[:, :, 1]) * c + sig(pre[:, :, 0]) * tnh(pre[:, :, 2])
        h1 = sig(pre[:, :, 3]) * tnh(c1)
    assert c1.dtype == f and h1.dtype == f
    a3 = act[:, :, None]
    return np.where(a3, h1, hin), np.where(a3, c1, c)


# ------------------------------------------------------------------ several steps
def seq(gx, gxi, whh, h0, c0, outi, out, out_cols, round_h=False):
    """`steps` applications of step; gxi / outi int [steps, ndir, B].  round_h False: the mathematical LSTM; True: h rounded to
    bf16 (round to nearest even, rowref.bf16_round) after every step, the kernels' documented storage (the rows of `out`
    hold the rounded h too).  -> h, c, out, written, steps (the per-step results)"""
    h, c, out = _f64(h0), _f64(c0), np.array(out, dtype=F64, copy=True)
    written = np.zeros(out.shape, bool)
    res = []
    for s in range(np.asarray(gxi).shape[0]):
        r = step(gx, gxi[s], whh, h, c, outi[s], out, out_cols)
        h, c, out = r.h, r.c, r.out
        if round_h:
            h = rowref.bf16_round(h).astype(F64)
            out[r.written] = rowref.bf16_round(out[r.written]).astype(F64)
        written |= r.written
        res.append(r)
    return NS(h=h, c=c, out=out, written=written, steps=res)


def _observed(out_k, outi_s, act, h_prev, out_cols):
    """the h every sequence holds after a step as the KERNEL stored it: the out row it wrote, else what it held before"""
    h = np.array(h_prev, copy=True)
    ndir, B, Hp = h.shape
    for d in range(ndir):
        for b in np.nonzero(act[d] & (outi_s[d] >= 0))[0]:
            h[d, b] = out_k[outi_s[d, b], out_cols[d]:out_cols[d] + Hp]
    return h


def seq_forced(gx, gxi, whh, h0, c0, outi, out, out_cols, h_kernel):
    """The same recurrence, but the matrix product of step t reads the h the kernel produced at step t - 1.  h_kernel: the
    kernel's `out` matrix of a run whose tables give every step's h rows of its own (h0 at step 0; a sequence that stored
    nothing keeps the h it had).  c stays the reference's own, in float64.  Next to it runs the float32 evaluation (eval32,
    forced the same way, its c carried in float32).  -> per step: ref (a step result), h32, c32, h_seen (the kernel's h
    after the step)"""
    hk, c, c32 = _f64(h0), _f64(c0), np.asarray(c0, np.float32)
    res = []
    for s in range(np.asarray(gxi).shape[0]):
        r = step(gx, gxi[s], whh, hk, c, outi[s], out, out_cols, h_mm=hk)
        h32, c32 = eval32(gx, gxi[s], whh, hk, c32)
        hk, c = _observed(_f64(h_kernel), np.asarray(outi[s]), r.act, hk, out_cols), r.c
        res.append(NS(ref=r, h32=h32, c32=c32, h_seen=hk))
    return res


# ------------------------------------------------------------------ cases
# (entry, kind, Hp, B, ndir, steps).  Shapes: the smallest at which each path exists.
#   step: Hp 32 = one K iteration, 160 = five under `#pragma unroll 4`; B 15 / 16 / 17 / 33 / 49 = a partial, a full, a second and
#         a third sequence tile.
#   seq:  Hp 64 = only wave 0 owns a K slice, 128 / 192 = waves without one, 256 = one each, 320 / 576 = unequal numbers of slices and
#         the last slice re-requesting itself; B 16|17, 32|33, 48|49 = the NT templates, 64|65 and 70 = the second batch chunk.
# Every Hp runs with B 17 and 49, every B with Hp 64 and 320, every ndir and every step count several times per entry.
def _shapes(hps, bs):
    seen, outl = set(), []
    for hp, b in [(hp, b) for hp in hps for b in (17, 49)] + [(hp, b) for b in bs for hp in (64, 320)]:
        if (hp, b) not in seen:
            seen.add((hp, b))
            outl.append((hp, b))
    return outl


STEP_SHAPES = _shapes((32, 64, 96, 160), (1, 15, 16, 17, 33))
SEQ_SHAPES = _shapes((64, 128, 192, 256, 320, 576), (1, 16, 17, 32, 33, 48, 49, 64, 65, 70))
CASES = []
for _i, (_hp, _b) in enumerate(STEP_SHAPES):
    CASES.append(("step", "exact", _hp, _b, 1 + _i % 3, (2, 3, 5)[_i % 3]))
    CASES.append(("step", "real", _hp, _b, 1 + (_i + 1) % 3, 1))
for _i, (_hp, _b) in enumerate(SEQ_SHAPES):
    CASES.append(("seq", "exact", _hp, _b, 1 + _i % 3, (1, 2, 5, 8)[(_i // 3) % 4]))
    CASES.append(("seq", "real", _hp, _b, 1 + (_i + 1) % 3, (1, 2, 5, 8)[_i % 4]))
EXACT_CASES = [c for c in CASES if c[1] == "exact"]
REAL_CASES = [c for c in CASES if c[1] == "real"]
# kbner_lstm_seq with steps = 0 launches nothing
ZERO_STEP_CASES = [("seq", "exact", 64, 17, 2, 0), ("seq", "exact", 320, 65, 1, 0)]

H_VALUES = np.array([0.0, 195.0, 247.0, 255.0, 256.0]) / 256.0     # 0, bf16(tanh 1), bf16(tanh 2), bf16(tanh 3), 1 (|c| >= 4)
SWITCH_M = 2              # whh = 65536 m, m an integer of [-SWITCH_M, SWITCH_M]
SWITCH_TERMS = 1.4        # expected number of non-zero products per pre-activation (at the density of h0)
SWITCH_H0_DENSITY = 0.5
SWITCH_C0 = 3


def case_id(case):
    return "%s-%s-Hp%d-B%d-d%d-s%d" % case


def geometry(entry, Hp, ndir):
    """-> out_cols, ldo, out_dir_stride (None for kbner_lstm_seq).  kbner_lstm_step: equidistant blocks, stride != Hp, behind a
    column offset; kbner_lstm_seq: blocks that are NOT equidistant.  Every gap stays NaN."""
    if entry == "step":
        stride = Hp + 12
        cols = [8 + d * stride for d in range(ndir)]
    else:
        stride, cols, col = None, [], 4
        for d in range(ndir):
            cols.append(col)
            col += Hp + 8 + 12 * d
    return cols, cols[-1] + Hp + 8, stride


def tables(rng, ndir, B, steps, mute=True):
    """Row tables [steps, ndir, B] of `ndir` models over ragged sequences: lengths of [1, steps] (one of them `steps`), from
    B = 3 on one sequence inactive from step 0 and (mute) one active throughout that never stores (outi = -1).  Every model
    has its own ids: a permuted table in which several (step, sequence) pairs consume one gx row (the character-LM case).  Odd
    directions read their sequence in reversed order, as the backward direction of a packed BiLSTM does.  h of position t of
    sequence b goes to out row t * B + b: every step's h has rows of its own.
    -> gxi, outi, rows_gx, rows_out, lengths, dead, mute (indices or None)"""
    lengths = rng.integers(1, steps + 1, size=B) if steps else np.zeros(B, np.int64)
    dead = mute_b = None
    if steps:
        lengths[rng.integers(B)] = steps
    if B >= 3 and steps:
        dead, mute_b = (int(x) for x in rng.choice(B, size=2, replace=False))
        lengths[dead] = 0
        if mute:
            lengths[mute_b] = steps
        else:
            mute_b = None
        if lengths.max() < steps:
            lengths[[b for b in range(B) if b != dead][0]] = steps
    rows_gx = (2 * steps * B) // 3 + 2              # fewer rows than (step, sequence) pairs; the last one is never named
    rows_out = max(steps, 1) * B
    ids = rng.integers(0, rows_gx - 1, size=(ndir, max(steps, 1), B))
    gxi = np.full((steps, ndir, B), -1, np.int32)
    outi = np.full((steps, ndir, B), -1, np.int32)
    for s in range(steps):
        for d in range(ndir):
            for b in range(B):
                if s < lengths[b]:
                    t = s if d % 2 == 0 else lengths[b] - 1 - s
                    gxi[s, d, b] = ids[d, t, b]
                    if b != mute_b:
                        outi[s, d, b] = t * B + b
    return gxi, outi, rows_gx, rows_out, lengths, dead, mute_b


def _read_mask(gxi, rows_gx, ndir):
    """[rows_gx, ndir]: which (row, direction block) of gx some step reads"""
    m = np.zeros((rows_gx, ndir), bool)
    for d in range(ndir):
        r = gxi[:, d, :]
        m[r[r >= 0], d] = True
    return m


def switchboard(rng, ndir, B, Hp, steps, entry="seq"):
    """The generator of the EXACT cases (module docstring).  -> the inputs and the float64 result of seq(round_h=True), its c
    rounded to the integer it is next to (`c_snap`: the largest distance)."""
    gxi, outi, rows_gx, rows_out, lengths, dead, mute = tables(rng, ndir, B, steps)
    cols, ldo, stride = geometry(entry, Hp, ndir)
    pw = min(1.0, SWITCH_TERMS / (Hp * SWITCH_H0_DENSITY))
    m = rng.integers(1, SWITCH_M + 1, size=(ndir, 4 * Hp, Hp)) * rng.choice([-1, 1], size=(ndir, 4 * Hp, Hp))
    whh = 65536.0 * m * (rng.random((ndir, 4 * Hp, Hp)) < pw)
    odd = 2 * rng.integers(0, 128, size=(rows_gx, ndir * 4 * Hp)) + 1
    gx = 128.0 * odd * rng.choice([-1, 1], size=odd.shape)
    gx[~np.repeat(_read_mask(gxi, rows_gx, ndir), 4 * Hp, axis=1)] = NAN
    c0 = rng.integers(-SWITCH_C0, SWITCH_C0 + 1, size=(ndir, B, Hp)).astype(F64)
    h0 = rng.choice(H_VALUES[1:], size=(ndir, B, Hp)) * rng.choice([-1, 1], size=(ndir, B, Hp)) * (
        rng.random((ndir, B, Hp)) < SWITCH_H0_DENSITY)
    out0 = np.full((rows_out, ldo), NAN)
    ref = seq(gx, gxi, whh, h0, c0, outi, out0, cols, round_h=True)
    snap = np.rint(ref.c)
    ref.c_snap = float(np.abs(ref.c - snap).max()) if snap.size else 0.0
    ref.c = snap
    return NS(kind="exact", entry=entry, ndir=ndir, B=B, Hp=Hp, steps=steps, gx=gx, gxi=gxi, whh=whh, h0=h0, c0=c0, outi=outi,
              out0=out0, out_cols=cols, ldo=ldo, out_dir_stride=stride, rows_gx=rows_gx, rows_out=rows_out, lengths=lengths,
              dead=dead, mute=mute, ref=ref)


def real_inputs(rng, ndir, B, Hp, steps, entry="seq"):
    """The inputs of the REAL cases.  A run of several steps has no sequence that never stores: its h would not be observable
    (seq_forced); the single steps and the EXACT cases have one."""
    gxi, outi, rows_gx, rows_out, lengths, dead, mute = tables(rng, ndir, B, steps, mute=steps == 1)
    cols, ldo, stride = geometry(entry, Hp, ndir)
    k = 3.0 / np.sqrt(Hp)
    whh = rowref.bf16_round(rng.uniform(-k, k, size=(ndir, 4 * Hp, Hp))).astype(F64)
    gx = rowref.bf16_round(rng.standard_normal((rows_gx, ndir * 4 * Hp))).astype(F64)
    gx[~np.repeat(_read_mask(gxi, rows_gx, ndir), 4 * Hp, axis=1)] = NAN
    c0 = rng.standard_normal((ndir, B, Hp)).astype(np.float32).astype(F64)
    h0 = rowref.bf16_round(rng.uniform(-1, 1, size=(ndir, B, Hp))).astype(F64)
    return NS(kind="real", entry=entry, ndir=ndir, B=B, Hp=Hp, steps=steps, gx=gx, gxi=gxi, whh=whh, h0=h0, c0=c0, outi=outi,
              out0=np.full((rows_out, ldo), NAN), out_cols=cols, ldo=ldo, out_dir_stride=stride, rows_gx=rows_gx,
              rows_out=rows_out, lengths=lengths, dead=dead, mute=mute, ref=None)


@functools.lru_cache(maxsize=None)
def build_case(case):
    """the inputs (and, for an EXACT case, the reference) of a case tuple; computed once, shared, never modified"""
    entry, kind, Hp, B, ndir, steps = case
    rng = np.random.default_rng([Hp, B, ndir, steps, entry == "seq", kind == "real"])
    return (switchboard if kind == "exact" else real_inputs)(rng, ndir, B, Hp, steps, entry)


# ------------------------------------------------------------------ the comparison
def as_stored(h, c, out, written):
    """float64 results -> what a correct kernel leaves in memory: c float32, h and the written part of out bf16 (as float32
    values), the rest of out NaN"""
    o = np.full(out.shape, NAN, np.float32)
    o[written] = rowref.bf16_round(out[written])
    return NS(h=rowref.bf16_round(h), c=np.asarray(c, F64).astype(np.float32), out=o)


def check_exact(got, ref64, what=""):
    """integer-valued case: the float32 output EQUALS the float64 reference"""
    ref64 = _f64(ref64)
    ref = ref64.astype(np.float32)
    assert np.array_equal(ref.astype(F64), ref64), "%s: the reference is not a float32 value" % what
    g = np.asarray(got, np.float32).reshape(ref.shape)
    bad = np.argwhere(g != ref)
    assert bad.shape[0] == 0, "%s: %d elements differ, first at %s: got %r expected %r" % (
        what, bad.shape[0], tuple(bad[0]), g[tuple(bad[0])], ref[tuple(bad[0])])


def check_exact_bf16(got, ref64, what=""):
    """the bf16 output (given as float32 values) EQUALS the bf16 rounding of the reference"""
    check_exact(got, rowref.bf16_round(_f64(ref64)).astype(F64), what)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def _check_out_shape(got, written, what):
    nan = np.isnan(got.out)
    assert not nan[written].any(), "%s: an out row that outi names was not written (or holds NaN)" % what
    bad = np.argwhere(~nan & ~written)
    assert bad.shape[0] == 0, "%s: out written at %s, which no outi / out_col names" % (what, tuple(bad[0]))


def _check_carried(d, got, what):
    """a sequence that is never active keeps h0 and c0 bit for bit"""
    never = ~(d.gxi >= 0).any(axis=0) if d.steps else np.ones((d.ndir, d.B), bool)
    assert _same_bits(got.h[never], d.h0[never]), "%s: h of a sequence that was never active changed" % what
    assert _same_bits(got.c[never], d.c0[never]), "%s: c of a sequence that was never active changed" % what


def check_exact_case(d, got, what=""):
    """EXACT: c EQUALS the reference, h and every written out row its bf16 rounding; nothing else of out is written"""
    _check_out_shape(got, d.ref.written, what)
    check_exact(got.c, d.ref.c, what + " c")
    check_exact_bf16(got.h, d.ref.h, what + " h")
    check_exact_bf16(got.out[d.ref.written], d.ref.out[d.ref.written], what + " out")
    _check_carried(d, got, what)


def _share(kernel, what, diff, tol, err32, bf16_out, stats, log):
    kerr = float(diff.max()) if diff.size else 0.0
    share = float((diff / np.maximum(tol, 1e-300)).max()) if diff.size else 0.0
    ratio = kerr / err32 if err32 > 0 else (0.0 if kerr == 0 else float("inf"))
    if log is not None:
        log("[lstmk] %s %s: kernel_err %.3e  f32_eval_err %.3e  ratio %.3f  tolerance_share %.3f%s"
            % (kernel, what, kerr, err32, ratio, share, "  (bf16 output)" if bf16_out else ""))
    if stats is not None:
        w = stats.setdefault(kernel, [0.0, 0.0])
        if not bf16_out and np.isfinite(ratio):
            w[0] = max(w[0], ratio)
        w[1] = max(w[1], share)
    if share > 1.0:
        i = np.unravel_index(int(np.argmax(diff / np.maximum(tol, 1e-300))), diff.shape)
        raise AssertionError("%s %s: element %s off by %.3e, tolerance share %.3f" % (kernel, what, i, diff[i], share))


def check_real_case(d, got, what="", stats=None, log=None):
    """REAL: every emitted h_t against seq_forced under rowref.tolerance(ref, eval32, sum_abs_h, bf16_out=True), the single-step
    rule; the final c under the rule with sum_abs_c and scale = steps; the final h EQUALS the last out row its sequence
    emitted, bit for bit (a sequence that never stores: the final h under the h rule, single steps only)."""
    assert d.steps >= 1
    kname = "lstm_" + d.entry
    forced = seq_forced(d.gx, d.gxi, d.whh, d.h0, d.c0, d.outi, d.out0, d.out_cols, got.out)
    written = np.zeros(d.out0.shape, bool)
    for r in forced:
        written |= r.ref.written
    _check_out_shape(got, written, what)
    _check_carried(d, got, what)
    assert np.isfinite(got.h).all() and np.isfinite(got.c).all(), "%s: non-finite state" % what
    for s, r in enumerate(forced):
        emit = r.ref.act & (d.outi[s] >= 0)
        if not emit.any():
            continue
        tol, err32 = rowref.tolerance(r.ref.h[emit], r.h32[emit], r.ref.sum_abs_h[emit], bf16_out=True)
        _share(kname + " (h_t, bf16)", "%s step %d" % (what, s), np.abs(r.h_seen - r.ref.h)[emit], tol, err32, True, stats, log)
    last = forced[-1]
    ever = (d.gxi >= 0).any(axis=0)
    sa_c = np.max([r.ref.sum_abs_c for r in forced], axis=0)
    tol, err32 = rowref.tolerance(last.ref.c[ever], last.c32[ever], sa_c[ever], scale=float(d.steps))
    _share(kname + (" (c, 1 step)" if d.steps == 1 else " (c, 2 to 8 steps)"), what, np.abs(_f64(got.c) - last.ref.c)[ever], tol, err32, False, stats, log)
    emitted = ((d.gxi >= 0) & (d.outi >= 0)).any(axis=0)
    assert _same_bits(got.h[emitted], last.h_seen[emitted]), "%s: the final h is not the last h its sequence emitted" % what
    hidden = ever & ~emitted
    if hidden.any():
        assert d.steps == 1
        tol, err32 = rowref.tolerance(last.ref.h[hidden], last.h32[hidden], last.ref.sum_abs_h[hidden], bf16_out=True)
        _share(kname + " (h_t, bf16)", what + " (outi = -1)", np.abs(_f64(got.h) - last.ref.h)[hidden], tol, err32, True, stats, log)


def check_case(d, got, what="", stats=None, log=None):
    """THE comparison: what tests/test_gpu_lstm_kernels.py asserts of a kernel run and tests/test_lstmref_cpu.py of the
    defective evaluations.  got: h [ndir, B, Hp] and out [rows_out, ldo] as float32 values of the stored bf16 (NaN where
    nothing was written), c float32."""
    if d.kind == "exact":
        check_exact_case(d, got, what)
    else:
        check_real_case(d, got, what, stats, log)
