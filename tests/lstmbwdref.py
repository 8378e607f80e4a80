"""TEST INFRASTRUCTURE: plain float64 references of the LSTM training kernels (csrc/lstm_train.hip: kbner_lstm_seq_train,
kbner_lstm_seq_bwd), written from the formulas at the top of that file and in include/kbner.h (numpy only, no kernel structure),
the cases tests/test_gpu_lstm_train_kernels.py runs and the comparison it uses.  tests/test_lstmbwdref_cpu.py proves the
references against float64 torch.nn.LSTM autograd and proves that the comparison refuses ten defective evaluations.

Backward step s for an active (d, b), r = gxi[s], nx = gxi[s + 1] (-1 past the end or when finished), pv = gxi[s - 1] (-1 at 0):
    dh  = dout[outi[s]] (0 where outi < 0) + (nx >= 0 ? dgx[nx, d-block] . Whh_d : 0)
    t   = tanh(c[r]) ;  c_prev = pv >= 0 ? c[pv] : 0 ;  dc = dc_carry + dh o (1 - t^2)
    di  = dc g i (1 - i) ;  df = dc c_prev f (1 - f) ;  dg = dc i (1 - g^2) ;  do = dh t o (1 - o)
    dc_carry = dc f ;  dgx[r, d-block] = (di, df, dg, do)

Arrays are host float64 holding values of the storage type (bf16: gx, whh, gates, hprev, dout, dgx; float32: c, dc_carry).

train_fwd        the forward recurrence from h_0 = c_0 = 0 with what the kernel saves per consumed gx row
bwd_step         one backward step (float64, or the plain-float32 evaluation for rowref.tolerance with f32=True)
bwd_seq          the whole walk, every step reading the reference's own dgx and carry
bwd_seq_forced   the same, every step reading the KERNEL's dgx[nx] and the KERNEL's carry (errors do not compound, as
                 lstmref.seq_forced does for the forward), next to the float32 evaluation forced the same way
weight_grads     dWih = dgx^T X, dWhh_d = dgx_d^T hprev_d, both bias gradients = colsum(dgx)
emulate          the whole head (input GEMM .. CRF .. weight gradients) in float64 with values rounded to bf16 / float32 at
                 exactly the storage points kbner.stack.BiLSTMHead.loss_backward has (listed at the function)

Two kinds of backward case.
EXACT: gates = 0.5, c = 0 (so t = 0, do = 0, df = 0), dout in 16 * {-1, 0, 1}, whh in {0, +-1, +-2} with two non-zero entries per
column in the i and g gate blocks (and one in the f / o blocks, which multiplies zeros).  Step steps - 1: dc = dout / 2, di = dc / 8,
dg = 3 dc / 8 -- integers; the step before: dh = dout + (at most 2 * 2 * 6 = 24), dc = carry + dh / 2 a multiple of 1/2 of magnitude
<= 24, so 3 dc / 8 has a numerator below 256 and is a bf16 value.  Every product and sum is exact in float32 and bf16 in any order;
dgx and dc_carry must EQUAL the reference.  A third step multiplies by 3 / 8 again and adds terms a factor 8 apart: its values no
longer fit bf16's 8 bits, so the EXACT cases run 0, 1 and 2 steps (test_lstmbwdref_cpu.py asserts the conditions for every one);
5, 8 and 9 steps run as REAL cases.
REAL: the saved state comes from train_fwd on Gaussian gx, whh ~ U(+-3 / sqrt(Hp)); Gaussian dout and initial carry; compared
under rowref.tolerance (8 x the float32 evaluation's worst error; bf16 outputs take the bf16 term) against bwd_seq_forced.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

import lstmref
import rowref

F64 = np.float64
NAN = float("nan")
CARRY_GUARD = 7.25        # dc_carry of a sequence that is never active: must come back bit for bit


def _f64(a):
    return np.asarray(a, dtype=F64)


def _act64(pre):
    """pre [.., 4, Hp] -> post-activation gates, same shape"""
    g = np.empty_like(pre)
    g[..., 0, :], g[..., 1, :], g[..., 3, :] = lstmref._sigmoid(pre[..., 0, :]), lstmref._sigmoid(pre[..., 1, :]), lstmref._sigmoid(pre[..., 3, :])
    g[..., 2, :] = np.tanh(pre[..., 2, :])
    return g


# ------------------------------------------------------------------ forward with saved state
def train_fwd(gx, gxi, whh, outi, out0, out_cols, rows_gx=None, round_h=True, hprev_kernel=None):
    """kbner_lstm_seq_train from h_0 = c_0 = 0.  round_h: h rounded to bf16 after every step (the kernel's storage).
    hprev_kernel (what the kernel saved as hprev): the matrix product of step t reads the h row the KERNEL multiplied, so a one-ulp
    bf16 difference in h is never amplified through Whh (lstmref.seq_forced); c stays the reference's own.
    -> h, c, out, written, gates [rows, ndir*4Hp], cs / hprev [rows, ndir*Hp] (NaN where no step consumes the row; gates and cs NOT
       rounded, hprev the stored bf16), hprev64 / hprev32 / sa_h: the unrounded h_{t-1}, its float32 evaluation and bound,
       gates32 / cs32: the float32 evaluation, sa_g / sa_c: first-order bounds, step_of [rows, ndir]"""
    gx, whh = _f64(gx), _f64(whh)
    gxi, outi = np.asarray(gxi), np.asarray(outi)
    steps, ndir, B = gxi.shape
    Hp = whh.shape[2]
    rows = gx.shape[0] if rows_gx is None else rows_gx
    f = np.float32
    h, c = np.zeros((ndir, B, Hp)), np.zeros((ndir, B, Hp))
    h64, h32, sah = np.zeros((ndir, B, Hp)), np.zeros((ndir, B, Hp), f), np.zeros((ndir, B, Hp))
    c32 = np.zeros((ndir, B, Hp), f)
    out = np.array(out0, dtype=F64, copy=True)
    written = np.zeros(out.shape, bool)
    wide, narrow = (rows, ndir * 4 * Hp), (rows, ndir * Hp)
    sv = NS(gates=np.full(wide, NAN), gates32=np.full(wide, NAN), sa_g=np.full(wide, NAN), cs=np.full(narrow, NAN),
            cs32=np.full(narrow, NAN), sa_c=np.full(narrow, NAN), hprev=np.full(narrow, NAN), hprev64=np.full(narrow, NAN),
            hprev32=np.full(narrow, NAN), sa_h=np.full(narrow, NAN), step_of=np.full((rows, ndir), -1))
    for s in range(steps):
        act = gxi[s] >= 0
        h_mm = h.copy()
        if hprev_kernel is not None:
            for d in range(ndir):
                a = np.nonzero(act[d])[0]
                h_mm[d, a] = _f64(hprev_kernel)[gxi[s, d, a], d * Hp:(d + 1) * Hp]
        r = lstmref.step(gx, gxi[s], whh, h, c, outi[s], out, out_cols, h_mm=h_mm)
        g64 = _act64(r.pre)
        # the float32 evaluation of the gates, c and h (lstmref.eval32's formulas, which returns only h and c)
        gg, _ = lstmref._gather_gx(np.asarray(gx, f), gxi[s], Hp)
        pre32 = np.stack([gg[d] + rowref.seq_dot32(np.asarray(h_mm[d], f), np.asarray(whh[d], f)) for d in range(ndir)]).reshape(ndir, B, 4, Hp)
        with np.errstate(over="ignore"):
            g32 = np.empty_like(pre32)
            for q in (0, 1, 3):
                g32[:, :, q] = f(1) / (f(1) + np.exp(-pre32[:, :, q]))
            g32[:, :, 2] = f(1) - f(2) / (np.exp(f(2) * pre32[:, :, 2]) + f(1))
            c32n = np.where(act[:, :, None], g32[:, :, 1] * c32 + g32[:, :, 0] * g32[:, :, 2], c32)
            h32n = np.where(act[:, :, None], g32[:, :, 3] * (f(1) - f(2) / (np.exp(f(2) * c32n) + f(1))), h32)
        for d in range(ndir):
            a = np.nonzero(act[d])[0]
            rr = gxi[s, d, a]
            sv.gates[rr, d * 4 * Hp:(d + 1) * 4 * Hp] = g64[d, a].reshape(len(a), 4 * Hp)
            sv.gates32[rr, d * 4 * Hp:(d + 1) * 4 * Hp] = g32[d, a].reshape(len(a), 4 * Hp)
            sa = r.sum_abs[d, a].copy()
            sa[:, (0, 1, 3)] /= 4.0                                   # |d sigmoid| <= 1/4, |d tanh| <= 1
            sv.sa_g[rr, d * 4 * Hp:(d + 1) * 4 * Hp] = sa.reshape(len(a), 4 * Hp)
            sv.cs[rr, d * Hp:(d + 1) * Hp] = r.c[d, a]
            sv.cs32[rr, d * Hp:(d + 1) * Hp] = c32n[d, a]
            sv.sa_c[rr, d * Hp:(d + 1) * Hp] = r.sum_abs_c[d, a]
            sv.hprev[rr, d * Hp:(d + 1) * Hp] = h[d, a]
            sv.hprev64[rr, d * Hp:(d + 1) * Hp] = h64[d, a]
            sv.hprev32[rr, d * Hp:(d + 1) * Hp] = h32[d, a]
            sv.sa_h[rr, d * Hp:(d + 1) * Hp] = sah[d, a]
            sv.step_of[rr, d] = s
        h64, h32, sah = r.h, h32n, np.where(act[:, :, None], r.sum_abs_h, sah)
        h, c, c32, out = r.h, r.c, c32n, r.out
        if round_h:
            h = rowref.bf16_round(h).astype(F64)
            out[r.written] = rowref.bf16_round(out[r.written]).astype(F64)
        written |= r.written
    sv.h, sv.c, sv.out, sv.written = h, c, out, written
    return sv


# ------------------------------------------------------------------ backward
DEFECTS = ("no_dc_carry", "c_for_c_prev", "no_recurrent", "whh_not_transposed", "other_direction_whh", "no_1_minus_g2",
           "swap_i_f_derivatives", "finished_updated", "dout_wrong_step_reverse", "next_from_prev")


def bwd_step(d, s, dgx, carry, f32=False, defect=None):
    """One backward step of case d (fields: gxi, outi, whh, gates, cs, dout, out_cols, Hp).  dgx [rows, ndir*4Hp]: rows gxi[s + 1]
    are read; carry [ndir, B, Hp].  f32: the formula in plain float32 numpy (sequential K sum, tanh as 1 - 2 / (exp(2x) + 1)).
    -> rows: per direction the consumed rows; val: their new dgx blocks [n, 4Hp]; carry (new array; inactive entries as they
       were); sa_dgx / sa_carry: the first-order bounds (float64 only)"""
    f = np.float32 if f32 else F64
    gxi, outi, Hp = d.gxi, d.outi, d.Hp
    steps, ndir, B = gxi.shape
    K = 4 * Hp
    carry_new = np.array(carry, dtype=f, copy=True)
    rows, vals, sas, sa_carry = [], [], [], np.zeros(carry_new.shape)
    for dd in range(ndir):
        a = np.nonzero(gxi[s, dd] >= 0)[0]
        r = gxi[s, dd, a]
        nx = gxi[s + 1, dd, a] if s + 1 < steps else np.full(len(a), -1)
        pv = gxi[s - 1, dd, a] if s > 0 else np.full(len(a), -1)
        if defect == "next_from_prev":
            nx = pv
        oi = outi[s, dd, a]
        if defect == "dout_wrong_step_reverse" and dd % 2 == 1:
            oi = outi[s, 0, a]
        w = np.asarray(d.whh[dd], f)
        if defect == "other_direction_whh":
            w = np.asarray(d.whh[(dd + 1) % ndir], f)
        if defect == "whh_not_transposed":            # the [4Hp, Hp] buffer read as if it were [Hp, 4Hp]
            w = w.reshape(Hp, K).T
        rec, rec_abs = np.zeros((len(a), Hp), f), np.zeros((len(a), Hp))
        m = nx >= 0
        if m.any() and defect != "no_recurrent":
            dn = np.asarray(dgx[nx[m], dd * K:(dd + 1) * K], f)
            rec[m] = rowref.seq_dot32(dn, w.T) if f32 else dn @ w
            rec_abs[m] = np.abs(_f64(dn)) @ np.abs(_f64(w))
        dh = rec.copy()
        mo = oi >= 0
        do_rows = np.asarray(d.dout[oi[mo], d.out_cols[dd]:d.out_cols[dd] + Hp], f)
        dh[mo] = dh[mo] + do_rows
        dh_abs = rec_abs
        dh_abs[mo] += np.abs(_f64(do_rows))
        g4 = np.asarray(d.gates[r, dd * K:(dd + 1) * K], f).reshape(len(a), 4, Hp)
        ig, fg, gg, og = g4[:, 0], g4[:, 1], g4[:, 2], g4[:, 3]
        c = np.asarray(d.cs[r, dd * Hp:(dd + 1) * Hp], f)
        cp = np.zeros((len(a), Hp), f)
        mp = pv >= 0
        cp[mp] = np.asarray(d.cs[pv[mp], dd * Hp:(dd + 1) * Hp], f)
        if defect == "c_for_c_prev":
            cp = c
        one, two = f(1), f(2)
        with np.errstate(over="ignore"):
            t = (one - two / (np.exp(two * c) + one)) if f32 else np.tanh(c)
        cin = np.asarray(carry[dd, a], f)
        if defect == "no_dc_carry":
            cin = np.zeros_like(cin)
        dc = cin + dh * og * (one - t * t)
        di, df = dc * gg * ig * (one - ig), dc * cp * fg * (one - fg)
        if defect == "swap_i_f_derivatives":
            di, df = dc * gg * fg * (one - fg), dc * cp * ig * (one - ig)
        dg = dc * ig * ((one - gg * gg) if defect != "no_1_minus_g2" else one)
        do = dh * t * og * (one - og)
        carry_new[dd, a] = dc * fg
        if defect == "finished_updated":
            fin = np.nonzero(gxi[s, dd] < 0)[0]
            carry_new[dd, fin] = carry_new[dd, fin] * f(0.5)
        assert dc.dtype == f
        dc_abs = np.abs(_f64(cin)) + dh_abs * np.abs(_f64(og * (one - t * t)))
        sa = np.stack([dc_abs * np.abs(_f64(gg * ig * (one - ig))), dc_abs * np.abs(_f64(cp * fg * (one - fg))),
                       dc_abs * np.abs(_f64(ig * (one - gg * gg))), dh_abs * np.abs(_f64(t * og * (one - og)))], 1)
        sa_carry[dd, a] = dc_abs * np.abs(_f64(fg))
        rows.append(r)
        vals.append(np.stack([di, df, dg, do], 1).reshape(len(a), K))
        sas.append(sa.reshape(len(a), K))
    return NS(rows=rows, val=vals, carry=carry_new, sa_dgx=sas, sa_carry=sa_carry)


def _put(dgx, Hp, st, rnd):
    for dd, (r, v) in enumerate(zip(st.rows, st.val)):
        dgx[r, dd * 4 * Hp:(dd + 1) * 4 * Hp] = rowref.bf16_round(v) if rnd else v


def bwd_seq(d, carry0=None, dgx0=None, round_store=False, defect=None):
    """The whole backward walk, step steps - 1 first.  round_store: dgx rounded to bf16 and the carry to float32 after every step
    (what a kernel leaves in memory).  -> dgx [rows_gx, ndir*4Hp] (dgx0, default NaN, where no step consumes), carry_after: list
    of steps + 1 arrays, carry_after[s] = the carry once step s has run, carry_after[steps] = the initial one"""
    steps = d.gxi.shape[0]
    dgx = np.full((d.rows_gx, d.ndir * 4 * d.Hp), NAN) if dgx0 is None else np.array(dgx0, dtype=F64, copy=True)
    carry = _f64(d.carry0 if carry0 is None else carry0).copy()
    after = [None] * steps + [carry]
    for s in range(steps - 1, -1, -1):
        st = bwd_step(d, s, dgx, carry, defect=defect)
        _put(dgx, d.Hp, st, round_store)
        carry = st.carry.astype(np.float32).astype(F64) if round_store else st.carry
        after[s] = carry
    return NS(dgx=dgx, carry_after=after)


def bwd_seq_forced(d, dgx_kernel, carry_after_kernel):
    """Per step s: the float64 step and the float32 evaluation, both reading the kernel's dgx (rows gxi[s + 1]) and the kernel's
    carry before the step (carry_after_kernel[s + 1]).  -> list indexed by s of (ref, e32)"""
    steps = d.gxi.shape[0]
    return [(bwd_step(d, s, _f64(dgx_kernel), _f64(carry_after_kernel[s + 1])),
             bwd_step(d, s, _f64(dgx_kernel), _f64(carry_after_kernel[s + 1]), f32=True)) for s in range(steps)]


def weight_grads(X, dgx, hprev, ndir, Hp):
    """X [rows, D]; dgx [rows, ndir*4Hp] and hprev [rows, ndir*Hp] with zero rows where nothing was consumed
    -> dWih [ndir*4Hp, D], dWhh [ndir, 4Hp, Hp], db [ndir*4Hp] (the gradient of bias_ih and of bias_hh)"""
    X, dgx, hprev = _f64(X), _f64(dgx), _f64(hprev)
    dwhh = np.stack([dgx[:, d * 4 * Hp:(d + 1) * 4 * Hp].T @ hprev[:, d * Hp:(d + 1) * Hp] for d in range(ndir)])
    return dgx.T @ X, dwhh, dgx.sum(0)


# ------------------------------------------------------------------ cases
# (kind, Hp, B, ndir, steps).  Hp 64 / 128 / 192 / 320: 1, 2, 3 and 5 K slices per wave at K = 4Hp (the forward's K = Hp: only wave 0,
# waves without a slice, unequal numbers); B 1 / 16 / 17 / 33 / 65 / 70: 1, 2 and 4 sequence tiles (NT = 1, 2, 3 at B 33 -> 48, 4) and two
# batch chunks; every Hp with B 17 and 33, every B with Hp 64 and 320.
def _shapes():
    seen, out = set(), []
    for hp, b in [(hp, b) for hp in (64, 128, 192, 320) for b in (17, 33)] + [(hp, b) for b in (1, 16, 17, 33, 65, 70) for hp in (64, 320)]:
        if (hp, b) not in seen:
            seen.add((hp, b))
            out.append((hp, b))
    return out


SHAPES = _shapes()
REAL_CASES = [("real", hp, b, 1 + (i + 1) % 2, (1, 2, 5, 8)[i % 4]) for i, (hp, b) in enumerate(SHAPES)] + [("real", 1024, 4, 2, 9), ("real", 128, 48, 2, 2)]
EXACT_CASES = [("exact", hp, b, 1 + i % 2, (2, 1, 2)[i % 3]) for i, (hp, b) in enumerate(SHAPES)] + [("exact", 128, 48, 2, 2)]
ZERO_STEP_CASES = [("exact", 64, 17, 2, 0), ("exact", 320, 65, 1, 0)]
CASES = REAL_CASES + EXACT_CASES


def case_id(case):
    return "%s-Hp%d-B%d-d%d-s%d" % case


def tables(rng, ndir, B, steps):
    """Prefix-active, ragged, permuted row tables [steps, ndir, B]: sequence b is active for steps 0 .. len_b - 1 (lengths of
    [1, steps], one of them `steps`; from B = 3 on one sequence never active and one that never stores, outi = -1); every
    (direction, position, sequence) has a gx row of its own in a random order, a third of the rows is consumed by no step; odd
    directions walk their sequence backwards; the h of position t of sequence b belongs to out row t * B + b.
    -> gxi, outi, rows_gx, rows_out, lengths, dead, mute"""
    lengths = rng.integers(1, steps + 1, size=B) if steps else np.zeros(B, np.int64)
    dead = mute = None
    if steps:
        lengths[rng.integers(B)] = steps
    if B >= 3 and steps:
        dead, mute = (int(x) for x in rng.choice(B, size=2, replace=False))
        lengths[dead], lengths[mute] = 0, steps
    rows_gx = (3 * max(steps, 1) * B) // 2 + 2
    rows_out = max(steps, 1) * B
    gxi = np.full((steps, ndir, B), -1, np.int32)
    outi = np.full((steps, ndir, B), -1, np.int32)
    for dd in range(ndir):
        ids = rng.permutation(rows_gx)[:max(steps, 1) * B].reshape(max(steps, 1), B)
        for s in range(steps):
            for b in range(B):
                if s < lengths[b]:
                    t = s if dd % 2 == 0 else lengths[b] - 1 - s
                    gxi[s, dd, b] = ids[t, b]
                    if b != mute:
                        outi[s, dd, b] = t * B + b
    return gxi, outi, rows_gx, rows_out, lengths, dead, mute


def _consumed(gxi, rows_gx, ndir):
    m = np.zeros((rows_gx, ndir), bool)
    for dd in range(ndir):
        r = gxi[:, dd]
        m[r[r >= 0], dd] = True
    return m


def _geometry(Hp, ndir):
    cols = [4 + dd * (Hp + 12) for dd in range(ndir)]
    return cols, cols[-1] + Hp + 8


def _dout(rng, d, values):
    """dout [rows_out, ldo]: `values(shape)` where some step reads it, NaN elsewhere"""
    dout = np.full((d.rows_out, d.ldo), NAN)
    for dd in range(d.ndir):
        r = d.outi[:, dd]
        r = r[r >= 0]
        dout[r, d.out_cols[dd]:d.out_cols[dd] + d.Hp] = values((len(r), d.Hp))
    return dout


def _carry0(d, values):
    ever = (d.gxi >= 0).any(axis=0) if d.steps else np.zeros((d.ndir, d.B), bool)
    c0 = np.full((d.ndir, d.B, d.Hp), CARRY_GUARD)
    c0[ever] = values((int(ever.sum()), d.Hp))
    return c0


@functools.lru_cache(maxsize=None)
def build_case(case):
    """the inputs of a case tuple (and the reference walk of an EXACT case); computed once, shared, never modified"""
    kind, Hp, B, ndir, steps = case
    rng = np.random.default_rng([Hp, B, ndir, steps, kind == "real"])
    gxi, outi, rows_gx, rows_out, lengths, dead, mute = tables(rng, ndir, B, steps)
    cols, ldo = _geometry(Hp, ndir)
    d = NS(kind=kind, Hp=Hp, B=B, ndir=ndir, steps=steps, gxi=gxi, outi=outi, rows_gx=rows_gx, rows_out=rows_out, lengths=lengths,
           dead=dead, mute=mute, out_cols=cols, ldo=ldo)
    used = np.repeat(_consumed(gxi, rows_gx, ndir), Hp, axis=1)
    used4 = np.repeat(_consumed(gxi, rows_gx, ndir), 4 * Hp, axis=1)
    if kind == "exact":
        whh = np.zeros((ndir, 4 * Hp, Hp))
        for dd in range(ndir):
            for j in range(Hp):
                ki = rng.integers(0, Hp)
                kg = 2 * Hp + rng.integers(0, Hp)
                kz = (Hp, 3 * Hp)[rng.integers(2)] + rng.integers(0, Hp)
                for k in (ki, kg, kz):
                    whh[dd, k, j] = rng.choice([-2, -1, 1, 2])
        d.whh = whh
        d.gates = np.where(used4, 0.5, NAN)
        d.cs = np.where(used, 0.0, NAN)
        d.dout = _dout(rng, d, lambda sh: 16.0 * rng.integers(-1, 2, size=sh))
        d.carry0 = _carry0(d, lambda sh: np.zeros(sh))
        d.ref = bwd_seq(d)
        return d
    k = 3.0 / np.sqrt(Hp)
    d.whh = rowref.bf16_round(rng.uniform(-k, k, size=(ndir, 4 * Hp, Hp))).astype(F64)
    gx = rowref.bf16_round(rng.standard_normal((rows_gx, ndir * 4 * Hp))).astype(F64)
    gx[~used4] = NAN
    d.gx = gx
    d.out0 = np.full((rows_out, ldo), NAN)
    d.fwd = train_fwd(gx, gxi, d.whh, outi, d.out0, cols)
    d.gates = rowref.bf16_round(d.fwd.gates).astype(F64)
    d.cs = d.fwd.cs.astype(np.float32).astype(F64)
    d.dout = _dout(rng, d, lambda sh: rowref.bf16_round(rng.standard_normal(sh)).astype(F64))
    d.carry0 = _carry0(d, lambda sh: rng.standard_normal(sh).astype(np.float32).astype(F64))
    d.ref = None
    return d


# ------------------------------------------------------------------ the comparison
def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def as_stored(res):
    """a float64 walk -> what a correct kernel leaves in memory (dgx bf16, carries float32), as float32 values"""
    return NS(dgx=np.where(np.isnan(res.dgx), np.float32(NAN), rowref.bf16_round(np.nan_to_num(res.dgx))),
              carry_after=[np.asarray(c, F64).astype(np.float32) for c in res.carry_after])


def check_bwd_case(d, got, what="", stats=None, log=None, dgx0=None):
    """THE comparison of a backward run.  got.dgx [rows_gx, ndir*4Hp] (float32 values of the stored bf16), got.carry_after: list of
    steps + 1 float32 arrays (carry_after[s]: dc_carry once step s has run; [steps]: the initial one).  dgx0: what dgx held before
    the call (default NaN everywhere)."""
    steps, Hp, K = d.steps, d.Hp, 4 * d.Hp
    used4 = np.repeat(_consumed(d.gxi, d.rows_gx, d.ndir), K, axis=1)
    if dgx0 is None:
        assert np.isnan(got.dgx[~used4]).all(), "%s: a dgx row that no step consumes was written" % what
    else:
        assert _bits_equal(got.dgx[~used4], np.asarray(dgx0)[~used4]), "%s: a dgx row that no step consumes was written" % what
    assert np.isfinite(got.dgx[used4]).all(), "%s: a consumed dgx row was not written (or is not finite)" % what
    assert _bits_equal(got.carry_after[steps], d.carry0), "%s: the initial carry is not the case's" % what
    for s in range(steps - 1, -1, -1):
        fin = d.gxi[s] < 0
        assert _bits_equal(got.carry_after[s][fin], got.carry_after[s + 1][fin]), "%s step %d: the carry of a finished sequence changed" % (what, s)
    if d.kind == "exact":
        ref = as_stored(d.ref)
        assert np.array_equal(ref.dgx[used4].astype(F64), d.ref.dgx[used4]), "%s: the reference is not a bf16 value" % what
        bad = np.argwhere((got.dgx != ref.dgx) & used4)
        assert bad.shape[0] == 0, "%s: %d dgx elements differ, first at %s: got %r expected %r" % (
            what, bad.shape[0], tuple(bad[0]), got.dgx[tuple(bad[0])], ref.dgx[tuple(bad[0])])
        for s in range(steps):
            lstmref.check_exact(got.carry_after[s], d.ref.carry_after[s], "%s carry after step %d" % (what, s))
        return
    forced = bwd_seq_forced(d, got.dgx, got.carry_after)
    for s in range(steps - 1, -1, -1):
        ref, e32 = forced[s]
        for dd in range(d.ndir):
            r = ref.rows[dd]
            if not len(r):
                continue
            tol, err32 = rowref.tolerance(ref.val[dd], e32.val[dd], ref.sa_dgx[dd], bf16_out=True)
            lstmref._share("lstm_seq_bwd (dgx, bf16)", "%s step %d dir %d" % (what, s, dd),
                           np.abs(_f64(got.dgx[r, dd * K:(dd + 1) * K]) - ref.val[dd]), tol, err32, True, stats, log)
        act = d.gxi[s] >= 0
        if act.any():
            tol, err32 = rowref.tolerance(ref.carry[act], e32.carry[act], ref.sa_carry[act])
            lstmref._share("lstm_seq_bwd (dc_carry)", "%s step %d" % (what, s), np.abs(_f64(got.carry_after[s]) - ref.carry)[act], tol,
                           err32, False, stats, log)


def check_saved(d, got, what="", stats=None, log=None):
    """What kbner_lstm_seq_train saved, REAL case d.  got: out [rows_out, ldo], gates [rows_gx, ndir*4Hp], cs, hprev [rows_gx, ndir*Hp]
    (float32 values, NaN where nothing was written).  Gates under rowref.tolerance with the bf16 term, c_t with scale = step + 1
    (the reference's c chain is its own); hprev is 0 at step 0, EQUAL to the out row the sequence stored one step earlier, and
    under the h rule of lstmref (bf16 term) for every sequence, the one that never stores included."""
    Hp, K = d.Hp, 4 * d.Hp
    fw = train_fwd(d.gx, d.gxi, d.whh, d.outi, d.out0, d.out_cols, hprev_kernel=got.hprev)
    used = np.repeat(_consumed(d.gxi, d.rows_gx, d.ndir), Hp, axis=1)
    used4 = np.repeat(_consumed(d.gxi, d.rows_gx, d.ndir), K, axis=1)
    for name, g, u in (("gates", got.gates, used4), ("cs", got.cs, used), ("hprev", got.hprev, used)):
        assert np.isnan(g[~u]).all(), "%s: %s written at a row no step consumes" % (what, name)
        assert np.isfinite(g[u]).all(), "%s: %s of a consumed row not written" % (what, name)
    for s in range(d.steps):
        for dd in range(d.ndir):
            a = np.nonzero(d.gxi[s, dd] >= 0)[0]
            hp = got.hprev[d.gxi[s, dd, a], dd * Hp:(dd + 1) * Hp]
            if s == 0:
                assert not hp.any(), "%s: hprev of step 0 is not h_0 = 0" % what
                continue
            st = a[d.outi[s - 1, dd, a] >= 0]
            seen = got.out[d.outi[s - 1, dd, st], d.out_cols[dd]:d.out_cols[dd] + Hp]
            assert _bits_equal(got.hprev[d.gxi[s, dd, st], dd * Hp:(dd + 1) * Hp], seen), "%s step %d: hprev is not the h the sequence emitted" % (what, s)
    later = np.repeat(fw.step_of >= 1, Hp, axis=1)
    if later.any():
        tol, err32 = rowref.tolerance(fw.hprev64[later], fw.hprev32[later], fw.sa_h[later], bf16_out=True)
        lstmref._share("lstm_seq_train (hprev, bf16)", what, np.abs(_f64(got.hprev) - fw.hprev64)[later], tol, err32, True, stats, log)
    tol, err32 = rowref.tolerance(fw.gates[used4], fw.gates32[used4], fw.sa_g[used4], bf16_out=True)
    lstmref._share("lstm_seq_train (gates, bf16)", what, np.abs(_f64(got.gates) - fw.gates)[used4], tol, err32, True, stats, log)
    for s in range(d.steps):
        m = np.repeat(fw.step_of == s, Hp, axis=1)
        if m.any():
            tol, err32 = rowref.tolerance(fw.cs[m], fw.cs32[m], fw.sa_c[m], scale=float(s + 1))
            lstmref._share("lstm_seq_train (c_t)", "%s step %d" % (what, s), np.abs(_f64(got.cs) - fw.cs)[m], tol, err32, False, stats, log)


# ------------------------------------------------------------------ SGD
def sgd(p, g, lr, gnorm_sq=None, max_norm=5.0, grad_scale=1.0, n_shadow=None):
    """kbner_sgd in float64: p -= lr * clip * grad_scale * g, the clip rule of rowref.adamw_hf.  -> p, shadow (bf16 of float32(p))"""
    gs = float(grad_scale)
    if gnorm_sq is not None:
        coef = max_norm / (np.sqrt(float(gnorm_sq)) * grad_scale + 1e-6)
        if coef < 1.0:
            gs *= coef
    p = _f64(p) - lr * (_f64(g) * gs)
    return p, (None if n_shadow is None else rowref.bf16_round(p.astype(np.float32)[:n_shadow]))


def sgd32(p, g, lr, gnorm_sq=None, max_norm=5.0, grad_scale=1.0):
    """the same in plain float32"""
    f = np.float32
    gs = f(grad_scale)
    if gnorm_sq is not None:
        coef = f(max_norm) / (np.sqrt(f(gnorm_sq)) * f(grad_scale) + f(1e-6))
        if coef < 1.0:
            gs = gs * coef
    return np.asarray(p, f) - f(lr) * (np.asarray(g, f) * gs)


# ------------------------------------------------------------------ the whole head
def head_reference64(x, lengths, tags, st, start, stop, weights=None, post_mask=None):
    """float64 autograd of the reference's head: torch.nn.LSTM (packed, bidirectional) -> [post_mask *] -> linear -> CRF NLL
    (oracle.train_step.crf_nll_torch), sum_b weights[b] * nll_b (default 1 / B).  x [B, n, D]; st: the reference-layout state dict.
    -> loss (float), grads {name: float64 array} named as kbner.stack.BiLSTMHead.state() names them, emissions [B, n, T]"""
    import torch
    from oracle.train_step import crf_nll_torch
    B, n, D = x.shape
    H = st["rnn"]["weight_hh_l0"].shape[1]
    rnn = torch.nn.LSTM(D, H, 1, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for k, p in rnn.named_parameters():
            p.copy_(torch.as_tensor(np.asarray(st["rnn"][k], F64)))
    lw = torch.tensor(np.asarray(st["linear.weight"], F64), requires_grad=True)
    lb = torch.tensor(np.asarray(st["linear.bias"], F64), requires_grad=True)
    tr = torch.tensor(np.asarray(st["transitions"], F64), requires_grad=True)
    lens = torch.as_tensor(np.asarray(lengths))
    packed = torch.nn.utils.rnn.pack_padded_sequence(torch.from_numpy(_f64(x)), lens, batch_first=True, enforce_sorted=False)
    y, _ = rnn(packed)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=n)
    if post_mask is not None:
        y = y * torch.from_numpy(_f64(post_mask))
    em = y @ lw.t() + lb
    nll = crf_nll_torch(em, torch.as_tensor(np.asarray(tags)), lens, tr, start, stop)
    w = torch.full((B,), 1.0 / B, dtype=torch.float64) if weights is None else torch.as_tensor(_f64(weights))
    loss = (nll * w).sum()
    loss.backward()
    grads = {"rnn." + k: p.grad.numpy() for k, p in rnn.named_parameters()}
    grads.update({"linear.weight": lw.grad.numpy(), "linear.bias": lb.grad.numpy(), "transitions": tr.grad.numpy()})
    return float(loss.detach()), grads, em.detach().numpy()


def emulate(x, lengths, tags, st, start, stop, weights=None):
    """The same computation in float64 with values rounded at exactly the storage points of BiLSTMHead.loss_backward (dropout off):
      forward   X bf16 (given) ; Wih, Whh bf16 (the shadow) ; gx = bf16(X Wih^T + float32(bias_ih + bias_hh)) ; h_t bf16 after every
                step (the state and the `out` rows) ; c_t float32 ; emissions float32 (linear.* stay float32)
      backward  d emissions float32 ; d out = bf16(d emissions . linear.weight) ; the saved gates bf16 and c_t float32 ; dgx bf16
                after every step, dc_carry float32 ; the weight gradients are float32 sums over bf16 dgx, X and hprev
    (the CRF runs in float64: its float32 kernels have parity tests of their own).  Sums run in numpy's order, not the kernels'.
    -> loss, grads as head_reference64"""
    import torch
    from oracle.train_step import crf_nll_torch
    x = _f64(x)
    B, n, D = x.shape
    H = st["rnn"]["weight_hh_l0"].shape[1]
    bf = lambda a: rowref.bf16_round(_f64(a)).astype(F64)                      # noqa: E731
    f32 = lambda a: _f64(a).astype(np.float32).astype(F64)                     # noqa: E731
    sfx = ("", "_reverse")
    X = x.reshape(B * n, D)
    wih = [bf(st["rnn"]["weight_ih_l0" + s]) for s in sfx]
    whh = np.stack([bf(st["rnn"]["weight_hh_l0" + s]) for s in sfx])
    gx = bf(np.concatenate([X @ wih[d].T + f32(_f64(st["rnn"]["bias_ih_l0" + s]) + _f64(st["rnn"]["bias_hh_l0" + s]))
                            for d, s in enumerate(sfx)], 1))
    lengths = np.asarray(lengths)
    steps = int(lengths.max())
    s_ = np.arange(steps)[:, None]
    live = s_ < lengths[None, :]
    base = (np.arange(B) * n)[None, :]
    tab = np.stack([np.where(live, base + s_, -1), np.where(live, base + (lengths[None, :] - 1 - s_), -1)], 1).astype(np.int32)
    fw = train_fwd(gx, tab, whh, tab, np.zeros((B * n, 2 * H)), [0, H], round_h=True)
    lw, lb = _f64(st["linear.weight"]), _f64(st["linear.bias"])
    em = torch.tensor(f32(fw.out @ lw.T + lb).reshape(B, n, -1), requires_grad=True)
    tr = torch.tensor(_f64(st["transitions"]), requires_grad=True)
    nll = crf_nll_torch(em, torch.as_tensor(np.asarray(tags)), torch.as_tensor(lengths), tr, start, stop)
    w = torch.full((B,), 1.0 / B, dtype=torch.float64) if weights is None else torch.as_tensor(_f64(weights))
    loss = (nll * w).sum()
    loss.backward()
    dem = f32(em.grad.numpy().reshape(B * n, -1))
    d = NS(gxi=tab, outi=tab, whh=whh, gates=bf(fw.gates), cs=f32(fw.cs), dout=bf(dem @ lw), out_cols=[0, H], Hp=H, ndir=2, rows_gx=B * n,
           carry0=np.zeros((2, B, H)))
    dgx = np.nan_to_num(bwd_seq(d, round_store=True).dgx)
    dwih, dwhh, db = weight_grads(X, dgx, np.nan_to_num(fw.hprev), 2, H)
    grads = {"linear.weight": f32(dem.T @ fw.out), "linear.bias": f32(dem.sum(0)), "transitions": f32(tr.grad.numpy())}
    for dd, s in enumerate(sfx):
        blk = slice(dd * 4 * H, (dd + 1) * 4 * H)
        grads["rnn.weight_ih_l0" + s], grads["rnn.weight_hh_l0" + s] = f32(dwih[blk]), f32(dwhh[dd])
        grads["rnn.bias_ih_l0" + s] = grads["rnn.bias_hh_l0" + s] = f32(db[blk])
    return float(loss.detach()), grads
