"""GPU: element-wise and exact parity tests of the LSTM training kernels (csrc/lstm_train.hip: kbner_lstm_seq_train,
kbner_lstm_seq_bwd) and of kbner_sgd (csrc/optim.hip), through the C ABI with test-owned, NaN-guarded buffers, against the
float64 references of tests/lstmbwdref.py (which tests/test_lstmbwdref_cpu.py proves against torch.nn.LSTM autograd).

Training forward (REAL cases): h, c and out bit-equal to kbner_lstm_seq on the same inputs; the saved gates, c_t and hprev under
rowref.tolerance (lstmbwdref.check_saved).  Backward: the REAL cases against bwd_seq_forced, every step reading the kernel's own
dgx[nx] and carry -- the carry a step starts from is observed by running the tail of the walk (steps s .. steps - 1) on its own,
which is the same launches on the same data --, the EXACT cases (gates 0.5, c 0, small integers) bit for bit.  Shapes:
lstmbwdref.CASES (Hp 64 / 128 / 192 / 320: 1, 2, 3 and 5 K slices per wave; B 1 .. 70: every NT template and a second batch
chunk; 1 and 2 directions; 0, 1, 2, 5, 8 steps; Hp 1024 x 9 steps once).  Structure: zero dout gives dgx exactly 0, rows no step
consumes keep what they held, the carry of a finished sequence is untouched, rejected calls return EINVAL and write nothing.

Worst figures of the MI355X run that accompanied this module (66 tests, all passing, 8 s on its own; run with -s): `ratio` = kernel
error / float32 evaluation error (of which the rule allows 8), `share` = the largest fraction of its tolerance any element used.
For the bf16 outputs the error IS the rounding of the output (share just below 1) and the ratio says nothing.

    kernel (output)                    ratio   share      kernel (output)                    ratio   share
    lstm_seq_bwd (dc_carry)            1.63    0.20       lstm_seq_train (c_t)               1.39    0.15
    lstm_seq_bwd (dgx, bf16)           -       0.994      lstm_seq_train (gates, bf16)       -       0.995
    sgd (p)                            1.00    0.13       lstm_seq_train (hprev, bf16)       -       0.993
"""
import ctypes

import numpy as np
import pytest
import torch

import lstmbwdref as R
import lstmref
import rowref

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
GUARD = 64
EINVAL = -22
WORST = {}


@pytest.fixture(scope="module")
def L():
    from kbner import lib as _L
    _L.load()
    yield _L
    print("\n[lstmtk] worst per kernel (error ratio kernel / float32 evaluation, largest share of the tolerance used):")
    for k in sorted(WORST):
        print("[lstmtk]   %-34s ratio %8.3f   share %6.3f" % (k, WORST[k][0], WORST[k][1]))


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def dev2d(a, dtype, pad_cols=0, extra_rows=2):
    """device buffer [rows + extra_rows, cols + pad_cols] of NaN holding `a` (its own NaN included) in its top-left corner"""
    a = np.asarray(a)
    full = torch.full((a.shape[0] + extra_rows, a.shape[1] + pad_cols), NAN, dtype=dtype, device=DEV)
    full[:a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)
    return full


def flat(a, dtype):
    a = np.asarray(a)
    full = torch.full((a.size + GUARD,), NAN, dtype=dtype, device=DEV)
    full[:a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV).reshape(-1)
    return full


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).clone()


def tables(d):
    tab = (max(d.steps, 1), d.ndir, d.B)                                 # steps = 0: a table of one step that is never read
    gxi = torch.full(tab, -1, dtype=I32, device=DEV)
    outi = torch.full(tab, -1, dtype=I32, device=DEV)
    gxi[:d.steps] = torch.from_numpy(np.ascontiguousarray(d.gxi)).to(DEV)
    outi[:d.steps] = torch.from_numpy(np.ascontiguousarray(d.outi)).to(DEV)
    assert d.gxi.max(initial=-1) < d.rows_gx and d.outi.max(initial=-1) < d.rows_out
    assert all(c % 4 == 0 and c + d.Hp <= d.ldo for c in d.out_cols) and d.ldo % 4 == 0
    return gxi, outi, torch.tensor(d.out_cols, dtype=I32, device=DEV)


# ====================================================================== backward
class Bwd:
    """the device buffers of one backward case"""

    def __init__(self, d, dout=None, carry0=None, dgx_fill=NAN):
        self.d = d
        K = d.ndir * 4 * d.Hp
        self.n = d.ndir * d.B * d.Hp
        self.gxi, self.outi, self.out_col = tables(d)
        self.dout = dev2d(d.dout if dout is None else dout, BF16)
        self.whht = flat(np.ascontiguousarray(d.whh.transpose(0, 2, 1)), BF16)       # [ndir, Hp, 4Hp]
        self.gates = dev2d(d.gates, BF16, extra_rows=1)
        self.cs = dev2d(d.cs, F32, extra_rows=1)
        self.carry0 = d.carry0 if carry0 is None else carry0
        self.carry = flat(self.carry0, F32)
        self.dgx = torch.full((d.rows_gx + 2, K + 8), dgx_fill, dtype=BF16, device=DEV)
        self.dgx[d.rows_gx:] = NAN
        self.dgx[:, K:] = NAN
        assert d.gates.shape == (d.rows_gx, K) and d.cs.shape == (d.rows_gx, d.ndir * d.Hp) and self.dgx.shape[1] % 8 == 0

    def args(self, L, s0=0, carry_t=None, dgx_t=None, **kw):
        d = self.d
        off = 4 * s0 * d.ndir * d.B
        a = dict(dout=L.ptr(self.dout), ldo=self.dout.shape[1], out_col=L.ptr(self.out_col),
                 outi=ctypes.c_void_p(self.outi.data_ptr() + off), gxi=ctypes.c_void_p(self.gxi.data_ptr() + off), whht=L.ptr(self.whht),
                 gates=L.ptr(self.gates), cs=L.ptr(self.cs), dc_carry=L.ptr(self.carry if carry_t is None else carry_t),
                 dgx=L.ptr(self.dgx if dgx_t is None else dgx_t), ld_dgx=self.dgx.shape[1], steps=d.steps - s0, B=d.B, Hp=d.Hp, ndir=d.ndir,
                 stream=L.stream_ptr())
        a.update(kw)
        return list(a.values())

    def run(self, L):
        """-> got for lstmbwdref.check_bwd_case: the full walk, and the carry every step started from (the walk's tails)"""
        d, n = self.d, self.n
        after = [None] * d.steps + [host(self.carry[:n]).reshape(d.ndir, d.B, d.Hp)]
        for s0 in range(d.steps - 1, 0, -1):
            carry, dgx = self.carry.clone(), self.dgx.clone()
            L.call("kbner_lstm_seq_bwd", *self.args(L, s0=s0, carry_t=carry, dgx_t=dgx))
            after[s0] = host(carry[:n]).reshape(d.ndir, d.B, d.Hp)
        L.call("kbner_lstm_seq_bwd", *self.args(L))
        torch.cuda.synchronize()
        if d.steps:
            after[0] = host(self.carry[:n]).reshape(d.ndir, d.B, d.Hp)
        K = d.ndir * 4 * d.Hp
        assert bool(torch.isnan(self.carry[n:]).all()), "wrote behind dc_carry"
        assert bool(torch.isnan(self.dgx[d.rows_gx:]).all()) and bool(torch.isnan(self.dgx[:, K:]).all()), "wrote beside dgx"
        return R.NS(dgx=host(self.dgx[:d.rows_gx, :K]), carry_after=after)


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=R.case_id)
def test_bwd_exact(L, case):
    d = R.build_case(case)
    R.check_bwd_case(d, Bwd(d).run(L), R.case_id(case))


@pytest.mark.parametrize("case", R.REAL_CASES, ids=R.case_id)
def test_bwd_real(L, case):
    d = R.build_case(case)
    R.check_bwd_case(d, Bwd(d).run(L), R.case_id(case), WORST, print)


@pytest.mark.parametrize("case", R.ZERO_STEP_CASES, ids=R.case_id)
def test_bwd_zero_steps_launches_nothing(L, case):
    d = R.build_case(case)
    buf = Bwd(d)
    before = [bits(buf.carry), bits(buf.dgx)]
    got = buf.run(L)
    assert torch.equal(before[0], bits(buf.carry)) and torch.equal(before[1], bits(buf.dgx))
    R.check_bwd_case(d, got, R.case_id(case))


def test_bwd_zero_dout_gives_exactly_zero_and_unconsumed_rows_keep_what_they_held(L):
    case = ("real", 128, 33, 2, 5)
    d = R.build_case(case)
    K = d.ndir * 4 * d.Hp
    ever = (d.gxi >= 0).any(axis=0)
    carry0 = np.where(ever[:, :, None], 0.0, d.carry0)
    buf = Bwd(d, dout=np.where(np.isnan(d.dout), NAN, 0.0), carry0=carry0, dgx_fill=3.0)
    buf.run(L)
    dgx = host(buf.dgx[:d.rows_gx, :K])
    used4 = np.repeat(R._consumed(d.gxi, d.rows_gx, d.ndir), 4 * d.Hp, axis=1)
    assert used4.any() and (~used4).any()
    assert not dgx[used4].any(), "zero dout and zero carry: dgx must be exactly 0"
    assert (dgx[~used4] == 3.0).all(), "a row no step consumes was written"
    carry = host(buf.carry[:buf.n]).reshape(d.ndir, d.B, d.Hp)
    assert not carry[ever].any() and (carry[~ever] == R.CARRY_GUARD).all()


BWD_NAMES = ["dout", "ldo", "out_col", "outi", "gxi", "whht", "gates", "cs", "dc_carry", "dgx", "ld_dgx", "steps", "B", "Hp", "ndir", "stream"]


def test_bwd_rejects_bad_arguments(L):
    d = R.build_case(("exact", 64, 17, 1, 2))
    buf = Bwd(d)
    good = buf.args(L)
    ldo, ld = good[1], good[10]
    bad = [({n: None}, "null " + n) for n in BWD_NAMES if isinstance(good[BWD_NAMES.index(n)], ctypes.c_void_p) and n != "stream"]
    assert len(bad) == 9
    bad += [({"B": 0}, "B = 0"), ({"ndir": 0}, "ndir = 0"), ({"ldo": ldo + 2}, "ldo % 4"), ({"ld_dgx": ld + 4}, "ld_dgx % 8"),
            ({"ld_dgx": 4 * 64 - 8}, "ld_dgx < ndir * 4Hp"), ({"Hp": 96}, "Hp = 96"), ({"Hp": 32}, "Hp = 32"), ({"steps": -1}, "steps < 0")]
    for kw, what in bad:
        before = [bits(buf.carry), bits(buf.dgx)]
        rc = L.load().kbner_lstm_seq_bwd(*buf.args(L, **kw))
        torch.cuda.synchronize()
        assert rc == EINVAL, (what, rc)
        assert torch.equal(before[0], bits(buf.carry)) and torch.equal(before[1], bits(buf.dgx)), what
    R.check_bwd_case(d, buf.run(L), "after the rejected calls")


# ====================================================================== training forward
class Fwd:
    def __init__(self, d):
        self.d = d
        self.n = d.ndir * d.B * d.Hp
        self.gxi, self.outi, self.out_col = tables(d)
        self.gx = dev2d(d.gx, BF16, pad_cols=8)
        self.whh = flat(d.whh, BF16)
        z = np.zeros((2, d.ndir, d.B, d.Hp))
        self.h, self.c = flat(z, BF16), flat(z[0], F32)
        self.out = torch.full((d.rows_out + 3, d.ldo), NAN, dtype=BF16, device=DEV)
        self.gates = torch.full((d.rows_gx + 1, d.ndir * 4 * d.Hp), NAN, dtype=BF16, device=DEV)
        self.cs = torch.full((d.rows_gx + 1, d.ndir * d.Hp), NAN, dtype=F32, device=DEV)
        self.hprev = torch.full((d.rows_gx + 1, d.ndir * d.Hp), NAN, dtype=BF16, device=DEV)

    def seq_args(self, L):
        d = self.d
        return [L.ptr(self.gx), self.gx.shape[1], L.ptr(self.gxi), L.ptr(self.whh), L.ptr(self.h), L.ptr(self.c), L.ptr(self.out), d.ldo,
                L.ptr(self.out_col), L.ptr(self.outi), d.steps, d.B, d.Hp, d.ndir]

    def train_args(self, L, **kw):
        names = ["gx", "ld_gx", "gxi", "whh", "h", "c", "out", "ldo", "out_col", "outi", "steps", "B", "Hp", "ndir", "gates", "cs", "hprev", "stream"]
        a = dict(zip(names, self.seq_args(L) + [L.ptr(self.gates), L.ptr(self.cs), L.ptr(self.hprev), L.stream_ptr()]))
        a.update(kw)
        return list(a.values())

    def outputs(self):
        return [self.h, self.c, self.out, self.gates, self.cs, self.hprev]


TRAIN_CASES = R.REAL_CASES


@pytest.mark.parametrize("case", TRAIN_CASES, ids=R.case_id)
def test_train_forward_equals_inference_and_saves_its_state(L, case):
    d = R.build_case(case)
    what = R.case_id(case)
    inf, trn = Fwd(d), Fwd(d)
    L.call("kbner_lstm_seq", *(inf.seq_args(L) + [L.stream_ptr()]))
    L.call("kbner_lstm_seq_train", *trn.train_args(L))
    torch.cuda.synchronize()
    for name, a, b in (("h", inf.h, trn.h), ("c", inf.c, trn.c), ("out", inf.out, trn.out)):
        assert torch.equal(bits(a), bits(b)), "%s: %s differs from kbner_lstm_seq" % (what, name)
    assert bool(torch.isnan(trn.gates[d.rows_gx:]).all()) and bool(torch.isnan(trn.cs[d.rows_gx:]).all()) and bool(torch.isnan(trn.hprev[d.rows_gx:]).all())
    got = R.NS(out=host(trn.out[:d.rows_out]), gates=host(trn.gates[:d.rows_gx]), cs=host(trn.cs[:d.rows_gx]), hprev=host(trn.hprev[:d.rows_gx]))
    R.check_saved(d, got, what, WORST, print)
    # the final c is the c_t saved at every sequence's last step, bit for bit
    c = host(trn.c[:trn.n]).reshape(d.ndir, d.B, d.Hp)
    for dd in range(d.ndir):
        for b in range(d.B):
            if d.lengths[b]:
                row = d.gxi[d.lengths[b] - 1, dd, b]
                assert R._bits_equal(c[dd, b], got.cs[row, dd * d.Hp:(dd + 1) * d.Hp]), what


def test_train_forward_rejects_bad_arguments(L):
    d = R.build_case(("real", 64, 17, 2, 2))
    buf = Fwd(d)
    good = buf.train_args(L)
    names = ["gx", "ld_gx", "gxi", "whh", "h", "c", "out", "ldo", "out_col", "outi", "steps", "B", "Hp", "ndir", "gates", "cs", "hprev", "stream"]
    bad = [({n: None}, "null " + n) for n in names if isinstance(good[names.index(n)], ctypes.c_void_p) and n != "stream"]
    assert len(bad) == 11
    bad += [({"B": 0}, "B = 0"), ({"Hp": 96}, "Hp = 96"), ({"steps": -1}, "steps < 0"), ({"ld_gx": good[1] + 2}, "ld_gx % 4")]
    for kw, what in bad:
        before = [bits(t) for t in buf.outputs()]
        rc = L.load().kbner_lstm_seq_train(*buf.train_args(L, **kw))
        torch.cuda.synchronize()
        assert rc == EINVAL, (what, rc)
        assert all(torch.equal(b, bits(t)) for b, t in zip(before, buf.outputs())), what


def test_host_wrappers_run_the_kernels_and_refuse_a_table_outside_the_contract(L):
    from kbner.stack import LSTMGroup, step_tables
    d = R.build_case(("real", 64, 17, 2, 5))
    grp = LSTMGroup([torch.from_numpy(d.whh[0]), torch.from_numpy(d.whh[1])], 64, DEV)
    gx = torch.from_numpy(np.nan_to_num(d.gx)).to(BF16).to(DEV)
    out = torch.zeros((d.rows_out, 128), dtype=BF16, device=DEV)
    bad = d.gxi.copy()
    b = int(np.argmin(np.where(d.lengths > 0, d.lengths, 99)))
    assert 0 < d.lengths[b] < d.steps
    bad[d.steps - 1, 0, b] = bad[0, 0, b]
    with pytest.raises(L.KbnerError):
        grp.run_train(gx, bad, out, d.B, [0, 64])
    lengths = np.minimum(d.lengths, 5)
    tab = step_tables(lengths, 5)
    X = torch.zeros((d.B * 5, 2 * 4 * 64), dtype=BF16, device=DEV).normal_()
    out = torch.zeros((d.B * 5, 128), dtype=BF16, device=DEV)
    saved = grp.run_train(X, tab, out, d.B, [0, 64])
    ref = torch.zeros_like(out)
    t = torch.from_numpy(tab).to(DEV)
    grp.run(X, t, t, ref, 64, d.B)
    assert torch.equal(bits(out), bits(ref))
    dgx = grp.run_bwd(torch.ones_like(out), saved, grp.whh_t())
    torch.cuda.synchronize()
    live = torch.from_numpy((np.arange(5)[None, :] < lengths[:, None]).reshape(-1)).to(DEV)
    assert bool(torch.isfinite(dgx.float()).all()) and bool((dgx[~live] == 0).all()) and bool((dgx[live].float().abs().sum(1) > 0).all())


# ====================================================================== SGD
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n,n_shadow", [(4, 4), (1028, 512), (300000, 300000)])
def test_sgd(L, n, n_shadow, clip):
    rng = np.random.default_rng([n, clip])
    p = rng.standard_normal(n).astype(np.float32)
    g = (3.0 * rng.standard_normal(n)).astype(np.float32)
    lr, max_norm, gscale = 0.1, 5.0, 0.25
    gn = rowref.sqnorm(g)
    assert (np.sqrt(gn) * gscale > max_norm) == (n > 1000)          # the larger cases clip when asked to
    pd, gd = flat(p, F32), flat(g, F32)
    sh = torch.full((n + GUARD,), NAN, dtype=BF16, device=DEV)
    gsq = torch.tensor([gn], dtype=F32, device=DEV) if clip else None
    L.call("kbner_sgd", L.ptr(pd), L.ptr(gd), L.ptr(sh), n, n_shadow, lr, L.ptr(gsq), max_norm, gscale, 1, L.stream_ptr())
    torch.cuda.synchronize()
    gn32 = float(gsq[0]) if clip else None
    ref, shadow = R.sgd(p, g, lr, gn32, max_norm, gscale, n_shadow=n_shadow)
    e32 = R.sgd32(p, g, lr, gn32, max_norm, gscale)
    tol, err32 = rowref.tolerance(ref, e32, np.abs(p.astype(np.float64)) + np.abs(ref - p))
    diff = np.abs(host(pd[:n]).astype(np.float64) - ref)
    lstmref._share("sgd (p)", "n %d clip %s" % (n, clip), diff, tol, err32, False, WORST, print)
    got_p = host(pd[:n])
    assert np.array_equal(host(sh[:n_shadow]), rowref.bf16_round(got_p[:n_shadow])), "the shadow is not the bf16 rounding of p"
    assert bool(torch.isnan(sh[n_shadow:]).all()) and bool(torch.isnan(pd[n:]).all()) and bool(torch.isnan(gd[n:]).all())
    assert not host(gd[:n]).any(), "the gradient was not zeroed"
    # zero_grad = 0, no shadow: the gradient stays
    pd2, gd2 = flat(p, F32), flat(g, F32)
    L.call("kbner_sgd", L.ptr(pd2), L.ptr(gd2), None, n, 0, lr, L.ptr(gsq), max_norm, gscale, 0, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(bits(pd2[:n]), bits(pd[:n])) and np.array_equal(host(gd2[:n]), g)


def test_sgd_rejects_bad_arguments(L):
    p, g = flat(np.ones(8), F32), flat(np.ones(8), F32)
    for args, what in (((None, L.ptr(g), None, 8, 0), "null p"), ((L.ptr(p), None, None, 8, 0), "null g"), ((L.ptr(p), L.ptr(g), None, 6, 0), "n % 4"),
                       ((L.ptr(p), L.ptr(g), None, 8, 12), "n_shadow > n"), ((L.ptr(p), L.ptr(g), None, 8, 2), "n_shadow % 4")):
        before = [bits(p), bits(g)]
        rc = L.load().kbner_sgd(*args, 0.1, None, 5.0, 1.0, 1, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (what, rc)
        assert torch.equal(before[0], bits(p)) and torch.equal(before[1], bits(g)), what
