"""GPU: element-wise and exact parity tests of the LSTM recurrence kernels (csrc/lstm.hip) -- kbner_lstm_step, the one-wave
step kernel, and kbner_lstm_seq, the four-wave split-K kernel behind the BiLSTM tagger head and every character LM -- through
the C ABI with test-owned buffers, each entry point on its own against the float64 references of tests/lstmref.py (which
tests/test_lstmref_cpu.py proves against torch.nn.LSTM).  tests/test_gpu_stack.py reaches these kernels through one relative
L2 number per emission matrix and through a cross-check of the two entry points against each other: a 16-unit x 16-sequence
tile that reads the wrong h row, a dropped 64-wide K slice of one wave or a defect the two kernels share passes there.  Here
every element of c, h and out is compared, at every hidden width and batch size at which the code takes another path
(lstmref.CASES), with non-zero h0 / c0, ragged row tables, a sequence inactive from step 0, one that never stores, several
sequences consuming one gx row, reversed odd directions and output column blocks that are not equidistant.

EXACT cases (lstmref.switchboard: saturated gates decided by the product h Whh^T): c EQUALS the reference, h and out its bf16
rounding.  REAL cases: rowref.tolerance, 8 x the float32 evaluation's worst error (lstmref.eval32), floor 2 * 2^-24 * the
first-order bound of the cell update, plus one bf16 ulp for h; several steps against the forced reference
(lstmref.seq_forced), final c with scale = steps.  The comparison is lstmref.check_case, whose power the CPU module proves.
Every buffer sits in a parent with NaN guards: rows behind gx, whh, h, c and out, columns beside gx and out, the rows of gx no
gxi names, the half of h that holds no input; after the call every row and column of out that no outi / out_col names is still
NaN, and so are the guards.  Rejected calls return EINVAL and leave every output bit-identical.

Worst figures per kernel of the MI355X run that accompanied this module (95 cases, all passing, 7 s on its own; run with -s):
`ratio` = kernel error / float32 evaluation error (of which the rule allows 8), `share` = the largest fraction of its tolerance
any element used.  For h the error IS the bf16 rounding of the output (share just below 1: half a bf16 ulp is 2^-8 relative at
the bottom of a binade) and the ratio says nothing; the final c of several steps is held to `steps` times the rule, which its
float32 chain uses little of.

    kernel (output)                  ratio   share      kernel (output)                  ratio   share
    lstm_step (c, 1 step)            1.78    0.15       lstm_seq (c, 1 step)             1.00    0.13
    lstm_step (h_t, bf16)            -       0.993      lstm_seq (c, 2 to 8 steps)       1.04    0.06
                                                        lstm_seq (h_t, bf16)             -       0.995

No kernel needed more than 1.8 of the factor 8: `__expf` costs nothing measurable against numpy's exponential in the documented
forms of sigmoid and tanh.  Every EXACT case is bit-equal, every guard intact; the tests exposed no defect in csrc/lstm.hip or
kbner/stack.py.  (kbner_lstm_seq refuses a null table even with steps = 0, as include/kbner.h says: the zero-step cases hand it
a table of one step that is never read.)
"""
import ctypes

import numpy as np
import pytest
import torch

import lstmref as R

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
GUARD = 64            # NaN elements behind every flat buffer
EINVAL = -22
WORST = {}


@pytest.fixture(scope="module")
def L():
    from kbner import lib as _L
    _L.load()
    yield _L
    print("\n[lstmk] worst per kernel (error ratio kernel / float32 evaluation, largest share of the tolerance used):")
    for k in sorted(WORST):
        print("[lstmk]   %-30s ratio %8.3f   share %6.3f" % (k, WORST[k][0], WORST[k][1]))


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def parent(a, dtype, pad_cols=0, extra_rows=0):
    """device buffer [rows + extra_rows, cols + pad_cols] of NaN holding `a` (its own NaN included) in its top-left corner"""
    a = np.asarray(a)
    full = torch.full((a.shape[0] + extra_rows, a.shape[1] + pad_cols), NAN, dtype=dtype, device=DEV)
    full[:a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)
    return full


def flat(a, dtype, copies=1):
    """flat device buffer: `a`, then (copies - 1) * a.size + GUARD elements of NaN"""
    a = np.asarray(a)
    full = torch.full((copies * a.size + GUARD,), NAN, dtype=dtype, device=DEV)
    full[:a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV).reshape(-1)
    return full


def host(t):
    return t.detach().float().cpu().numpy()


class Buffers:
    """the device buffers of one case, every one of them test-owned and guarded"""

    def __init__(self, d):
        self.d = d
        self.n = d.ndir * d.B * d.Hp
        self.gx = parent(d.gx, BF16, pad_cols=8, extra_rows=2)           # ld_gx > ndir * 4 * Hp
        self.whh = flat(d.whh, BF16)
        self.h = flat(d.h0, BF16, copies=2)                              # [2, ndir, B, Hp]: h0, then the half no input is in
        self.c = flat(d.c0, F32)
        self.out = torch.full((d.rows_out + 3, d.ldo), NAN, dtype=BF16, device=DEV)
        tab = (max(d.steps, 1), d.ndir, d.B)                             # steps = 0: a table of one step that is never read
        self.gxi = torch.full(tab, -1, dtype=I32, device=DEV)
        self.outi = torch.full(tab, -1, dtype=I32, device=DEV)
        self.gxi[:d.steps] = torch.from_numpy(np.ascontiguousarray(d.gxi)).to(DEV)
        self.outi[:d.steps] = torch.from_numpy(np.ascontiguousarray(d.outi)).to(DEV)
        self.out_col = torch.tensor(d.out_cols, dtype=I32, device=DEV)
        # what the kernels index stays inside what they were given
        assert self.gx.shape[1] % 4 == 0 and d.ldo % 4 == 0 and all(c % 4 == 0 and c + d.Hp <= d.ldo for c in d.out_cols)
        assert d.gxi.max(initial=-1) < d.rows_gx and d.outi.max(initial=-1) < d.rows_out
        assert d.gx.shape == (d.rows_gx, d.ndir * 4 * d.Hp) and d.whh.shape == (d.ndir, 4 * d.Hp, d.Hp)

    def outputs(self):
        return [self.h, self.c, self.out]

    def seq_args(self, L, **kw):
        d = self.d
        a = dict(gx=L.ptr(self.gx), ld_gx=self.gx.shape[1], gxi=L.ptr(self.gxi), whh=L.ptr(self.whh), h=L.ptr(self.h), c=L.ptr(self.c),
                 out=L.ptr(self.out), ldo=d.ldo, out_col=L.ptr(self.out_col), outi=L.ptr(self.outi), steps=d.steps, B=d.B, Hp=d.Hp,
                 ndir=d.ndir, stream=L.stream_ptr())
        a.update(kw)
        return list(a.values())

    def step_args(self, L, s, **kw):
        d, e = self.d, 2 * self.n
        hp = self.h.data_ptr()
        a = dict(gx=L.ptr(self.gx), ld_gx=self.gx.shape[1], gxi=L.ptr(self.gxi[s]), whh=L.ptr(self.whh),
                 h_in=ctypes.c_void_p(hp + (s & 1) * e), h_out=ctypes.c_void_p(hp + ((s + 1) & 1) * e), c=L.ptr(self.c),
                 out=ctypes.c_void_p(self.out.data_ptr() + 2 * d.out_cols[0]), ldo=d.ldo, out_dir_stride=d.out_dir_stride,
                 outi=L.ptr(self.outi[s]), B=d.B, Hp=d.Hp, ndir=d.ndir, stream=L.stream_ptr())
        a.update(kw)
        return list(a.values())

    def run(self, L):
        d = self.d
        if d.entry == "seq":
            L.call("kbner_lstm_seq", *self.seq_args(L))
        else:
            assert all(c == d.out_cols[0] + i * d.out_dir_stride for i, c in enumerate(d.out_cols))
            for s in range(d.steps):
                L.call("kbner_lstm_step", *self.step_args(L, s))
        torch.cuda.synchronize()

    def got(self, what):
        """what the kernels left, after asserting that every guard is as it was"""
        d, n = self.d, self.n
        assert bool(torch.isnan(self.h[2 * n:]).all()) and bool(torch.isnan(self.c[n:]).all()), what + ": wrote behind h or c"
        assert bool(torch.isnan(self.out[d.rows_out:]).all()), what + ": wrote behind out"
        assert bool(torch.isnan(self.whh[d.whh.size:]).all()) and bool(torch.isnan(self.gx[d.rows_gx:]).all())
        half = d.steps & 1
        return R.NS(h=host(self.h[half * n:(half + 1) * n]).reshape(d.ndir, d.B, d.Hp), c=host(self.c[:n]).reshape(d.ndir, d.B, d.Hp),
                    out=host(self.out[:d.rows_out]))


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).clone()


def _run_case(L, case):
    d = R.build_case(case)
    what = R.case_id(case)
    buf = Buffers(d)
    buf.run(L)
    R.check_case(d, buf.got(what), what, WORST, print)


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=R.case_id)
def test_lstm_exact(L, case):
    _run_case(L, case)


@pytest.mark.parametrize("case", R.REAL_CASES, ids=R.case_id)
def test_lstm_real(L, case):
    _run_case(L, case)


@pytest.mark.parametrize("case", R.ZERO_STEP_CASES, ids=R.case_id)
def test_lstm_seq_zero_steps_launches_nothing(L, case):
    d = R.build_case(case)
    buf = Buffers(d)
    before = [bits(t) for t in buf.outputs()]
    buf.run(L)
    assert all(torch.equal(b, bits(t)) for b, t in zip(before, buf.outputs()))
    R.check_case(d, buf.got(R.case_id(case)), R.case_id(case))               # h[0] = h0, c = c0, out all NaN


# ====================================================================== argument rejection
STEP_NAMES = ["gx", "ld_gx", "gxi", "whh", "h_in", "h_out", "c", "out", "ldo", "out_dir_stride", "outi", "B", "Hp", "ndir", "stream"]
SEQ_NAMES = ["gx", "ld_gx", "gxi", "whh", "h", "c", "out", "ldo", "out_col", "outi", "steps", "B", "Hp", "ndir", "stream"]


def _rejected(L, name, buf, args, what):
    before = [bits(t) for t in buf.outputs()]
    rc = getattr(L.load(), name)(*args)
    torch.cuda.synchronize()
    assert rc == EINVAL, (name, what, rc)
    assert all(torch.equal(b, bits(t)) for b, t in zip(before, buf.outputs())), (name, what)


def test_lstm_step_rejects_bad_arguments(L):
    buf = Buffers(R.build_case(("step", "exact", 32, 17, 1, 2)))
    good = buf.step_args(L, 0)
    ld_gx, ldo, stride = good[1], good[8], good[9]
    bad = [({n: None}, "null " + n) for n in STEP_NAMES if isinstance(good[STEP_NAMES.index(n)], ctypes.c_void_p) and n != "stream"]
    assert len(bad) == 8
    bad += [({"B": 0}, "B = 0"), ({"ndir": 0}, "ndir = 0"), ({"ld_gx": ld_gx + 2}, "ld_gx % 4"), ({"ldo": ldo + 2}, "ldo % 4"),
            ({"Hp": 48}, "Hp = 48"), ({"out_dir_stride": stride + 2}, "out_dir_stride % 4")]
    for kw, what in bad:
        _rejected(L, "kbner_lstm_step", buf, buf.step_args(L, 0, **kw), what)
    buf.run(L)                                                               # the unmodified arguments are accepted
    R.check_case(buf.d, buf.got("after the rejected calls"), "after the rejected calls")


def test_lstm_seq_rejects_bad_arguments(L):
    buf = Buffers(R.build_case(("seq", "exact", 64, 17, 1, 1)))
    good = buf.seq_args(L)
    ld_gx, ldo = good[1], good[7]
    bad = [({n: None}, "null " + n) for n in SEQ_NAMES if isinstance(good[SEQ_NAMES.index(n)], ctypes.c_void_p) and n != "stream"]
    assert len(bad) == 8
    bad += [({"B": 0}, "B = 0"), ({"ndir": 0}, "ndir = 0"), ({"ld_gx": ld_gx + 2}, "ld_gx % 4"), ({"ldo": ldo + 2}, "ldo % 4"),
            ({"Hp": 96}, "Hp = 96"), ({"steps": -1}, "steps < 0")]
    for kw, what in bad:
        _rejected(L, "kbner_lstm_seq", buf, buf.seq_args(L, **kw), what)
    buf.run(L)
    R.check_case(buf.d, buf.got("after the rejected calls"), "after the rejected calls")


def test_lstm_group_refuses_an_output_column_that_is_no_multiple_of_4(L):
    """out_col lives in device memory, the library cannot check it: kbner.stack.LSTMGroup does"""
    from kbner.stack import LSTMGroup
    d = R.build_case(("seq", "exact", 64, 17, 1, 1))
    buf = Buffers(d)
    grp = LSTMGroup([torch.zeros(4 * 64, 64)], 64, DEV)
    before = bits(buf.out)
    with pytest.raises(L.KbnerError):
        grp.run(buf.gx, buf.gxi, buf.outi, buf.out, 0, d.B, col=6)
    with pytest.raises(L.KbnerError):
        grp.run(buf.gx, buf.gxi, buf.outi, buf.out, 0, d.B, out_cols=[10])
    with pytest.raises(L.KbnerError):
        grp.run_stepwise(buf.gx, buf.gxi, buf.outi, buf.out, 0, d.B, col=6)
    torch.cuda.synchronize()
    assert torch.equal(before, bits(buf.out))
