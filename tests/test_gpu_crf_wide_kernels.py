"""GPU: direct parity tests of the wide CRF kernels (csrc/crf_wide.hip: kbner_crf_wide_viterbi, _nll_fwd, _nll_bwd, _posterior), each
through the C ABI with test-owned, NaN-filled, guarded buffers, the way tests/test_gpu_crf_kernels.py tests the single-wave kernels.

  - every case of tests/crfwide_cases.WIDE (T in {65, 96, 127, 128, 129, 137, 160, 191, 192}: wave boundaries, the backward kernel's
    <128> | <192> switch, the limit) through crfref.check_grid, unchanged: Viterbi tags and popped equal oracle.crf's float32 decoder
    bit for bit on Gaussian and on tie inputs (tests/test_crfwide_cpu.py asserts that those tie), every smooth output is compared with
    the float64 reference under rowref.tolerance.  No new tolerance;
  - crfref.GRID cases at T = 3, 29, 33, 64 through the WIDE entry points, same check, and Viterbi tags / popped equal to what the
    single-wave kernels write from the same device buffers;
  - n is bounded by the workspace, not by LDS: T = 192, B = 2, n = 300 (the single-wave design would need 288 000 B of LDS);
  - kbner_crf_wide_viterbi_ws_bytes is monotone in each argument and nothing is written behind it;
  - rejected arguments return -22 and write nothing.

The module prints the crfref.Stats table (run with -s).  Worst figures of the MI355X run that accompanied this module are in
DESIGN.md section 3.
"""
import ctypes

import numpy as np
import pytest
import torch

import crfref
import crfwide_cases

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
DEV = "cuda"
GUARD = 96            # elements behind every output buffer that no kernel may touch
ISENT = -7777         # int sentinel
EINVAL = -22
STATS = crfref.Stats("crfw")


@pytest.fixture(scope="module")
def lib():
    from kbner import lib as L
    yield L.load()
    STATS.table()


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


class Out:
    """a test-owned output buffer: `shape` elements pre-filled with NaN (float) / ISENT (int) or with `init`, GUARD more behind"""

    def __init__(self, shape, dtype=F32, init=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.size = int(np.prod(self.shape)) if len(self.shape) else 1
        self.fill = float("nan") if dtype == F32 else ISENT
        self.full = torch.full((self.size + GUARD,), self.fill, dtype=dtype, device=DEV)
        if init is not None:
            self.full[:self.size] = dev(init, np.float32 if dtype == F32 else np.int32).reshape(-1)
        self.ptr = P(self.full)

    def _untouched(self, part):
        return bool(torch.isnan(part).all()) if self.dtype == F32 else bool((part == ISENT).all())

    def get(self):
        """the written part as numpy, after asserting that the guard behind it is as it was"""
        assert self._untouched(self.full[self.size:]), "wrote behind the buffer"
        return self.full[:self.size].cpu().numpy().reshape(self.shape)

    def untouched(self):
        return self._untouched(self.full)


def no_sentinel(a):
    return not np.isnan(a).any() if a.dtype.kind == "f" else not (a == ISENT).any()


WS_FILL = 0x5A
WS_GUARD = 4096       # bytes behind kbner_crf_wide_viterbi_ws_bytes that must stay as they were


class Workspace:
    def __init__(self, lib, B, n, T):
        self.bytes = int(lib.kbner_crf_wide_viterbi_ws_bytes(B, n, T))
        self.full = torch.full((self.bytes + WS_GUARD,), WS_FILL, dtype=torch.uint8, device=DEV)
        assert self.full.data_ptr() % 16 == 0
        self.ptr = P(self.full)

    def guard_intact(self):
        return bool((self.full[self.bytes:] == WS_FILL).all())

    def untouched(self):
        return bool((self.full == WS_FILL).all())


# ====================================================================== the shared check on a case
def _viterbi(lib, emit, trans, lens, start, stop, narrow=False, on_device=None):
    """-> tags, conf, popped of kbner_crf_wide_viterbi (narrow: of kbner_crf_viterbi) on device copies of the inputs (on_device:
    on these device buffers)"""
    B, n, T = emit.shape
    tags, conf, popped = Out((B, n), I32), Out((B, n)), Out((B,), I32)
    d_emit, d_trans, d_lens = on_device or (dev(emit), dev(trans), dev(lens, np.int32))     # held until the kernel has run
    if narrow:
        rc = lib.kbner_crf_viterbi(P(d_emit), P(d_trans), P(d_lens), B, n, T, start, stop, tags.ptr, conf.ptr, popped.ptr, _stream())
    else:
        ws = Workspace(lib, B, n, T)
        rc = lib.kbner_crf_wide_viterbi(P(d_emit), P(d_trans), P(d_lens), B, n, T, start, stop, tags.ptr, conf.ptr, popped.ptr,
                                        ws.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert narrow or ws.guard_intact(), "wrote behind the workspace"
    out = tags.get(), conf.get(), popped.get()
    assert all(no_sentinel(a) for a in out), "viterbi left an output element unwritten"
    return out


def _smooth(lib, x, got):
    """kbner_crf_wide_nll_fwd, _nll_bwd and _posterior on the inputs x of a case -> got[logz, gold, alpha, demit, dtrans, marg]"""
    B, n, T, start, stop = x["B"], x["n"], x["T"], x["start"], x["stop"]
    emit, trans, tags, lens, dloss = dev(x["emit"]), dev(x["trans"]), dev(x["tags"], np.int32), dev(x["lens"], np.int32), dev(x["dloss"])
    logz, gold, alpha = Out((B,)), Out((B,)), Out((B, n + 1, T))
    rc = lib.kbner_crf_wide_nll_fwd(P(emit), P(trans), P(tags), P(lens), B, n, T, start, stop, logz.ptr, gold.ptr, alpha.ptr, _stream())
    assert rc == 0, rc
    demit, dtrans, marg = Out((B, n, T)), Out((T, T), init=x["pattern"]), Out((B, n, T))
    rc = lib.kbner_crf_wide_nll_bwd(P(emit), P(trans), P(tags), P(lens), alpha.ptr, logz.ptr, P(dloss), B, n, T, start, stop, demit.ptr,
                                    dtrans.ptr, _stream())
    assert rc == 0, rc
    rc = lib.kbner_crf_wide_posterior(P(emit), P(trans), P(lens), alpha.ptr, logz.ptr, B, n, T, start, stop, marg.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for k, o in (("logz", logz), ("gold", gold), ("alpha", alpha), ("demit", demit), ("dtrans", dtrans), ("marg", marg)):
        got[k] = o.get()
        if k != "alpha":                                                          # alpha rows above lens[b] are unspecified
            assert no_sentinel(got[k]), "%s: an element was left unwritten" % k


def _run_case(lib, case, also_narrow):
    x = crfref.grid_inputs(case)
    start, stop = x["start"], x["stop"]
    got = {}
    sets = [("v", x["emit"], x["trans"], x["lens"])]
    if x["tie_emit"] is not None:
        sets.append(("tie_", x["tie_emit"], x["tie_trans"], x["tie_lens"]))
    for pre, emit, trans, lens in sets:
        d = (dev(emit), dev(trans), dev(lens, np.int32))
        tags, conf, popped = _viterbi(lib, emit, trans, lens, start, stop, on_device=d)
        got[pre + "tags"], got[("vconf" if pre == "v" else "tie_conf")], got[pre + "popped"] = tags, conf, popped
        if also_narrow:
            ntags, _, npopped = _viterbi(lib, emit, trans, lens, start, stop, narrow=True, on_device=d)
            assert np.array_equal(tags, ntags) and np.array_equal(popped, npopped), "%s: wide and single-wave Viterbi differ" % pre
    _smooth(lib, x, got)
    crfref.check_grid(case, got, STATS)


@pytest.mark.parametrize("case", crfwide_cases.WIDE, ids=crfref.grid_id)
def test_crf_wide_grid(lib, case):
    _run_case(lib, case, also_narrow=False)


@pytest.mark.parametrize("case", crfwide_cases.NARROW, ids=crfref.grid_id)
def test_wide_entry_points_on_narrow_tag_sets(lib, case):
    """1 <= T <= 64 is accepted too: same check, and the decode equals the single-wave kernels' on the same inputs"""
    _run_case(lib, case, also_narrow=True)


# ====================================================================== n is bounded by the workspace alone
def test_sentence_length_is_not_lds_bound(lib):
    """T = 192, B = 2, n = 300: scores and backpointers of 300 x 192 cells are 288 000 B, more than a CU's LDS.  Viterbi against
    oracle.crf (tags, popped) and conf as test_viterbi_dynamic_lds checks it; nll_fwd / nll_bwd against crfref under the rule of
    crfref.check_grid (magnitudes as crfref.grid_reference forms them)."""
    B, n, T, start, stop = 2, 300, 192, 17, 5
    rng = np.random.default_rng(n + T)
    emit, trans, gtags, lens = crfref.real_case(rng, B, n, T, start, stop, 2.0)
    assert lens[0] == n
    tags, conf, popped = _viterbi(lib, emit, trans, lens, start, stop)
    rt, _, rp = crfref._oracle_viterbi(emit, trans, lens, start, stop)
    assert np.array_equal(tags, rt) and np.array_equal(popped, rp)
    r64 = crfref.viterbi(emit, trans, lens, start, stop, np.float64, with_scores=True)
    r32 = crfref.viterbi(emit, trans, lens, start, stop, np.float32)
    step = np.abs(emit.astype(np.float64)).max(axis=2) + crfref.fin(trans).max()
    cid = "T192-n300"
    crfref.check_close(STATS, "viterbi conf", cid, conf, r64[1], r32[1], 2.0 * np.cumsum(step, axis=1))
    # forward / backward
    dloss = np.array([0.7, -0.4], np.float32)
    pattern = crfref.dtrans_pattern(T)
    x = {"B": B, "n": n, "T": T, "start": start, "stop": stop, "emit": emit, "trans": trans, "tags": gtags, "lens": lens,
         "dloss": dloss, "pattern": pattern}
    got = {}
    _smooth(lib, x, got)
    F64 = np.float64
    ref = {}
    for name, dt in (("r64", F64), ("r32", np.float32)):
        r = {}
        r["logz"], r["alpha"] = crfref.forward(emit, trans, lens, start, stop, dtype=dt)
        r["gold"] = crfref.gold(emit, trans, gtags, lens, start, stop, dtype=dt)
        r["demit"], r["dtrans"] = crfref.nll_grads(emit, trans, gtags, lens, dloss, start, stop, dtype=dt)
        r["dtrans"] = r["dtrans"] + pattern.astype(dt)
        ref[name] = r
    r64, r32 = ref["r64"], ref["r32"]
    beta = crfref.backward(emit, trans, lens, start, stop, dtype=F64)
    tmax = crfref.fin(trans).max()
    scan = np.concatenate([np.zeros((B, 1)), np.cumsum(step, axis=1)], axis=1) + tmax
    crfref.check_close(STATS, "nll_fwd logz", cid, got["logz"], r64["logz"], r32["logz"], scan[np.arange(B), lens] + tmax)
    g = np.zeros(B)
    for b in range(B):
        tg = [int(t) for t in gtags[b, :lens[b]]]
        prev = [start] + tg
        g[b] = sum(abs(float(emit[b, k, tg[k]])) + abs(float(trans[tg[k], prev[k]])) for k in range(len(tg))) + abs(float(trans[stop, prev[-1]]))
    crfref.check_close(STATS, "nll_fwd gold", cid, got["gold"], r64["gold"], r32["gold"], g)
    rows = np.repeat((np.arange(n + 1)[None, :] <= lens[:, None])[:, :, None], T, 2)
    small = np.abs(r64["alpha"]) < crfref.BIG
    crfref.check_close(STATS, "nll_fwd alpha", cid, got["alpha"], r64["alpha"], r32["alpha"], np.repeat(scan[:, :, None], T, 2), sel=rows & small)
    size = crfref.fin(r64["alpha"][:, 1:]) + crfref.fin(beta[:, 1:]) + np.abs(r64["logz"])[:, None, None]
    for b in range(B):
        size[b, lens[b]:] = 0.0
    w = np.abs(dloss.astype(F64))
    crfref.check_close(STATS, "nll_bwd demit", cid, got["demit"], r64["demit"], r32["demit"], w[:, None, None] * (size + 1.0))
    mag_dtrans = float((w * (size.reshape(B, -1).max(axis=1) + np.abs(r64["logz"]) + 1.0)).sum()) + np.abs(pattern.astype(F64))
    crfref.check_close(STATS, "nll_bwd dtrans", cid, got["dtrans"], r64["dtrans"], r32["dtrans"], mag_dtrans)
    below = np.arange(n)[None, :] < lens[:, None]
    assert (got["demit"][~below] == 0.0).all() and (got["marg"][~below] == 0.0).all()
    m64, m32 = (crfref.marginals(emit, trans, lens, start, stop, dtype=dt) for dt in (F64, np.float32))
    crfref.check_close(STATS, "posterior", cid, got["marg"], m64, m32, size)


def test_backtrace_walks_more_than_one_chunk(lib):
    """the backtrace stages the backpointers through 32 760 B of LDS, 32 760 // T rows at a time: 171 at T = 191, so n = 301 takes
    two chunks, the second starting at row 130; with T and n odd the chunks and the sentences start at every byte offset of a dword"""
    B, n, T, start, stop = 3, 301, 191, 189, 190
    rows = 32760 // T
    assert rows == 171 < n and {(b * n * T + (n - rows) * T) % 4 for b in range(B)} == {0, 1, 2}
    rng = np.random.default_rng(n * T)
    emit, trans, _, lens = crfref.real_case(rng, B, n, T, start, stop, 2.0)
    lens[1] = 200                                                       # two chunks on a sentence that does not fill the buffer
    tags, conf, popped = _viterbi(lib, emit, trans, lens, start, stop)
    rt, _, rp = crfref._oracle_viterbi(emit, trans, lens, start, stop)
    assert np.array_equal(tags, rt) and np.array_equal(popped, rp)
    temit, ttrans, tlens = crfref.tie_case(np.random.default_rng(n + T), B, n, T, start, stop)
    tlens[0] = n
    tags, conf, popped = _viterbi(lib, temit, ttrans, tlens, start, stop)
    rt, _, rp = crfref._oracle_viterbi(temit, ttrans, tlens, start, stop)
    assert np.array_equal(tags, rt) and np.array_equal(popped, rp)


# ====================================================================== the workspace
def test_workspace_size_is_monotone(lib):
    f = lambda B, n, T: int(lib.kbner_crf_wide_viterbi_ws_bytes(B, n, T))
    for B, n, T in ((1, 1, 1), (2, 130, 65), (16, 48, 137), (2, 300, 192), (5, 1, 191)):
        here = f(B, n, T)
        assert here >= B * n * T * 5                                   # fp32 score + u8 backpointer per cell
        assert f(B + 1, n, T) >= here and f(B, n + 1, T) >= here and (T == 192 or f(B, n, T + 1) >= here)
    assert f(0, 5, 65) == 0 and f(5, 0, 65) == 0


def test_empty_batches_need_no_workspace(lib):
    T = 137
    trans = torch.zeros((T, T), device=DEV)
    # B = 0: returns 0, nothing launched; n = 0 with B = 3: popped = START, a null workspace is fine
    assert lib.kbner_crf_wide_viterbi(None, P(trans), None, 0, 5, T, 3, 4, None, None, None, None, _stream()) == 0
    emit, lens = torch.zeros((3, 0, T), device=DEV), torch.zeros((3,), dtype=I32, device=DEV)
    tags, conf, popped = Out((1,), I32), Out((1,)), Out((3,), I32)
    assert lib.kbner_crf_wide_viterbi(P(emit), P(trans), P(lens), 3, 0, T, 3, 4, tags.ptr, conf.ptr, popped.ptr, None, _stream()) == 0
    torch.cuda.synchronize()
    assert tags.untouched() and conf.untouched() and (popped.get() == 3).all()
    for fn in ("kbner_crf_wide_nll_fwd", "kbner_crf_wide_nll_bwd", "kbner_crf_wide_posterior"):
        nargs = len(getattr(lib, fn).argtypes)
        pre = {"kbner_crf_wide_nll_fwd": 4, "kbner_crf_wide_nll_bwd": 7, "kbner_crf_wide_posterior": 5}[fn]
        args = [None] * pre + [0, 5, T, 3, 4] + [None] * (nargs - pre - 5)
        assert getattr(lib, fn)(*args) == 0


# ====================================================================== argument rejection: -22, nothing launched, nothing written
def _wide_entry_points(lib, B, n, T, start, stop, TA, null_ws=False):
    """the four wide entry points with buffers sized for |B|, |n| and tag count TA (>= 1); -> [(name, rc, outputs)]"""
    Ba, na = max(abs(B), 1), max(abs(n), 1)
    z = lambda *s: torch.zeros(s, device=DEV)
    zi = lambda *s: torch.zeros(s, dtype=I32, device=DEV)
    emit, trans, tags, lens, dloss = z(Ba, na, TA), z(TA, TA), zi(Ba, na), zi(Ba) + na, z(Ba) + 1.0
    alpha, logz = z(Ba, na + 1, TA), z(Ba)
    ws = Workspace(lib, Ba, na, min(TA, 192))
    res = []
    o = [Out((Ba, na), I32), Out((Ba, na)), Out((Ba,), I32)]
    rc = lib.kbner_crf_wide_viterbi(P(emit), P(trans), P(lens), B, n, T, start, stop, o[0].ptr, o[1].ptr, o[2].ptr,
                                    None if null_ws else ws.ptr, _stream())
    res.append(("viterbi", rc, o + [ws]))
    if null_ws:
        return res
    o = [Out((Ba,)), Out((Ba,)), Out((Ba, na + 1, TA))]
    res.append(("nll_fwd", lib.kbner_crf_wide_nll_fwd(P(emit), P(trans), P(tags), P(lens), B, n, T, start, stop, o[0].ptr, o[1].ptr,
                                                      o[2].ptr, _stream()), o))
    o = [Out((Ba, na, TA)), Out((TA, TA))]
    res.append(("nll_bwd", lib.kbner_crf_wide_nll_bwd(P(emit), P(trans), P(tags), P(lens), P(alpha), P(logz), P(dloss), B, n, T, start,
                                                      stop, o[0].ptr, o[1].ptr, _stream()), o))
    o = [Out((Ba, na, TA))]
    res.append(("posterior", lib.kbner_crf_wide_posterior(P(emit), P(trans), P(lens), P(alpha), P(logz), B, n, T, start, stop, o[0].ptr,
                                                          _stream()), o))
    return res


@pytest.mark.parametrize("B,n,T,start,stop", [(2, 3, 0, 0, 0), (2, 3, 193, 0, 1), (2, 3, 137, -1, 28), (2, 3, 137, 137, 28),
                                              (2, 3, 137, 27, -1), (2, 3, 137, 27, 137), (2, 3, 192, 192, 0), (2, 3, 65, 0, 65),
                                              (-1, 3, 137, 27, 28), (2, -1, 137, 27, 28)])
def test_wide_entry_points_reject_bad_arguments(lib, B, n, T, start, stop):
    res = _wide_entry_points(lib, B, n, T, start, stop, max(T, 1))
    torch.cuda.synchronize()
    for name, rc, outs in res:
        assert rc == EINVAL, (name, rc)
        assert all(o.untouched() for o in outs), name


def test_viterbi_rejects_a_null_workspace(lib):
    (name, rc, outs), = _wide_entry_points(lib, 2, 3, 137, 27, 28, 137, null_ws=True)
    torch.cuda.synchronize()
    assert rc == EINVAL and all(o.untouched() for o in outs)
