"""GPU: kbner_gather_rows_blocks_drop (csrc/rows.hip) through kbner.ops against the numpy reference of tests/storeref.py.

The two dropout multipliers are materialised with kbner_dropout_mask (the keep test and scale every product kernel uses) and handed to
the reference, which forms m_e * m_l and the product with the value in float32 and rounds to bf16 once -- the kernel's definition, so
the assertion is EXACT equality, at p = 0.5 (scale 2) and p = 0.25 (scale 4/3, not a bf16 number) alike.  `out` is poisoned with NaN
before every call and carries NaN canary rows behind it: every element of out[0:R_out, 0:ld_out] is written, nothing behind it.

Shapes: B, n = 3, 5 (R = 15, R_out = 128: 113 padding rows, more rows than one workgroup's 4 waves), four blocks of 32 / 8 / 128 / 24
columns (one narrower than a lane's 16 bytes would need care; boundaries inside a 512-column pass), W = 192, ld_store and ld_out in
{192, 256}; idx with -1 rows and a repeated row; block_on all on / all off / alternating; dropout off / element / locked / both.  One
wide case: B, n = 2, 64, W = ld_out = 5120 (ten 512-column passes) with block widths of the ACE stack's kinds that add up to it: one
2048-unit character LM and three 1024-wide encoders.

With every block on the output equals, byte for byte, what the head composed before the kernel existed: gather_rows_ld into a zeroed
X, gather_rows_drop with the same index and sites into a zeroed Xd, Xd copied into a zeroed padded matrix.  Each contract violation
returns KbnerError (-22).  (MI355X run that accompanied this module: 69 cases, 2.8 s, every comparison exact.)"""
import numpy as np
import pytest
import torch

import storeref

pytestmark = pytest.mark.gpu

BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
DEV = "cuda"
NAN = float("nan")
CANARY = 3


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def ops():
    from kbner import ops as _ops
    return _ops


def _sites(ops, p_e, p_l, salt):
    return (((0x9E3779B9 ^ (salt * 7919)) & 0xFFFFFFFF, ops.drop_thresh(p_e) if p_e else 0),
            ((0xC2B2AE35 + salt * 104729) & 0xFFFFFFFF, ops.drop_thresh(p_l) if p_l else 0))


def _masks(ops, B, n, W, de, dl):
    m_e = ops.dropout_mask(1, B * n, W, de[0], de[1])[0].cpu().numpy() if de[1] else None
    m_l = ops.dropout_mask(1, B, W, dl[0], dl[1])[0].cpu().numpy() if dl[1] else None
    return m_e, m_l


def _problem(B, n, ld_store, seed, rows_store=None):
    """bf16 store rows (no zero element: a wrongly zeroed or wrongly kept element shows), idx with -1 rows and one repeated row"""
    rng = np.random.default_rng(seed)
    R = B * n
    rows_store = rows_store or R + 5
    store = torch.from_numpy(rng.standard_normal((rows_store, ld_store)).astype(np.float32)).to(BF16)
    store[store == 0] = 1.0
    idx = rng.permutation(rows_store)[:R].astype(np.int32)
    idx[[2, R - 1]] = -1
    idx[n] = idx[0]
    return store, idx


def _run(ops, store, idx, block_col, block_on, n, R_out, ld_out, W, de, dl):
    full = torch.full((R_out + CANARY, ld_out), NAN, dtype=BF16, device=DEV)
    out = full[:R_out]
    got = ops.gather_rows_blocks_drop(store.to(DEV), torch.from_numpy(idx).to(DEV), block_col, torch.tensor(block_on, dtype=U8, device=DEV),
                                      n, R_out=R_out, W=W, drop_e=de, drop_l=dl, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.isnan(full[R_out:]).all(), "the kernel wrote behind out"
    return out.cpu()


BLOCK_COL = [0, 32, 40, 168, 192]
ON = {"all_on": [1, 1, 1, 1], "all_off": [0, 0, 0, 0], "alternating": [1, 0, 1, 0]}
DROPS = {"off": (0.0, 0.0), "element": (0.5, 0.0), "locked": (0.0, 0.25), "both_a": (0.5, 0.25), "both_b": (0.25, 0.5)}


@pytest.mark.parametrize("drop", sorted(DROPS))
@pytest.mark.parametrize("on", sorted(ON))
@pytest.mark.parametrize("ld_store,ld_out", [(192, 192), (256, 192), (192, 256), (256, 256)])
def test_equals_the_reference_exactly(ops, ld_store, ld_out, on, drop):
    B, n, W, R_out = 3, 5, 192, 128
    store, idx = _problem(B, n, ld_store, seed=ld_store + ld_out)
    de, dl = _sites(ops, *DROPS[drop], salt=ld_store // 64 + len(on))
    m_e, m_l = _masks(ops, B, n, W, de, dl)
    if m_e is not None or m_l is not None:
        m = (m_e if m_e is not None else 1.0) * (np.repeat(m_l, n, 0) if m_l is not None else 1.0)
        assert 0.2 < float((m == 0).mean()) < 0.8                # the sites do drop, and do keep
    got = _run(ops, store, idx, BLOCK_COL, ON[on], n, R_out, ld_out, W, de, dl)
    want = storeref.gather_blocks(store.float().numpy(), idx, BLOCK_COL, ON[on], ld_out, R_out, W, n, m_e, m_l)
    why = storeref.mismatch(got.float().numpy(), want)
    assert why is None, why
    if on == "all_off":
        assert not bool(got.view(torch.int16).any())


def test_wide_rows_with_the_ace_block_widths(ops):
    B, n, W = 2, 64, 5120
    block_col = [0, 2048, 3072, 4096, 5120]
    store, idx = _problem(B, n, W, seed=9, rows_store=B * n + 3)
    for k, (on, drop) in enumerate([([1, 1, 1, 1], (0.0, 0.0)), ([1, 0, 1, 1], (0.5, 0.25))]):
        de, dl = _sites(ops, *drop, salt=40 + k)
        m_e, m_l = _masks(ops, B, n, W, de, dl)
        got = _run(ops, store, idx, block_col, on, n, 128, W, W, de, dl)
        want = storeref.gather_blocks(store.float().numpy(), idx, block_col, on, W, 128, W, n, m_e, m_l)
        why = storeref.mismatch(got.float().numpy(), want)
        assert why is None, why


@pytest.mark.parametrize("drop", ["off", "element", "both_a"])
@pytest.mark.parametrize("Dp,Dq", [(192, 256), (256, 256)])
def test_every_block_on_equals_the_composition_it_replaces_byte_for_byte(ops, Dp, Dq, drop):
    """packing real-token rows of X into a store and reading them back through the new kernel against the head's first stage as it
    was: X (zero rows at padding) -> gather_rows_drop with an identity index (WordDropout: -1) into a zeroed Xd -> zero-padded Xt"""
    B, n, Mp = 3, 5, 128
    R = B * n
    lengths = [5, 1, 3]
    rng = np.random.default_rng(Dp + Dq)
    X = torch.zeros((Mp, Dp), dtype=BF16, device=DEV)
    for b, ln in enumerate(lengths):
        X[b * n:b * n + ln] = torch.from_numpy(rng.standard_normal((ln, Dp)).astype(np.float32)).to(BF16).to(DEV)
    word = np.zeros(n, bool)
    word[1] = True
    de, dl = _sites(ops, *DROPS[drop], salt=3)
    # the composition
    ident = torch.arange(R, dtype=I32, device=DEV)
    idx_old = torch.where(torch.from_numpy(np.tile(word, B)).to(DEV), torch.full_like(ident, -1), ident)
    Xd = torch.zeros((Mp, Dp), dtype=BF16, device=DEV)
    ops.gather_rows_drop(X, idx_old, n, de, dl, out=Xd)
    Xt = torch.zeros((Mp, Dq), dtype=BF16, device=DEV)
    Xt[:, :Dp] = Xd
    # the store: the real-token rows packed by gather_rows_ld, then one launch
    real = np.concatenate([b * n + np.arange(ln) for b, ln in enumerate(lengths)]).astype(np.int32)
    store = torch.full((len(real) + 2, Dp), NAN, dtype=BF16, device=DEV)
    ops.gather_rows_into(X, torch.from_numpy(real).to(DEV), store, 0, Dp)
    idx = np.full((B, n), -1, np.int32)
    off = 0
    for b, ln in enumerate(lengths):
        idx[b, :ln] = np.arange(off, off + ln)
        off += ln
    idx = np.where(np.tile(word, B), -1, idx.reshape(-1)).astype(np.int32)
    got = _run(ops, store, idx, [0, 32, 64, Dp], [1, 1, 1], n, Mp, Dq, Dp, de, dl)
    assert torch.equal(got.view(torch.int16), Xt.cpu().view(torch.int16))
    assert bool(Xt[:R].any()) and not bool(Xt[1].any())


def test_contract_violations_return_minus_22(ops):
    from kbner.lib import KbnerError
    B, n, W = 3, 5, 192
    store, idx = _problem(B, n, 256, seed=1)
    store, idx_d = store.to(DEV), torch.from_numpy(idx).to(DEV)
    on4 = torch.ones(4, dtype=U8, device=DEV)

    def call(block_col=BLOCK_COL, block_on=on4, n_=n, R_out=128, ld_out=256, W_=W, idx_=idx_d, store_=store):
        out = torch.full((max(R_out, 1), ld_out), NAN, dtype=BF16, device=DEV)
        ops.gather_rows_blocks_drop(store_, idx_, block_col, block_on, n_, R_out=R_out, W=W_, out=out)
        return out

    call()                                                           # the legal call
    bad = [dict(block_col=[0], block_on=torch.ones(0, dtype=U8, device=DEV)),                              # nblk = 0
           dict(block_col=list(range(0, 8 * 66, 8)), block_on=torch.ones(65, dtype=U8, device=DEV), W_=256),  # nblk = 65
           dict(block_col=[0, 32, 44, 168, 192]),                    # an entry that is no multiple of 8
           dict(block_col=[0, 32, 40, 168, 200]),                    # block_col[nblk] > W
           dict(block_col=[0, 40, 32, 168, 192]),                    # not ascending
           dict(W_=264),                                             # W > ld_store
           dict(W_=188, block_col=[0, 32, 40, 168, 184]),            # W no multiple of 8
           dict(store_=store[:, :252].contiguous()),                 # ld_store no multiple of 8
           dict(ld_out=252),                                         # ld_out no multiple of 8
           dict(ld_out=184),                                         # W > ld_out
           dict(n_=0), dict(n_=4),                                   # n >= 1, R % n == 0
           dict(R_out=8)]                                            # R > R_out
    for kw in bad:
        with pytest.raises(KbnerError, match="-22"):
            call(**kw)
    # the library's own check of the scalars, below the wrapper
    from kbner import lib as L
    lib = L.load()
    out = torch.empty((128, 256), dtype=BF16, device=DEV)
    cols = torch.tensor(BLOCK_COL, dtype=I32, device=DEV)
    st = L.stream_ptr()

    def raw(ld_store=256, nblk=4, ld_out=256, R=15, R_out=128, W_=192, n_=5):
        return lib.kbner_gather_rows_blocks_drop(L.ptr(store), ld_store, L.ptr(idx_d), L.ptr(cols), L.ptr(on4), nblk, L.ptr(out), ld_out, R,
                                                 R_out, W_, n_, 1, 0, 1, 0, st)
    assert raw() == 0
    for kw in (dict(nblk=0), dict(nblk=65), dict(W_=264), dict(W_=188), dict(ld_store=252), dict(ld_out=252), dict(ld_out=184), dict(n_=0),
               dict(n_=4), dict(R_out=8), dict(R=-5)):
        assert raw(**kw) == -22, kw
    torch.cuda.synchronize()


def test_an_empty_batch_writes_zeros(ops):
    """R = 0: no index is read, the padding rows are still written"""
    store = torch.ones((4, 64), dtype=BF16, device=DEV)
    got = _run(ops, store, np.zeros(0, np.int32), [0, 64], [1], 1, 128, 64, 64, (0, 0), (0, 0))
    assert not bool(got.view(torch.int16).any())
