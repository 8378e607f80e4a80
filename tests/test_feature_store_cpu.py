"""CPU: what the feature store of the stacked tagger rests on without a GPU.

  - tests/storeref.py (the numpy reference of kbner_gather_rows_blocks_drop) against a per-element loop written from the header's
    sentence, and `storeref.mismatch` refusing six defective evaluations (block boundary off by one, selection ignored, pad columns
    not zeroed, rows beyond R not zeroed, locked mask keyed by row instead of sentence, idx = -1 copied from row 0): the exact
    comparison of tests/test_gpu_store_kernels.py can tell each of them from the definition;
  - kbner.ops checks the table contract the library cannot see (the table is device memory);
  - kbner.stack.FeatureStore's host logic on CPU tensors, kbner.ops replaced by numpy stand-ins: offsets and lookup, re-batching,
    growth, chunks, the budget cut-off, "one sentence missing -> not served", the subset / superset selection rule, close."""
import logging

import numpy as np
import pytest
import torch

import storeref

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


# ---------------------------------------------------------------------- the reference
def naive(store, idx, block_col, block_on, ld_out, R_out, W, n, m_e, m_l, defect=None):
    """the header's sentence, one element at a time; `defect` names one deliberate error"""
    R = len(idx)
    out = np.zeros((R_out, ld_out), np.float32)
    if defect == "pad_cols":
        out[:R, W:] = 1.0
    if defect == "pad_rows":
        out[R:] = 1.0
    for r in range(R):
        s = int(idx[r])
        if s < 0:
            if defect != "minus_one":
                continue
            s = 0
        for c in range(W):
            on = False
            for b in range(len(block_col) - 1):
                inside = (block_col[b] < c <= block_col[b + 1]) if defect == "boundary" else (block_col[b] <= c < block_col[b + 1])
                if inside:
                    on = bool(block_on[b]) or defect == "selection"
            if not on:
                continue
            ml = m_l[r % m_l.shape[0], c] if defect == "locked_by_row" else m_l[r // n, c]
            m = np.float32(m_e[r, c]) * np.float32(ml)
            out[r, c] = storeref.bf16_round([np.float32(store[s, c]) * m])[0]
    return out


def case(seed=0, B=3, n=5, W=48, ld_store=56, ld_out=64, R_out=24, block_col=(0, 8, 24, 40), block_on=(1, 0, 1)):
    rng = np.random.default_rng(seed)
    R = B * n
    store = storeref.bf16_round(rng.standard_normal((11, ld_store)) + 3.0)        # (no zeros: a wrongly kept element shows)
    idx = rng.integers(0, 11, R)
    idx[[1, R - 1]] = -1
    idx[3] = idx[2]
    m_e = np.where(rng.random((R, W)) < 0.5, np.float32(2.0), np.float32(0.0))
    m_l = np.where(rng.random((B, W)) < 0.75, np.float32(4.0 / 3.0), np.float32(0.0)).astype(np.float32)
    return dict(store=store, idx=idx, block_col=list(block_col), block_on=list(block_on), ld_out=ld_out, R_out=R_out, W=W, n=n, m_e=m_e,
                m_l=m_l)


@pytest.mark.parametrize("seed,kw", [(0, {}), (1, dict(block_on=(1, 1, 1))), (2, dict(block_on=(0, 0, 0))),
                                     (3, dict(block_col=(8, 16, 32, 40), block_on=(0, 1, 1))), (4, dict(W=40, ld_store=40, ld_out=40, R_out=15))])
def test_reference_equals_the_per_element_loop(seed, kw):
    c = case(seed, **kw)
    want = naive(**c)
    got = storeref.gather_blocks(**c)
    assert storeref.mismatch(got, want) is None
    assert got[:, c["W"]:].sum() == 0 and got[15:].sum() == 0
    # masks left out are all-ones masks
    ones = dict(c, m_e=np.ones_like(c["m_e"]), m_l=np.ones_like(c["m_l"]))
    assert storeref.mismatch(storeref.gather_blocks(**dict(c, m_e=None, m_l=None)), naive(**ones)) is None


@pytest.mark.parametrize("defect", ["boundary", "selection", "pad_cols", "pad_rows", "locked_by_row", "minus_one"])
def test_the_comparison_refuses_defective_evaluations(defect):
    c = case(7)
    want = storeref.gather_blocks(**c)
    assert storeref.mismatch(naive(**c), want) is None
    why = storeref.mismatch(naive(defect=defect, **c), want)
    assert why is not None, defect
    print("[store] %s: %s" % (defect, why))


def test_contract_of_the_reference_and_of_the_binding():
    ok = dict(ld_store=192, block_col=[0, 32, 40, 168, 192], nblk=4, ld_out=256, R=15, R_out=128, W=192, n=5)
    assert storeref.check_contract(**ok)
    for kw in (dict(nblk=0, block_col=[0]), dict(block_col=[0, 32, 44, 168, 192]), dict(block_col=[0, 32, 40, 168, 200]), dict(W=184),
               dict(W=188), dict(ld_store=188), dict(ld_out=252), dict(ld_out=184), dict(n=0), dict(n=4), dict(R_out=14),
               dict(block_col=[0, 40, 32, 168, 192]), dict(ld_store=184)):
        assert not storeref.check_contract(**dict(ok, **kw)), kw
    from kbner import ops
    from kbner.lib import KbnerError
    assert ops.check_block_cols(np.asarray([0, 32, 40, 168, 192]), 192) == [0, 32, 40, 168, 192]
    for cols, W in (([0, 32, 44, 192], 192), ([0, 32, 200], 192), ([0, 40, 32, 192], 192), ([0], 192), (list(range(0, 8 * 66, 8)), 1024)):
        with pytest.raises(KbnerError, match="-22"):
            ops.check_block_cols(cols, W)


# ---------------------------------------------------------------------- FeatureStore host logic
class flair_log:
    """the messages logged to the "flair" logger inside the block (a handler of its own: the package may have switched the logger's
    propagation off, and propagation is what caplog listens to)"""

    def __enter__(self):
        self.messages = []
        self.handler = logging.Handler(level=logging.INFO)
        self.handler.emit = lambda record: self.messages.append(record.getMessage())
        self.logger = logging.getLogger("flair")
        self.level = self.logger.level
        self.logger.addHandler(self.handler)
        self.logger.setLevel(logging.INFO)
        return self.messages

    def __exit__(self, *exc):
        self.logger.removeHandler(self.handler)
        self.logger.setLevel(self.level)
        return False


class Sent:
    """what the store needs of a sentence: a length and an identity"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class FakeOps:
    """numpy stand-ins for the two kernels the store launches (kbner.ops.gather_rows_into, gather_rows_blocks_drop)"""

    def __init__(self, real):
        self.NO_DROP, self.check_block_cols = real.NO_DROP, real.check_block_cols
        self.calls = []

    def gather_rows_into(self, src, idx, out2d, col, H):
        self.calls.append(("gather_rows_into", idx.numel()))
        i = idx.long()
        rows = torch.where((i >= 0)[:, None], src[i.clamp(min=0), :H], torch.zeros((), dtype=src.dtype))
        out2d[:idx.numel(), col:col + H] = rows

    def gather_rows_blocks_drop(self, store, idx, block_col, block_on, n, R_out=None, ld_out=None, W=None, drop_e=(0, 0), drop_l=(0, 0),
                                out=None):
        self.calls.append(("gather_rows_blocks_drop", idx.numel(), R_out, ld_out, tuple(drop_e), tuple(drop_l)))
        W = store.shape[1] if W is None else W
        got = storeref.gather_blocks(store.float().numpy(), idx.numpy(), block_col.tolist(), block_on.tolist(), ld_out, R_out, W, n)
        return torch.from_numpy(got).to(BF16)


@pytest.fixture
def K(monkeypatch):
    from kbner import stack
    fake = FakeOps(stack.ops)
    monkeypatch.setattr(stack, "ops", fake)
    monkeypatch.setattr(stack, "fake_ops", fake, raising=False)
    return stack


DP, COLS = 64, [0, 32, 64]


def batch_matrix(sents, seed):
    """a batch as the producers leave it: X bf16 [rows padded to 128, DP], token-major rows b * n + t, zero rows at padding"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray([len(s) for s in sents], np.int64)
    B, n = len(sents), int(lengths.max())
    X = torch.zeros(((B * n + 127) // 128 * 128, DP), dtype=BF16)
    for b in range(B):
        X[b * n:b * n + int(lengths[b])] = torch.from_numpy(rng.standard_normal((int(lengths[b]), DP)).astype(np.float32) + 2).to(BF16)
    return X, lengths, n


@pytest.mark.parametrize("mode", ["gpu", "cpu"], ids=["device_store", "host_store"])
def test_offsets_lookup_and_rebatching(K, mode, monkeypatch):
    monkeypatch.setattr(K.FeatureStore, "CHUNK_ROWS", 16)        # several growth steps / chunks at this size
    st = K.FeatureStore(mode, DP, COLS, "cpu", budget_bytes=1 << 20)
    a, b = [Sent(5), Sent(1), Sent(3)], [Sent(7), Sent(7), Sent(2)]
    Xa, la, na = batch_matrix(a, 1)
    Xb, lb, nb = batch_matrix(b, 2)
    assert st.assemble(a, na, DP) is None and (st.hits, st.misses) == (0, 1)
    assert st.add(a, Xa, la, na) and st.add(b, Xb, lb, nb)
    assert len(st) == 6 and not st.add(a, Xa, la, na)             # nothing new: nothing stored twice
    ents = [st.index[id(s)] for s in a + b]
    assert [e[3] for e in ents] == [5, 1, 3, 7, 7, 2] and all(e[0] is s for e, s in zip(ents, a + b))
    if mode == "gpu":
        assert [e[2] for e in ents] == [0, 5, 6, 9, 16, 23] and st.rows == 25 and st.nbytes == 25 * DP * 2
        assert len(st.chunks) == 1 and st.chunks[0].shape[0] == 32  # grown in steps of CHUNK_ROWS, the earlier rows carried over
    else:
        assert [(e[1], e[2]) for e in ents] == [(0, 0), (0, 5), (0, 6), (1, 0), (1, 7), (1, 14)]   # no run straddles two chunks
        assert len(st.chunks) == 2 and all(c.shape == (16, DP) for c in st.chunks)
    for sents, X, n in ((a, Xa, na), (b, Xb, nb)):
        got = st.assemble(sents, n, DP)
        assert got.shape == X.shape and torch.equal(got, X)
    # another batch of stored sentences, another n: each sentence's rows, zero rows at its padding
    mix = [b[2], a[0], b[0]]
    got = st.assemble(mix, 7, 128)
    assert got.shape == (128, 128) and not bool(got[:, DP:].any()) and not bool(got[21:].any())
    assert torch.equal(got[0:2, :DP], Xb[2 * nb:2 * nb + 2]) and not bool(got[2:7].any())
    assert torch.equal(got[7:12, :DP], Xa[0:5]) and torch.equal(got[14:21, :DP], Xb[0:7])
    assert (st.hits, st.misses) == (3, 1)
    # the dropout sites and WordDropout travel to the launch: positions 1 and 6 of every sentence read index -1
    word = np.zeros(7, bool)
    word[[1, 6]] = True
    K.fake_ops.calls.clear()
    got = st.assemble(mix, 7, 128, drop=(word, (11, 22), (33, 44)))
    assert K.fake_ops.calls == [("gather_rows_blocks_drop", 21, 128, 128, (11, 22), (33, 44))]
    assert not bool(got[[1, 6, 8, 13, 15, 20]].any()) and torch.equal(got[7, :DP], Xa[0]) and torch.equal(got[14, :DP], Xb[0])


@pytest.mark.parametrize("mode", ["gpu", "cpu"], ids=["device_store", "host_store"])
def test_budget_cut_off_and_a_missing_sentence(K, mode, monkeypatch):
    monkeypatch.setattr(K.FeatureStore, "CHUNK_ROWS", 16)
    st = K.FeatureStore(mode, DP, COLS, "cpu", budget_bytes=20 * DP * 2)         # 20 rows: one growth step / one chunk of 16
    a, b, c = [Sent(5), Sent(4)], [Sent(6), Sent(6)], [Sent(1)]
    Xa, la, na = batch_matrix(a, 1)
    Xb, lb, nb = batch_matrix(b, 2)
    Xc, lc, nc = batch_matrix(c, 3)
    with flair_log() as messages:
        assert st.add(a, Xa, la, na)
        assert not st.add(b, Xb, lb, nb) and st.full             # 9 + 12 rows do not fit
        assert not st.add(c, Xc, lc, nc)                          # and the store stays shut: nothing is accepted after the cut-off
    assert sum("budget" in m for m in messages) == 1             # logged once
    assert len(st) == 2 and torch.equal(st.assemble(a, na, DP), Xa)
    assert st.assemble([a[0], b[0]], 6, DP) is None               # one sentence missing: the batch is not served
    assert st.assemble(b, nb, DP) is None and (st.hits, st.misses) == (1, 2)


def test_default_budget_is_a_share_of_free_memory(K, monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000 * DP * 2, 4000 * DP * 2))
    assert K.FeatureStore.MAX_FRACTION == 0.5
    assert K.FeatureStore("gpu", DP, COLS, "cpu").budget_rows == 500
    monkeypatch.setattr(K.FeatureStore, "MAX_FRACTION", 0.25)
    assert K.FeatureStore("gpu", DP, COLS, "cpu").budget_rows == 250
    assert K.FeatureStore("cpu", DP, COLS, "cpu").budget_rows > 0
    with pytest.raises(ValueError):
        K.FeatureStore("none", DP, COLS, "cpu")


def test_subset_is_served_superset_refills_and_close_frees(K):
    st = K.FeatureStore("gpu", DP, COLS, "cpu", budget_bytes=1 << 20)
    a, b = [Sent(3), Sent(2)], [Sent(4)]
    Xa, la, na = batch_matrix(a, 1)
    Xb, lb, nb = batch_matrix(b, 2)
    st.select([True, True])
    assert st.add(a, Xa, la, na) and st.have == [True, True]
    # a subset: served from the same rows, the switched-off block's columns zeroed, nothing else
    st.select([True, False])
    got = st.assemble(a, na, DP)
    assert torch.equal(got[:, :32], Xa[:, :32]) and not bool(got[:, 32:].any()) and len(st) == 2
    assert not st.add(b, Xb, lb, nb) and len(st) == 2             # rows computed under the narrower selection are not mixed in
    st.select([True, True])
    assert torch.equal(st.assemble(a, na, DP), Xa)
    # a store filled under a narrower selection lacks a block: a selection that needs it empties the store
    st.close()
    st.select([False, True])
    Xz = Xa.clone()
    Xz[:, :32] = 0                                                 # (the deselected embedding was not computed)
    assert st.add(a, Xz, la, na) and st.have == [False, True]
    with flair_log() as messages:
        st.select([True, True])
    assert len(st) == 0 and st.have is None and any("refills" in m for m in messages)
    assert st.assemble(a, na, DP) is None
    assert st.add(a, Xa, la, na) and torch.equal(st.assemble(a, na, DP), Xa)
    with pytest.raises(ValueError):
        st.select([True])
    # close: the rows, the index and the references to the sentences are gone
    st.close()
    assert st.chunks == [] and st.index == {} and st.rows == 0 and st.nbytes == 0 and len(st) == 0
