"""The host side of the sequence uploads (csrc/rifraf_seq_upload.h) without a
GPU: rf_host_row_codes runs the three coding passes of rf_set_sequences on a
dictionary of its own, rf_host_upload_chunks the chunk splitter of both upload
paths.  Everything is compared bit for bit (codes are keyed by bit patterns)."""
import numpy as np
import pytest

from rifraf_amd import _lib

# about 30 distinct doubles; -0.0 and 0.0 differ in their bits and so in their codes
POOL = np.array([-np.inf, -0.0, 0.0] + [-0.25 * k for k in range(1, 28)])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def pooled_tables(rng, lens):
    """Tables of sequences of the given lengths with values drawn from POOL,
    in rf_set_sequences' layout (del: n + 1 per sequence at off[k] + k)."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, K = int(off[-1]), len(lens)
    draw = lambda n: POOL[rng.integers(0, len(POOL), n)]   # noqa: E731
    return {"bases": rng.integers(0, 4, N).astype(np.uint8), "off": off, "match": draw(N), "mismatch": draw(N),
            "ins": draw(N), "del": draw(N + K)}


def run(t, **kw):
    return _lib.host_row_codes(t["bases"], t["off"], t["match"], t["mismatch"], t["ins"], t["del"], **kw)


def sequences(t):
    """(k, n, match, mismatch, ins, del, bases) per sequence."""
    off = t["off"]
    for k in range(len(off) - 1):
        a, b = int(off[k]), int(off[k + 1])
        yield k, b - a, t["match"][a:b], t["mismatch"][a:b], t["ins"][a:b], t["del"][a + k:b + k + 1], t["bases"][a:b]


def concat(*ts):
    """Several table sets as one sequence list."""
    off = np.concatenate([[0]] + [t["off"][1:] + sum(int(u["off"][-1]) for u in ts[:i]) for i, t in enumerate(ts)])
    out = {k: np.concatenate([t[k] for t in ts]) for k in ("bases", "match", "mismatch", "ins", "del")}
    out["off"] = off.astype(np.int64)
    return out


@pytest.fixture(scope="module")
def pooled():
    rng = np.random.default_rng(1212)
    lens = [1, 40] + rng.integers(1, 41, 10).tolist()
    t = pooled_tables(rng, lens)
    return t, run(t, nthreads=1), run(t, nthreads=4)


def test_code_order_is_serial_first_occurrence(pooled):
    """With 1 thread and with 4 the value arrays and every record are
    identical, and code i is the i-th distinct key in serial reading order."""
    t, one, four = pooled
    np.testing.assert_array_equal(one.records, four.records)
    np.testing.assert_array_equal(bits(one.val3), bits(four.val3))
    np.testing.assert_array_equal(bits(one.val1), bits(four.val1))
    assert (one.coded.tolist(), one.finite.tolist()) == (four.coded.tolist(), four.finite.tolist())
    seen3, seen1 = {}, {}
    for _, n, mt, mm, ins, dl, _ in sequences(t):
        for i in range(n):
            seen3.setdefault((int(bits(mt)[i]), int(bits(mm)[i]), int(bits(ins)[i])), len(seen3))
        for i in range(n + 1):
            seen1.setdefault(int(bits(dl)[i]), len(seen1))
    assert one.coded.all() and one.uncoded_reads == 0
    assert [tuple(int(x) for x in bits(r)[:3]) for r in one.val3] == list(seen3)
    assert (one.val3[:, 3] == 0).all()
    assert bits(one.val1).tolist() == list(seen1)
    assert len(seen1) == len(POOL)   # every pool value occurs, -0.0 and 0.0 as two codes


def test_record_packing(pooled):
    """Bits 0-15 / 16-31 / 32-47 / 48-55 of every record, looked up in the
    value arrays, give back (match, mismatch, ins)[i], del[i], del[i + 1] and
    the base, bit for bit."""
    t, one, _ = pooled
    off = t["off"]
    for k, n, mt, mm, ins, dl, bs in sequences(t):
        rec = one.records[off[k]:off[k + 1]]
        c3, d0, d1, base = (rec & 0xffff).astype(int), ((rec >> 16) & 0xffff).astype(int), \
            ((rec >> 32) & 0xffff).astype(int), ((rec >> 48) & 0xff).astype(np.uint8)
        assert (rec >> 56 == 0).all()
        np.testing.assert_array_equal(bits(one.val3[c3, 0]), bits(mt))
        np.testing.assert_array_equal(bits(one.val3[c3, 1]), bits(mm))
        np.testing.assert_array_equal(bits(one.val3[c3, 2]), bits(ins))
        np.testing.assert_array_equal(bits(one.val1[d0]), bits(dl[:-1]))
        np.testing.assert_array_equal(bits(one.val1[d1]), bits(dl[1:]))
        np.testing.assert_array_equal(base, bs)


def test_finite_flag(pooled):
    """finite is false exactly for the sequences with a non-finite entry among
    their 4 n + 1 table values."""
    t, one, _ = pooled
    exp = [bool(np.isfinite(np.concatenate([mt, mm, ins, dl])).all()) for _, _, mt, mm, ins, dl, _ in sequences(t)]
    assert one.finite.tolist() == exp
    assert True in exp and False in exp


def test_full_dictionary_tables_path():
    """One upload of 67 sequences x 1000 positions of all-distinct triples
    fills the 65,536 triple codes: the 65 sequences that fit are coded, the
    other two are not and are counted; a later sequence of values already held
    is coded; an upload flagged fresh starts from an empty dictionary."""
    K, n = 67, 1000
    match = -(1.0 + np.arange(K * n) * 2.0 ** -20)
    off = np.arange(K + 1, dtype=np.int64) * n
    big = {"bases": np.zeros(K * n, np.uint8), "off": off, "match": match, "mismatch": match - 1.0,
           "ins": match - 2.0, "del": np.full(K * n + K, -3.0)}
    r = run(big, nthreads=4)
    assert len(r.val3) == _lib.RF_CODES and len(r.val1) == 1
    assert r.coded.tolist() == [True] * 65 + [False] * 2
    assert r.uncoded_reads == 2
    np.testing.assert_array_equal(bits(r.val3[:, 0]), bits(match[:_lib.RF_CODES]))   # the 536 that still fitted stay
    held = {"bases": np.ones(n, np.uint8), "off": off[:2], "match": match[:n][::-1].copy(),
            "mismatch": match[:n][::-1] - 1.0, "ins": match[:n][::-1] - 2.0, "del": np.full(n + 1, -3.0)}
    last = {k: (v[-n:] if k not in ("off", "del") else v) for k, v in big.items()}
    last["off"], last["del"] = off[:2], np.full(n + 1, -3.0)
    r = run(concat(big, held, last), uploads=[0, K, K + 1, K + 2], flags=[0, 0, 1], nthreads=2)
    assert r.coded.tolist() == [True] * 65 + [False] * 2 + [True, True]
    assert r.uncoded_reads == 2
    np.testing.assert_array_equal(bits(r.val3[:, 0]), bits(match[-n:]))   # the fresh dictionary: the last upload's alone
    assert (r.records[-n:] & 0xffff).tolist() == list(range(n))


def test_undo_restores_the_dictionary():
    """Undoing an upload of held and new keys leaves the sizes, the values and
    the next code as before it: the new keys are unknown again, and a later
    upload gets the codes it would have got without the undone one."""
    rng = np.random.default_rng(77)
    a = pooled_tables(rng, [7, 9])
    a["match"] = np.abs(a["match"]) + 100.0           # A's triples are its own
    b = pooled_tables(rng, [12, 3, 8])                # del values A holds, triples it does not ...
    b["match"][:12], b["mismatch"][:12], b["ins"][:12] = a["match"][:12], a["mismatch"][:12], a["ins"][:12]   # ... and some it does
    c = pooled_tables(rng, [10])
    c["match"][:5], c["mismatch"][:5], c["ins"][:5] = b["match"][12:17], b["mismatch"][12:17], b["ins"][12:17]   # keys B had added
    only_a = run(a)
    undone = run(concat(a, b), uploads=[0, 2, 5], flags=[0, 2])
    assert undone.coded.all()
    for x, y in ((only_a.val3, undone.val3), (only_a.val1, undone.val1)):
        np.testing.assert_array_equal(bits(x), bits(y))
    nb = int(b["off"][-1])
    kept = run(concat(a, b), uploads=[0, 2, 5])
    assert len(kept.val3) > len(only_a.val3)          # B did add triples
    recb = undone.records[-nb:] & 0xffff
    assert (recb[:12] < len(only_a.val3)).all() and (recb[12:] >= len(only_a.val3)).all()
    after_undo = run(concat(a, b, c), uploads=[0, 2, 5, 6], flags=[0, 2, 0])
    without_b = run(concat(a, c), uploads=[0, 2, 3])
    for x, y in ((without_b.val3, after_undo.val3), (without_b.val1, after_undo.val1)):
        np.testing.assert_array_equal(bits(x), bits(y))
    np.testing.assert_array_equal(without_b.records[-10:], after_undo.records[-10:])
    assert ((after_undo.records[-10:-5] & 0xffff) >= len(only_a.val3)).all()   # B's keys were new again for C


def tables_chunks_before(n, nci, ncd, budget):
    """rf_set_sequences' chunk loop as it stood before the shared splitter."""
    out, k0 = [], 0
    while k0 < len(n):
        k1, ct = k0, 0
        while k1 < len(n):
            ln = 4 * n[k1] + 1 + nci[k1] + ncd[k1] + n[k1]
            if k1 > k0 and (ct + ln) * 8 > budget:
                break
            ct += ln
            k1 += 1
        out.append(k1)
        k0 = k1
    return out


def codes_chunks_before(off, budget):
    """rf_set_sequences_codes' chunk loop as it stood before the shared splitter."""
    out, k0, nseq = [], 0, len(off) - 1
    while k0 < nseq:
        k1 = k0 + 1
        while k1 < nseq and 2 * (off[k1 + 1] - off[k0]) <= budget:
            k1 += 1
        out.append(k1)
        k0 = k1
    return out


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def test_chunk_splitter_at_budget_boundaries():
    """Budgets exactly at, one below and one above every cumulative boundary,
    and one the first sequence alone exceeds (it is taken alone)."""
    lens = [5, 5, 5, 100, 1, 1]
    off, zero = offsets(lens), [0] * len(lens)
    tb = np.cumsum([(5 * n + 1) * 8 for n in lens])
    cb = np.cumsum([2 * n for n in lens])
    for b in sorted({int(x) + d for x in tb for d in (-1, 0, 1)} | {100}):
        assert _lib.host_upload_chunks(off, False, budget=b) == tables_chunks_before(lens, zero, zero, b), b
    for b in sorted({int(x) + d for x in cb for d in (-1, 0, 1)} | {3}):
        assert _lib.host_upload_chunks(off, True, budget=b) == codes_chunks_before(off.tolist(), b), b
    assert _lib.host_upload_chunks(off, False, budget=100)[0] == 1 and _lib.host_upload_chunks(off, True, budget=3)[0] == 1
    # with codon tables: n - 2 and n + 1 entries more per sequence
    nci, ncd = [3, 0, 3, 98, 0, 0], [6, 6, 0, 101, 0, 2]
    for b in (200, 300, 520, 4000, 6000, 7000):
        got = _lib.host_upload_chunks(off, False, budget=b, cins_off=offsets(nci), cdel_off=offsets(ncd))
        assert got == tables_chunks_before(lens, nci, ncd, b), b


@pytest.mark.parametrize("stage_kb", [16, 262144])
def test_chunk_splitter_budget_formulas(stage_kb):
    """Both paths' budgets at the stage_kb option: 8 B per table double within
    stage_kb KB; 2 B per position within a quarter of it, at least 1 MB."""
    rng = np.random.default_rng(stage_kb)
    cases = [[5, 5, 5, 100, 1, 1], [300] * 40, [600000, 300, 300, 300], rng.integers(1, 3000, 500).tolist(),
             rng.integers(100000, 9000000, 60).tolist(), [40000000, 5, 40000000, 40000000]]
    split = {False: 0, True: 0}
    for lens in cases:
        off, zero = offsets(lens), [0] * len(lens)
        t = _lib.host_upload_chunks(off, False, stage_kb=stage_kb)
        c = _lib.host_upload_chunks(off, True, stage_kb=stage_kb)
        assert t == tables_chunks_before(lens, zero, zero, max(stage_kb, 1) * 1024)
        assert c == codes_chunks_before(off.tolist(), max(stage_kb * 1024 // 4, 1 << 20))
        split[False] += len(t) > 1
        split[True] += len(c) > 1
    assert split[False] and split[True]   # both paths really split at this option value
