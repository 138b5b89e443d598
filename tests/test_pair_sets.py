"""The launch sets of the pair calls: every entry point gives the same
arrays whether its pairs go to the device one, two or all at a time
(RF_OPT_PAIR_CHUNK 1, 2, 65536).  Half of the reads are copies of their
template and stop after the first round of the band doubling, the others go
on, so the later rounds run over a non-contiguous list of pairs whose set
offsets (moves, texts, index maps) differ from the first round's.
"""
import numpy as np
import pytest

from _util import SEQ_SCORES, random_seq
from rifraf_amd import RifrafSequence
from rifraf_amd._lib import RF_SKEW, RF_TRIM

pytestmark = pytest.mark.gpu

NPAIRS, BW = 12, 3


@pytest.fixture(scope="module")
def pair_set():
    """Templates of 20..60 bases; read k is a copy (even k) or carries two
    substitutions, an insertion and a deletion (odd k)."""
    rng = np.random.default_rng(3301)
    seqs, tpls = [], []
    for k in range(NPAIRS):
        t = random_seq(int(rng.integers(22, 59)), rng)
        s = list(t)
        if k % 2:
            a, b, c, d = sorted(rng.choice(np.arange(2, len(t) - 2), size=4, replace=False).tolist())
            s[a] = (s[a] + 1) % 4
            s[c] = (s[c] + 2) % 4
            del s[d]
            s.insert(b, (s[b] + 3) % 4)
        s = np.array(s, np.uint8)
        assert 20 <= len(s) <= 60 and 20 <= len(t) <= 60
        seqs.append(RifrafSequence(s, np.full(len(s), -2.0), BW, SEQ_SCORES))
        tpls.append(t)
    return seqs, tpls


def flat(moves):
    """A list of per-pair arrays (None: an invalid pair) as lengths and one array."""
    lens = np.array([-1 if m is None else len(m) for m in moves])
    return lens, np.concatenate([np.zeros(0, np.int8) if m is None else m for m in moves])


def products(engine, seqs, tpls, flags):
    """Every output of the four entry points as a dict of arrays."""
    ids = np.arange(NPAIRS)
    caps = np.array([len(seqs[k]) + len(tpls[k]) for k in ids])
    out = {"scores": engine.pair_scores(ids, ids, BW, flags).view(np.int64)}
    sc, mv, ne = engine.pair_align(ids, ids, BW, flags, caps=caps)
    out.update(align_scores=sc.view(np.int64), align_nerr=ne)
    out["align_nmoves"], out["align_moves"] = flat(mv)
    sc, mv, ne, bw, rd = engine.pair_align_smart(ids, ids, BW, 0.0, max_doublings=2, flags=flags, caps=caps)
    out.update(smart_scores=sc.view(np.int64), smart_nerr=ne, smart_bw=bw, smart_rounds=rd)
    out["smart_nmoves"], out["smart_moves"] = flat(mv)
    sc, r = engine.pair_align_text(ids, ids, BW, 0.0, max_doublings=2, flags=flags, want_text=True, want_indices=True,
                                   want_tolerance=True, caps=(caps, np.array([len(t) for t in tpls])))
    out.update(text_scores=sc.view(np.int64), text_aln_len=r.aln_len, text_t2s_len=r.t2s_len,
               text_tolerance=r.tolerance, text_nerr=r.nerrors, text_bw=r.bandwidths, text_rounds=r.rounds)
    texts = [("", "") if x is None else x for x in r.texts()]
    out["text_t"] = np.frombuffer("|".join(t for t, _ in texts).encode(), np.uint8)
    out["text_s"] = np.frombuffer("|".join(s for _, s in texts).encode(), np.uint8)
    out["text_t2s"] = np.concatenate([np.zeros(0, np.int32) if r.indices(k) is None else r.indices(k) for k in ids])
    return {k: np.array(v, copy=True) for k, v in out.items()}


@pytest.mark.parametrize("flags", (0, RF_SKEW | RF_TRIM), ids=("plain", "skew_trim"))
def test_pair_chunk_does_not_change_any_output(engine, opts, pair_set, flags):
    seqs, tpls = pair_set
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    opts("pair_chunk", 65536)
    whole = products(engine, seqs, tpls, flags)
    # the copies stop after round 1, the edited reads go on: rounds 2.. run over a non-contiguous list
    for name in ("smart_rounds", "text_rounds"):
        assert (whole[name] == 1).any() and (whole[name] > 1).any(), (name, whole[name])
    for chunk in (1, 2):
        opts("pair_chunk", chunk)
        got = products(engine, seqs, tpls, flags)
        assert got.keys() == whole.keys()
        for name in whole:
            assert np.array_equal(got[name], whole[name]), (chunk, name, got[name], whole[name])
