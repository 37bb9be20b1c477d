"""Damaged streams of real size (tests/damaged_streams.py) against what the compiled reference did with them, replayed from
tests/golden/ref_answers.json: the oracle, the drop-in API, the four host stagers and the host index.  No device, except where the
`side` fixture of test_libacm_api.py has acm_read() synthesise on one (-m gpu).

The rule under test is the cursor after a failure: when decode_block fails, the reference's bit reader stands behind the last field it
took - behind the 5 or 7 bits of an out-of-range ternary symbol (decode.c:412, :438, :464), behind the 5 bits of an invalid code (:496),
wherever the data ran out - and the next acm_read parses on from there.  A reader that stands a few bits off delivers the same bytes
before the error and different ones after it."""
import numpy as np
import pytest

import damaged_streams as D
import oracle_api as O
from decode_index import check_hook
from libacm_amd import capi
from stream_edit import TERNARY, host_index
from test_host_synth import host_synth
from test_libacm_api import ours, side  # noqa: F401  (side: a fixture)

BASES = [b.name for b in D.bases()]


def cases_of(base_name):
    return [(c, a) for c, a in zip(D.population(), D.answers()) if c.base.name == base_name]


def pcm_after_error(rec):
    """does the looping decode deliver bytes behind the first failing acm_read?  (what it delivers starts with the blocks in front of it)"""
    first, loops = D.expand(rec)
    return first[1] < 0 and any(loop[0] != first[2] for loop in loops)


def test_population_conditions():
    """what makes the population worth running, asserted over the reference's recorded answers: a later shrink cannot empty the tests"""
    pop, ans = D.population(), D.answers()
    assert len(pop) == len(ans) >= 400 and len({c.name for c in pop}) == len(pop)
    opened = [(c, a) for c, a in zip(pop, ans) if a[0] == 0]
    assert sum(a[2][1] < 0 for c, a in opened) >= 60                    # the reference's looping decode ends with an error
    assert sum(pcm_after_error(a) for c, a in opened) >= 20
    for code in TERNARY:
        hit = [c.name for c, a in opened if c.kind == "symbol" and c.code == code and D.first_error(a) == (D.damaged_block(c), -6) and pcm_after_error(a)]
        assert len(hit) >= 2, (code, hit)
    # every crafted case fails where it was damaged, every kind of damage and every base is there, something opens no more
    for c, a in zip(pop, ans):
        if c.kind in ("symbol", "code"):
            assert D.first_error(a) == (D.damaged_block(c), -6), c.name
        if c.kind == "clean":
            assert D.first_error(a) == (c.base.blocks, 0) and a[2][1:3] == [0, D.samples(c.base) - 3 - (c.base.channels == 2)], c.name
    assert {c.kind for c in pop} == {"clean", "flip1", "flip3", "cut", "symbol", "code"} and {c.base.name for c in pop} == set(BASES)
    assert any(a[0] < 0 for a in ans) and any(len(a) == 6 for a in ans)         # (6 entries: the 2-byte reads are there)


def test_oracle_matches_the_reference():
    """all recorded fields.  (tests/golden/make_golden_ref_answers.py runs this test against the live reference to record them)"""
    wrong = [c.name for c, a in zip(D.population(), D.answers()) if D.record(O.Oracle, c) != a]
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("base", BASES)
def test_drop_in_api(side, base):
    """acm_read_loop at every request size - digest, final status, words, acm_raw_tell - and plain acm_read a block at a time: the error
    comes from the same call as the reference's, after the same bytes"""
    wrong = []
    for c, a in cases_of(base):
        got = D.record(ours, c)
        if got != a:
            wrong.append((c.name, got, a))
    assert not wrong, (len(wrong), wrong[:3])


def staged_by_mform(data):
    """acm_stage_file_mform -> (info, the staged int16 rows put together again: the rows of the byte-plane form, then the int16 tail, hdr)"""
    info, idx, hdr, blob, pairs, mf_rows, mf_bytes = capi.stage_file_mform(data)
    n = info.blocks * info.rows * info.cols
    if mf_rows:
        idx = idx.copy()
        idx[:mf_rows * info.cols] = capi.mform_unrows(info.level, blob, pairs, mf_rows)
    return info, idx[:n], hdr[:info.blocks], mf_rows


@pytest.mark.parametrize("base", BASES)
def test_host_stagers_and_index(base):
    """acm_stage_file, acm_stage_file_mform, acm_index_file and the stagers behind acmk_stage_marks: blocks staged = the blocks the reference
    delivers before its first error, the status is that error, the host synthesis of what was staged has the recorded digest; the marks
    are the clean stream's up to the damaged block"""
    clean = host_index(cases_of(base)[0][0].data)[3]
    forms = 0
    for c, a in cases_of(base):
        rc, info = capi.probe(c.data)
        assert (rc < 0) == (a[0] < 0), c.name
        if rc < 0:
            assert rc == a[0] and host_index(c.data)[0] == rc, c.name
            continue
        (blocks, status, digest), _ = D.expand(a)
        s = capi.stage_file(c.data)
        assert (s.info.blocks, s.info.end_status) == (blocks, status), (c.name, s.info.blocks, s.info.end_status, blocks, status)
        pcm = host_synth(s, n_emit=s.words) if blocks else np.zeros(0, np.uint16)
        assert D.sha(pcm.tobytes()) == digest, c.name
        # the byte-plane stager: the same rows, in whichever form it left them
        m_info, m_idx, m_hdr, mf_rows = staged_by_mform(c.data)
        forms += mf_rows > 0
        assert (m_info.blocks, m_info.end_status, m_info.npatches) == (blocks, status, s.info.npatches), c.name
        assert np.array_equal(m_idx, s.idx) and np.array_equal(m_hdr, s.hdr), c.name
        # the index
        rc, n, end, marks, promised, in_s = host_index(c.data)
        assert (rc, n, end) == (0, blocks, status), (c.name, n, end)
        d = D.damaged_block(c)
        keep = blocks if d is None else min(max(d, 0), blocks)
        assert np.array_equal(marks[:keep], clean[:keep]) and int(marks[keep]["bit"]) == int(clean[keep]["bit"]), c.name
    if capi.lib().acmhip_mform_tile_rows(cases_of(base)[0][0].base.level) > 0 and D.samples(cases_of(base)[0][0].base) >= 1 << 16:
        assert forms                    # (the byte-plane form was written for some of them, not only fallen back from)
    # every stager a batch's pool can pick: return code, blocks, end status and marks are acm_index_file's
    check_hook([c.data for c, a in cases_of(base)])
