"""The inputs of tests/test_gpu_many_blocks.py are what that module needs them to be -- conditions on the case builder
(tests/manyblocks.py), met by the reference alone: no engine here.  A condition that fails is a reason to change the generator,
not the bound."""
import numpy as np

import manyblocks as mb


def test_the_count_crosses_16_bits_and_leaves_a_remainder():
    assert mb.N > 65536 and mb.N % 256 == 1
    for per in (4, 16, 64, 256):
        assert mb.N % per == 1
    case = mb.ragged()
    assert case.n.size == mb.N and mb.contiguous_sizes().size == mb.N
    assert np.array_equal(case.n[:64], np.arange(64)) and np.array_equal(case.n[-64:], mb.BSZ - np.arange(64))
    assert int(case.n.min()) == 0 and int(case.n.max()) == mb.BSZ
    assert int((case.n == 0).sum()) >= 50
    assert int((case.n == mb.BSZ).sum()) * 10 >= mb.N
    assert 30e6 < int(case.off[-1]) < 40e6
    assert mb.contiguous().size == (mb.N - 1) * mb.BSZ + mb.LAST and 0 < mb.LAST < mb.BSZ


def test_the_cases_are_seeded():
    a, b = mb.ragged(), mb.ragged.__wrapped__()
    assert a is not b and np.array_equal(a.n, b.n) and np.array_equal(a.buf, b.buf)
    assert np.array_equal(mb.contiguous(), mb.contiguous.__wrapped__())


def test_verdicts_at_a_tight_capacity_are_mixed(ref):
    for level in (1, 9):
        res, _ = mb.want_raw(level, "n")
        share = float((res == 0).mean())
        assert 0.10 <= share <= 0.90, (level, share)
        full, _ = mb.want_raw(level, "bound")
        assert int((full <= 0).sum()) == 0, level


def test_records_are_stored_and_not(ref, orc):
    for form in ("ragged", "contiguous"):
        share = mb.stored_share(mb.want_records(1, form))
        assert 0.10 <= share <= 0.90, (form, share)
    # the record framing here == the oracle's own record of a block (a stored one, a compressed one, the empty one)
    recs = mb.want_records(1, "ragged")
    case = mb.ragged()
    for i in (0, 1, 63, 64, 69, 70, mb.N - 1):
        assert np.array_equal(recs.a[i, :recs.n[i]], orc.block_record(np.ascontiguousarray(case.block(i)), mb.BSZ, True)), i


def test_the_oracle_decodes_every_reference_block(ref, orc):
    """Every block of the reference at levels 1 and 9 goes back to its plaintext through the oracle's decoder."""
    case = mb.ragged()
    plain = mb.plaintext_rows("ragged")
    for level in (1, 9):
        res, comp = mb.want_raw(level, "bound")
        out = mb.rows(mb.N, mb.REC_STRIDE)
        f = mb._orc().orc_decompress_safe
        src, dst, n, cap = comp.addr().tolist(), mb.Rows(out, res).addr().tolist(), res.tolist(), case.n.tolist()
        got = np.array([f(src[i], n[i], dst[i], cap[i]) for i in range(mb.N)], dtype=np.int32)
        assert np.array_equal(got, case.n), level
        assert mb.first_bad_row(out, plain.a, case.n) is None, level


def test_damaged_inputs_are_damaged_and_mostly_refused(ref):
    """Every 101st raw block and every 89th record differs from the good one; the reference refuses a good part of the raw ones."""
    _, good = mb.want_raw(1, "bound")
    bad = mb.damaged_blocks()
    differs = (good.n != bad.n) | (good.a != bad.a).any(axis=1)
    assert np.array_equal(np.flatnonzero(differs), np.arange(0, mb.N, 101))
    for extra in (0, 8):
        res, _ = mb.want_decode(extra)
        hit = np.zeros(mb.N, dtype=bool); hit[::101] = True; hit[::97] = True
        assert np.array_equal(res[~hit], mb.ragged().n[~hit]), extra
        assert int((res[::101] < 0).sum()) >= 100, extra
        assert int((res[::97] < 0).sum()) >= 300, extra
    for checksum in (True, False):
        recs, res, st, out = mb.damaged_records(checksum)
        hit = np.flatnonzero(st != 0)
        assert np.all(hit % 89 == 0) and hit.size >= 200, checksum
        assert set(np.unique(st).tolist()) == ({0, 1, 2} if checksum else {0, 2, 3}), checksum


def test_history_outside_the_block_round_trips(ref, orc):
    """The linked and dictionary records of the contiguous form decode, with their history, to the plaintext (oracle decoder)."""
    case = mb.contiguous_as_ragged()
    for level in (1, 9):
        recs = mb.want_linked_records(level)
        assert 0.10 <= mb.stored_share(recs) <= 0.90, level
        for i in list(range(0, 300)) + list(range(mb.N - 300, mb.N)):
            word = int(recs.a[i, 0:4].view("<u4")[0])
            blk = case.block(i)
            if word & 0x80000000:
                assert np.array_equal(recs.a[i, 4:4 + blk.size], blk), (level, i)
            else:
                payload = np.ascontiguousarray(recs.a[i, 4:4 + word])
                r, out = (orc.decompress_safe_dict(payload, mb.BSZ + 8, np.ascontiguousarray(case.block(i - 1))) if i
                          else orc.decompress_safe(payload, mb.BSZ + 8))
                assert r == blk.size and np.array_equal(out, blk), (level, i)
    recs, dec, plain = mb.want_dict_records()
    assert np.array_equal(dec, case.n)
    assert mb.first_bad_row(plain.a, mb.plaintext_rows("contiguous").a, case.n) is None
