"""CPU: the stream contract's host side — the verdict-word layout (tests/stream_model.py against
the engine's unpacking), ir.pack_soa's row order, StreamResult.verdicts(), and the shape checks
Engine.eval_batch / eval_stream make before the call."""

import numpy as np
import op_programs as P
import pyoracle as O
import pytest
import stream_model as M

from mythril_amd import _lib, ir
from mythril_amd.engine import Engine, StreamResult, unpack_bits

SIZES = (1, 63, 64, 65, 200)


def _rows(n_cand, n=3):
    rng = np.random.default_rng(n_cand)
    rows = rng.integers(0, 2, size=(n, n_cand)).astype(bool)
    rows[0, :] = True            # every bit up to n_cand set: the tail must still be 0
    rows[1, -1] = True           # the last candidate's bit
    return rows


@pytest.mark.parametrize("n_cand", SIZES)
def test_bit_layout_and_zero_tail(n_cand):
    rows = _rows(n_cand)
    bits = M.pack_bits(rows)
    words = (n_cand + 63) // 64
    assert bits.shape == (3, words) and bits.dtype == np.uint64
    for i in range(3):
        for c in range(n_cand):
            assert (int(bits[i, c >> 6]) >> (c & 63)) & 1 == int(rows[i, c]), (i, c)
    assert M.tail_is_zero(bits, n_cand)
    assert int(bits[0, -1]) == (1 << (n_cand - 64 * (words - 1))) - 1
    assert np.array_equal(M.unpack_bits(bits, n_cand), rows)
    # the engine's numpy unpacking reads the same layout, from uint64 and from int64 words
    assert np.array_equal(unpack_bits(bits, n_cand), rows)
    assert np.array_equal(unpack_bits(bits.view(np.int64), n_cand), rows)
    if n_cand % 64:
        dirty = bits.copy()
        dirty[2, -1] |= np.uint64(1 << 63)
        assert not M.tail_is_zero(dirty, n_cand)
    with pytest.raises(ValueError):
        unpack_bits(bits, n_cand + 64)


@pytest.mark.parametrize("n_cand", SIZES)
def test_stream_result_verdicts(n_cand):
    rows = _rows(n_cand)
    bits, first, count = M.summarize(rows)
    res = StreamResult(bits, first, count, n_cand)
    assert np.array_equal(res.verdicts(), rows)
    assert res.verdicts().dtype == bool and res.verdicts().shape == (3, n_cand)
    assert first.tolist() == [0, int(np.argmax(rows[1])), int(np.argmax(rows[2])) if rows[2].any() else M.NONE]
    assert count.tolist() == [int(r.sum()) for r in rows]
    none = M.summarize([[False] * n_cand])
    assert none[1].tolist() == [M.NONE] and none[2].tolist() == [0] and not none[0].any()


def _batch():
    """Three sets of 2, 3 and 2 variables (widths 256, 64 and 1 among them)."""
    progs = [P.cmp_set(ir.B_ULT, 256, 1, 2, True, parents=False),
             P.ite_set(64, 1, 5, 6, 5, parents=False),
             P.cmp_set(ir.B_EQ, 200, 7, 7, True, base=8, parents=False)]
    assert [len(p.vars) for p in progs] == [2, 3, 2]
    return progs, ir.Batch(progs)


def _cands(prog, n, seed):
    rng = np.random.default_rng(seed)
    return [[int.from_bytes(rng.bytes(32), "little") for _ in prog.vars] for _ in range(n)]


@pytest.mark.parametrize("n_cand", [1, 65])
def test_pack_soa_rows_are_the_sets_rows_of_pf_eval_programs(n_cand):
    """Set s's block of pack_soa is its variables at rows descs[s].var_off .., each row limb by
    limb over the candidates: what pf_eval_programs and pf_eval_batch index."""
    progs, batch = _batch()
    cands = [_cands(p, n_cand, 10 + s) for s, p in enumerate(progs)]
    soa = ir.pack_soa(batch, cands)
    assert soa.shape == (7, 8, n_cand) and soa.dtype == np.uint32 and soa.flags.c_contiguous
    for s, p in enumerate(progs):
        off, nv = int(batch.descs[s][4]), int(batch.descs[s][5])
        for v in range(nv):
            for c in range(n_cand):
                assert ir.from_limbs(soa[off + v, :, c]) == cands[s][c][v]     # unmasked: the kernel masks
    # the layout pf_eval_assignments takes per set, for values within the variables' widths
    small = [[[x & ir.mask(p.vars[v].width) for v, x in enumerate(c)] for c in cs] for p, cs in zip(progs, cands)]
    soa = ir.pack_soa(batch, small)
    for s, p in enumerate(progs):
        off = int(batch.descs[s][4])
        assert np.array_equal(soa[off:off + len(p.vars)], ir.pack_assignments(p, small[s]))
    # a set left out keeps zero rows
    part = ir.pack_soa(batch, [cands[0], None, cands[2]])
    assert not part[2:5].any() and np.array_equal(part[:2], ir.pack_soa(batch, cands)[:2])
    with pytest.raises(ValueError):
        ir.pack_soa(batch, cands[:2])
    with pytest.raises(ValueError):
        ir.pack_soa(batch, [cands[0], cands[1][:-1] + [[1, 2]], cands[2]])
    if n_cand > 1:
        with pytest.raises(ValueError):
            ir.pack_soa(batch, [cands[0][:1], cands[1], cands[2]])


def test_model_matches_the_oracle_set_by_set():
    progs, batch = _batch()
    cands = [_cands(p, 70, 20 + s) for s, p in enumerate(progs)]
    for c in range(0, 70, 3):                       # make a third of set 0 and set 2 hold
        cands[0][c] = [3, 9]
        cands[2][c] = [c, c + (1 << 200)]           # equal at width 200
    bits, first, count = M.expected(batch, cands, [2, 0])
    rows = M.unpack_bits(bits, 70)
    for i, s in enumerate((2, 0)):
        sv = O.SetView.from_batch(batch, s)
        want = [sv.evaluate(a) for a in cands[s]]
        assert rows[i].tolist() == want and first[i] == 0 and count[i] == sum(want) >= 24


class _FakeDb:
    def __init__(self, batch):
        self.batch = batch

    def __len__(self):
        return len(self.batch)


def test_shape_checks_before_the_call():
    """A wrong row count is the likeliest mistake and the kernel cannot see it."""
    _, batch = _batch()
    db = _FakeDb(batch)
    assert Engine._stream_request(db, (7, 8, 5), None).tolist() == [0, 1, 2]
    assert Engine._stream_request(db, (7, 8, 0), [2, 0]).tolist() == [2, 0]
    for shape in ((6, 8, 5), (8, 8, 5), (7, 4, 5), (7, 8), (7, 8, 5, 1)):
        with pytest.raises(_lib.PathFeasError):
            Engine._stream_request(db, shape, None)
    eng = Engine.__new__(Engine)                    # no device: the checks come first
    with pytest.raises(_lib.PathFeasError, match="dtype"):
        eng.eval_batch(db, np.zeros((7, 8, 5), dtype=np.int64))
    with pytest.raises(_lib.PathFeasError, match="variable rows"):
        eng.eval_batch(db, np.zeros((5, 8, 5), dtype=np.uint32))
    with pytest.raises(_lib.PathFeasError, match="GPU"):
        eng.eval_stream(db, np.zeros((7, 8, 5), dtype=np.uint32))
