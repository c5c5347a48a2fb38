"""Operands for the wave-uniform tests and the saturating digits of pf::udivrem256
(mythril_amd/csrc/u256.h), with a model of the divider in Python integers that says which path
and which digits a case reaches (no GPU needed to import).

The divider takes, in this order, the first path whose test holds for the whole wave:

* zero:      every lane has b = 0 or a < b;
* short:     every lane's divisor fits one limb (b = 0 included): eight 64 / 32 digits;
* one-digit: every lane with b != 0 has the estimate a / b + 2^-12 below 2^32 - 2;
* general:   digits j = 7..0; lanes with b = 0 or b * 2^32j >= 2^288 ("bhigh") sit a digit out,
             a digit whose estimate floor(rem / 2^32j) / b + 2^-12 is below 1 in every other
             lane is skipped, and an estimate one above the true digit (the fraction exceeds
             1 - 2^-12) is put right by one add-back under a wave-uniform branch.

Every estimate is biased up by 2^-12 and converted with saturation at 2^32 - 1.  The f64
estimates are within 2^-16.6 of the exact quotients (u256.h), so the model computes them as
exact fractions and refuses (``Ambiguous``) any case closer than 2^-15 to a decision."""

from fractions import Fraction

import numpy as np

B32 = 1 << 32
FULL = B32 - 1
BIAS = Fraction(1, 1 << 12)
MARGIN = Fraction(1, 1 << 15)


class Ambiguous(AssertionError):
    pass


def limbs(x):
    return (x.bit_length() + 31) // 32


def _decide(est, bound):
    """est >= bound, refusing estimates within the f64 error of the bound."""
    if abs(est - bound) < MARGIN:
        raise Ambiguous((float(est), bound))
    return est >= bound


def _digit(est):
    """What the device makes of an estimate: (digit, saturated)."""
    sat = _decide(est, B32)
    if not sat and abs(est - round(est)) < MARGIN and est >= MARGIN:
        raise Ambiguous(float(est))
    return (FULL, True) if sat else (int(est), False)


def lane_zero(a, b):
    return b == 0 or a < b


def lane_short(a, b):
    return b < B32


def lane_onedigit(a, b):
    return b == 0 or not _decide(Fraction(a, b) + BIAS, B32 - 2)


def short_trace(a, b):
    """Per digit j = 7..0 of the short path: (j, true digit, saturated, corrected down)."""
    d, rem, out = (b or 1), 0, []
    for j in range(7, -1, -1):
        num = (rem << 32) | ((a >> (32 * j)) & FULL)
        q, sat = _digit(Fraction(num, d) + BIAS)
        true = num // d
        assert q in (true, true + 1) or (sat and true == FULL), (hex(a), hex(b), j)
        out.append((j, true, sat, q != true))
        rem = num - true * d
    return out


def onedigit_trace(a, b):
    """(true quotient, saturated, add-back) of a lane of the one-digit path."""
    if b == 0:
        return (0, False, False)
    q, sat = _digit(Fraction(a, b) + BIAS)
    true = a // b
    assert q in (true, true + 1)
    return (true, sat, q != true)


def general_trace(a, b):
    """Per digit j = 7..0 of the general path, for one lane: a dict with ``skip`` (the lane sits
    the digit out), ``want`` (its estimate is >= 1, so the wave must execute the digit),
    ``true`` (the digit), ``sat`` and ``addback`` (should the wave execute it)."""
    rem, out = a, []
    for j in range(7, -1, -1):
        if b == 0 or (b << (32 * j)) >= 1 << 288:
            out.append(dict(j=j, skip=True, want=False, true=0, sat=False, addback=False))
            continue
        est = Fraction(rem >> (32 * j), b) + BIAS
        want = _decide(est, 1)
        q, sat = _digit(est) if want else (0, False)
        true = rem // (b << (32 * j))
        assert true < B32 and q in (true, true + 1) or (sat and true == FULL), (hex(a), hex(b), j)
        out.append(dict(j=j, skip=False, want=want, true=true, sat=sat, addback=q > true))
        rem -= true * (b << (32 * j))
    assert rem == (a % b if b else a)
    return out


def wave_path(lanes):
    """The path a wave of (a, b) lanes takes."""
    if all(lane_zero(a, b) for a, b in lanes):
        return "zero"
    if all(lane_short(a, b) for a, b in lanes):
        return "short"
    if all(lane_onedigit(a, b) for a, b in lanes):
        return "onedigit"
    return "general"


def wave_digits(lanes):
    """For a general-path wave: {j: (lanes that want the digit, lanes that need the add-back)}
    over the digits the wave executes."""
    traces = [general_trace(a, b) for a, b in lanes]
    out = {}
    for k in range(8):
        j = 7 - k
        want = [i for i, t in enumerate(traces) if t[k]["want"]]
        if want:
            out[j] = (want, [i for i, t in enumerate(traces) if t[k]["addback"]])
    return out


def from_digits(digits):
    """A quotient from its digits, highest first."""
    q = 0
    for d in digits:
        q = (q << 32) | d
    return q


# ---- rows: one (a, b) per case, uniform over the wave ------------------------------------
# ``nl`` is the number of limbs the operands may fill: 8 (width 256, unsigned) or 6 (below
# 2^192: fits width 200, and is non-negative at both widths, so the signed ops hand the
# divider these very operands).

def _rng(tag):
    return np.random.default_rng(0xD1F7 + tag)


def _rand(rng, nl, top=None):
    """nl limbs at random, the top limb non-zero (or ``top``)."""
    x = int.from_bytes(rng.bytes(4 * nl), "little")
    t = top if top is not None else (x >> (32 * (nl - 1))) | 1
    return (x & ((1 << (32 * (nl - 1))) - 1)) | (t << (32 * (nl - 1)))


def rows_zero(nl):
    rng = _rng(1)
    top = 1 << (32 * nl)
    out = [(5, 7), (0, 1), (0, top - 1), (top - 2, top - 1), (0, 0), (1, 0), (top - 1, 0),
           (_rand(rng, nl), 0)]
    b = _rand(rng, nl, top=0x80000000)
    out += [(b - 1, b), (_rand(rng, nl - 1), b), (_rand(rng, 1), _rand(rng, 2))]
    for a, b in out:
        assert wave_path([(a, b)]) == "zero"
    return out


def rows_short_sat(nl):
    """One-limb divisors d > 4096, a = d q + (d - 1), a quotient limb 0xFFFFFFFF followed by a
    fraction above 1 - 2^-12: the biased estimate of that digit reaches 2^32.  The quotient's
    top limb is a's top limb over d, below 2^20, so the highest limb that can be all ones is
    limb nl - 2."""
    out = []
    for d in (0x2001, 0x10001, 0x89ABCDEF, FULL):   # 4097 itself is 2^-24 from the decision
        hi = nl - 2
        lead = B32 // (d + 1) - 1                    # (lead + 1) d < 2^32: a stays below nl limbs
        for name, digits in (
                ("top", [lead] + [FULL, FULL] + [0x13579BDF] * (hi - 1)),
                ("low", [lead] + [0x2468ACE0 + k for k in range(hi)] + [FULL]),
                ("all", [lead] + [FULL] * (hi + 1))):
            q = from_digits(digits)
            a = d * q + (d - 1)
            assert a < 1 << (32 * nl) and wave_path([(a, d)]) == "short", (name, d)
            tr = {j: (true, sat) for j, true, sat, _ in short_trace(a, d)}
            want = {"top": [hi], "low": [0], "all": list(range(hi + 1))}[name]
            for j in want:
                assert tr[j] == (FULL, True), (name, hex(d), j, tr[j])
            out.append((a, d))
    return out


def rows_short_plain(nl):
    rng = _rng(2)
    out = []
    for d in (1, 2, 4097, FULL):
        for a in (_rand(rng, nl), (1 << (32 * nl)) - 1, _rand(rng, nl - 3), d, d * 0x10000 + (d - 1)):
            if a < d:
                continue
            assert wave_path([(a, d)]) == "short"
            if d <= 2:
                assert not any(sat or fix for _, _, sat, fix in short_trace(a, d))
            out.append((a, d))
    return out


def rows_onedigit(nl):
    """Quotients 1, 2, 2^32 - 3 without and 1, 12345, 2^32 - 4 with the add-back
    (a = b q + (b - 1)).  A quotient 0 is the zero path in a uniform wave; it reaches the
    one-digit path only next to other lanes (waves, below)."""
    rng = _rng(3)
    out = []
    for bl in sorted({2, nl // 2 + 1, nl - 1}):
        b = _rand(rng, bl)
        for q, r, fix in ((1, 0, False), (2, b // 3, False), (B32 - 3, b // 2, False), (0x9E3779B9, 5, False),
                          (1, b - 1, True), (12345, b - 1, True), (B32 - 4, b - 1, True)):
            a = b * q + r
            assert a < 1 << (32 * nl) and wave_path([(a, b)]) == "onedigit"
            assert onedigit_trace(a, b) == (q, False, fix), (hex(a), hex(b))
            out.append((a, b))
    b = _rand(rng, nl, top=1)          # a full-length divisor: a / b < 2^32 - 2 with room
    a = b * 0x7FFF0000 + (b - 1)
    assert a < 1 << (32 * nl) and onedigit_trace(a, b) == (0x7FFF0000, False, True)
    out.append((a, b))
    return out


def rows_general(nl):
    """2-limb, mid-length and full-length divisors.  A full-length divisor leaves a quotient
    below 2^32; it is on the general path when that quotient is 2^32 - 2 or 2^32 - 1."""
    rng = _rng(4)
    out = []
    for bl in (2, nl // 2 + 1):
        for _ in range(3):
            b, a = _rand(rng, bl), _rand(rng, nl, top=0xC0000000 | int(rng.integers(1 << 30)))
            assert wave_path([(a, b)]) == "general"
            assert sum(t["want"] for t in general_trace(a, b)) >= 2
            out.append((a, b))
    b = 1 << (32 * (nl - 1))
    for a in ((1 << (32 * nl)) - 1, b * (B32 - 2) + 12345):
        assert wave_path([(a, b)]) == "general" and limbs(b) == nl
        out.append((a, b))
    return out


def rows_general_boundary(nl):
    """a = b Q + (b - 1) with a digit of Q that is 0xFFFFFFFF under a fraction above
    1 - 2^-12 (estimate >= 2^32: the conversion saturates), and with a digit that is 0 under
    such a fraction (estimate >= 1: executed, found one too large, added back) — each at the
    highest and at the lowest digit the wave executes.  An all-ones digit cannot be the very
    first one executed: under it the digit above has the estimate (2^32 - 1 + f) / 2^32 + 2^-12
    >= 1, so that zero digit is executed first (and added back), the all-ones digit next."""
    rng = _rng(5)
    out = []
    for bl in (2, nl // 2):
        b = _rand(rng, bl, top=0x80000001)
        nq = nl - bl                     # digits of Q that surely fit
        cases = {
            "sat_high": [FULL, FULL] + [0x0F1E2D3C] * (nq - 2),
            "sat_low": [0x7] + [0x5A5A5A5A] * (nq - 2) + [FULL],
            "zero_high": [0x7, 0, FULL] + [0x0BADF00D] * (nq - 3),
            "zero_low": [0x7] + [0x600DCAFE] * (nq - 2) + [0],
        }
        for name, digits in cases.items():
            Q = from_digits(digits)
            a = b * Q + (b - 1)
            assert a < 1 << (32 * nl) and wave_path([(a, b)]) == "general", (name, bl)
            tr = general_trace(a, b)
            ex = [t for t in tr if t["want"]]
            hi, lo = ex[0], ex[-1]
            assert lo["j"] == 0
            if name == "sat_high":
                assert hi["true"] == 0 and hi["addback"]
                assert ex[1]["j"] == hi["j"] - 1 and ex[1]["true"] == FULL and ex[1]["sat"] and not ex[1]["addback"]
            elif name == "sat_low":
                assert lo["true"] == FULL and lo["sat"] and not lo["addback"]
            elif name == "zero_high":
                z = ex[1]               # the digit below the leading 7
                assert z["true"] == 0 and z["addback"] and not z["sat"]
            else:
                assert lo["true"] == 0 and lo["addback"]
            out.append((a, b))
        # the zero digit as the very first one executed: Q's leading digit is the zero
        Q = from_digits([FULL] * (nq - 1))
        a = b * Q + (b - 1)
        tr = [t for t in general_trace(a, b) if t["want"]]
        assert wave_path([(a, b)]) == "general" and tr[0]["true"] == 0 and tr[0]["addback"]
        out.append((a, b))
    return out


FAMILIES = (rows_zero, rows_short_sat, rows_short_plain, rows_onedigit, rows_general, rows_general_boundary)


def all_rows(nl):
    return [(fam.__name__, a, b) for fam in FAMILIES for a, b in fam(nl)]


# ---- mixed waves: 64 lanes, one of them special ---------------------------------------------

WAVES = ("bz_in_general", "lone_high_digit", "lone_low_digit", "lone_addback_onedigit",
         "lone_addback_general", "bhigh_next_to_one_limb", "zeros_and_one_general", "q0_in_onedigit")
POSITIONS = (0, 31, 32, 63)


def _place(others, special, pos):
    lanes = list(others[:63])
    lanes.insert(pos, special)
    assert len(lanes) == 64
    return lanes


def wave_parts(name, nl=8):
    """(the 63 other lanes, the special lane) of a wave over operands of ``nl`` limbs: 8, or 6 —
    below 2^192, non-negative at width 256, so the signed ops hand the divider these very
    operands under every combination of signs."""
    rng = _rng(100 + WAVES.index(name))
    top = 1 << (32 * nl)
    half = nl // 2
    if name == "bz_in_general":
        others = [(_rand(rng, nl), _rand(rng, 2 + i % 4)) for i in range(63)]
        special = (_rand(rng, nl), 0)
    elif name == "lone_high_digit":
        # the others' divisors fill half the limbs: their highest digits are 0; the special
        # lane's one-limb divisor is below its a's top limb: digit nl - 1
        others = [(_rand(rng, nl), _rand(rng, half)) for i in range(63)]
        special = (_rand(rng, nl, top=0xF0000000), 0x10001)
    elif name == "lone_low_digit":
        # the others: a = b (Q << 32) + r with r < b / 2: digit 0 estimates below 1
        others = []
        for i in range(63):
            b = _rand(rng, half - 1)
            others.append((b * (_rand(rng, half - 1) << 32) + b // (2 + i), b))
        b = _rand(rng, half - 1)
        special = (b * ((_rand(rng, half - 1) << 32) + 0x1234567) + 99, b)
    elif name == "lone_addback_onedigit":
        others = []
        for i in range(63):
            b = _rand(rng, 2 + i % (nl - 2))
            others.append((b * int(rng.integers(1, B32 - 3)) + b // (2 + i), b))
        b = _rand(rng, nl - 3)
        special = (b * 0xFEDCBA98 + (b - 1), b)
    elif name == "lone_addback_general":
        others = [(_rand(rng, nl), _rand(rng, 2 + i % 4)) for i in range(63)]
        b = _rand(rng, half - 1)
        special = (b * from_digits([0x31415926, 0x53589793, 0x23846264, 0x33832795]) + (b - 1), b)
    elif name == "bhigh_next_to_one_limb":
        # full-length divisors (b * 2^32j passes nine limbs from j = 10 - nl on) whose lanes must
        # sit out the digits that the one-limb lanes execute above that; the special lane is a
        # one-limb one among 32 of each
        others = [(_rand(rng, nl, top=0xFFFFFFF0 | i % 16), _rand(rng, nl, top=1 + i % 3)) if i % 2 else
                  (_rand(rng, nl), _rand(rng, 1)) for i in range(63)]
        special = (top - 1, 3)
    elif name == "zeros_and_one_general":
        others = []
        for i in range(63):
            b = _rand(rng, 1 + i % nl)
            others.append((0, 0) if i == 7 else (_rand(rng, nl), 0) if i % 9 == 0 else (max(b - 1 - i, 0), b))
        special = (_rand(rng, nl), _rand(rng, 3))
    elif name == "q0_in_onedigit":
        # the quotient 0 on the one-digit path: one a < b lane among one-digit lanes
        others = []
        for i in range(63):
            b = _rand(rng, 2 + i % (nl - 2))
            others.append((b * int(rng.integers(1, B32 - 3)) + b // (3 + i), b))
        b = _rand(rng, nl - 2)
        special = (b - 1, b)
    else:
        raise ValueError(name)
    return others, special


def check_wave(name, lanes, pos, nl=8):
    """Asserts, against the model, what the wave ``name`` is there for: ``lanes`` are 64 (a, b)
    pairs as the divider sees them, the special lane at ``pos`` — the others in any order and
    with repeats (tests/lane_table_cases.py draws them from a table)."""
    assert len(lanes) == 64
    top = 1 << (32 * nl)
    if name == "bz_in_general":
        assert wave_path(lanes) == "general"
        assert all(t["skip"] for t in general_trace(*lanes[pos]))
    elif name == "lone_high_digit":
        assert wave_path(lanes) == "general"
        digs = wave_digits(lanes)
        assert max(digs) == nl - 1 and all(digs[j][0] == [pos] for j in range(nl - 1, nl // 2, -1))
    elif name == "lone_low_digit":
        assert wave_path(lanes) == "general"
        digs = wave_digits(lanes)
        assert min(digs) == 0 and digs[0][0] == [pos] and len(digs[1][0]) == 64
    elif name == "lone_addback_onedigit":
        assert wave_path(lanes) == "onedigit"
        assert [i for i, l in enumerate(lanes) if onedigit_trace(*l)[2]] == [pos]
    elif name == "lone_addback_general":
        assert wave_path(lanes) == "general"
        digs = wave_digits(lanes)
        assert sorted({i for _, fix in digs.values() for i in fix}) == [pos] and digs[0][1] == [pos]
    elif name == "bhigh_next_to_one_limb":
        assert wave_path(lanes) == "general"
        tr = [general_trace(a, b) for a, b in lanes]
        long = [i for i, (a, b) in enumerate(lanes) if limbs(b) == nl]
        assert len(long) >= 31 and all(tr[i][k]["skip"] for i in long for k in range(nl - 2))
        assert all(not tr[i][6]["skip"] and tr[i][7]["want"] for i in long)
        assert sorted(wave_digits(lanes)) == list(range(nl))
        assert limbs(lanes[pos][1]) == 1
    elif name == "zeros_and_one_general":
        assert wave_path(lanes) == "general"
        assert [i for i, l in enumerate(lanes) if not lane_zero(*l)] == [pos]
    elif name == "q0_in_onedigit":
        assert wave_path(lanes) == "onedigit"
        assert onedigit_trace(*lanes[pos]) == (0, False, True)   # fraction (b - 1) / b: add-back to 0
        assert [i for i, (a, b) in enumerate(lanes) if a < b] == [pos]
    else:
        raise ValueError(name)
    assert all(0 <= a < top and 0 <= b < top for a, b in lanes)


def wave(name, pos, nl=8):
    """The 64 (a, b) lanes of a wave with its special lane at ``pos``, checked against the
    model for what the wave is there for."""
    others, special = wave_parts(name, nl)
    lanes = _place(others, special, pos)
    check_wave(name, lanes, pos, nl)
    return lanes
