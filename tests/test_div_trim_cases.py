"""The operands of tests/test_gpu_div_trim.py reach the divider paths and digits they are meant
for: div_trim_cases.py's model of pf::udivrem256 in Python integers, checked without a GPU, and
the model itself against plain integer division."""

import div_trim_cases as C
import pytest


@pytest.mark.parametrize("nl", [8, 6])
def test_rows_reach_their_paths(nl):
    rows = C.all_rows(nl)                       # every builder asserts its own cases
    paths = {}
    for fam, a, b in rows:
        assert 0 <= a < 1 << (32 * nl) and 0 <= b < 1 << (32 * nl)
        paths.setdefault(C.wave_path([(a, b)]), set()).add(fam)
    assert paths["zero"] == {"rows_zero"}
    assert paths["short"] == {"rows_short_sat", "rows_short_plain"}
    assert paths["onedigit"] == {"rows_onedigit"}
    assert paths["general"] == {"rows_general", "rows_general_boundary"}
    # the saturating conversion is reached on the short and on the general path, and both
    # add-back branches are
    assert any(sat for _, a, b in rows if C.wave_path([(a, b)]) == "short" and b > 4097
               for _, _, sat, _ in C.short_trace(a, b))
    gen = [C.general_trace(a, b) for _, a, b in rows if C.wave_path([(a, b)]) == "general"]
    assert any(t["sat"] for tr in gen for t in tr) and any(t["addback"] for tr in gen for t in tr)
    assert any(C.onedigit_trace(a, b)[2] for _, a, b in rows if C.wave_path([(a, b)]) == "onedigit")
    # divisor lengths on the general path: 2 limbs, mid-length, full length
    assert {C.limbs(b) for fam, a, b in rows if fam == "rows_general"} == {2, nl // 2 + 1, nl}


@pytest.mark.parametrize("name", C.WAVES)
def test_waves_reach_their_paths(name):
    seen = set()
    for pos in C.POSITIONS:
        lanes = C.wave(name, pos)               # asserts what the wave is there for
        assert len(lanes) == 64
        seen.add(lanes[pos])
    assert len(seen) == 1                       # the same special lane, moved


def test_model_divides():
    """The traces end on the true quotient and remainder for every general-path row and lane."""
    for nl in (8, 6):
        for _, a, b in C.all_rows(nl):
            if b and C.wave_path([(a, b)]) == "general":
                tr = C.general_trace(a, b)      # asserts the remainder
                assert C.from_digits([t["true"] for t in tr]) == a // b
            if b and b != 4097 and C.wave_path([(a, b)]) == "short":   # 4097: 2^-24 from a decision
                assert C.from_digits([t for _, t, _, _ in C.short_trace(a, b)]) == a // b
