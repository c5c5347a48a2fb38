"""The launch half of the host driver that makes no HIP call (mythril_amd/csrc/pf_launch.h: request
checks, launch orders, launch geometry, the counter sum, the block alignment) through
tests/host_launch_check.cpp, built with the address and undefined-behaviour sanitizers and run as a
child process:

* the geometry reproduces every row of tests/host_launch_geometry.txt, the table the host driver
  printed before these rules moved into the header — a slip in them changes speed, not results, so
  no GPU test would see it;
* every rejection of a request stands beside the nearest accepted one, with the entry points'
  messages;
* the two launch orders on a batch whose wave order is not the identity;
* the counter sum over lines with a distinct value in every (stripe, slot).

CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_launch_check.cpp")
TABLE = os.path.join(ROOT, "tests", "host_launch_geometry.txt")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(CLANG), "the host clang++ is needed to build tests/host_launch_check.cpp"
    out = str(tmp_path_factory.mktemp("host_launch") / "host_launch_check")
    # the sanitizers' runtimes are linked into the program itself: it runs as it is
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, SRC], check=True)
    return out


def run(exe, *args, ok=(0,)):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert p.stderr == "" and p.returncode in ok, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout.rstrip("\n")


# ---- geometry: the table of the commit before the move -----------------------------------------

def _rows():
    with open(TABLE) as f:
        return [line.split() for line in f if line.strip() and not line.startswith("#")]


def test_the_table_covers_the_grid():
    rows = _rows()
    cus, sets = {"4", "256"}, {"1", "2", "3", "64", "65", "1024", "4608", "65536"}
    budgets = {"1", "63", "64", "65", "128", "200", "2048", "65472", "65536"}
    search = [r for r in rows if r[0] == "C"]
    stream = [r for r in rows if r[0] == "S" and r[3] != "4294967295"]
    side = [r for r in rows if r[0] == "K" and r[3] != "4294967295"]
    # every (num_cus, sets, budget) in both knob settings: the full sweep once, the early-exit search for
    # every (all_parented, PF_FLAG_NO_PROBE, probe_max_sets in {0, 64}); stream with no override, 1 and 2
    assert {(r[1], r[2], r[3]) for r in search} == {(c, s, b) for c in cus for s in sets for b in budgets}
    assert len(search) == 2 * 8 * 9 * 2 * (1 + 8) and {r[8] for r in search} == {"0", "1"}
    assert {(r[4], r[5], r[6], r[7]) for r in search if r[4] == "1"} == {
        ("1", a, n, m) for a in "01" for n in "01" for m in ("0", "64")}
    assert len(stream) == 2 * 8 * 9 * 2 * 3 and {r[5] for r in stream} == {"0", "1", "2"}
    assert len(side) == 2 * 8 * 9 * 2
    # the probe launches and does not, and the phase behind it starts at candidate 64
    assert {r[-1] for r in search} == {"0", "1"}
    # item counts that no longer fit 32 bits are on record as rejected, beside the largest that fit
    big = [r for r in rows if r[3] == "4294967295"]
    assert {(r[0], r[2], r[-1]) for r in big} == {("S", "65536", "1"), ("K", "65536", "1"), ("S", "63", "0"),
                                                  ("K", "63", "0")}
    assert any(r[0] == "K" and int(r[6]) > 0xffffffff for r in big)      # items
    assert any(r[0] == "S" and int(r[7]) > 0xffffffff for r in big)
    # the probe launch's own geometry, at every set count at which a probe runs
    probes = [r for r in rows if r[0] == "P"]
    assert {(r[1], r[2], r[3]) for r in probes} == {(c, s, k) for c in cus for s in ("2", "3", "64") for k in "01"}
    assert len(rows) == len(search) + len(stream) + len(side) + len(big) + len(probes)


def test_geometry_reproduces_the_table(exe):
    assert run(exe, "geometry", TABLE) == f"rows {len(_rows())}"


def test_a_changed_row_is_seen(exe, tmp_path):
    """The comparison itself: one figure of one row changed, and that row is reported."""
    lines = open(TABLE).read().splitlines()
    at = next(i for i, l in enumerate(lines) if l.startswith("C 256 1024 65536 0 "))
    f = lines[at].split()
    f[9] = str(int(f[9]) + 1)                      # slices
    lines[at] = " ".join(f)
    bad = tmp_path / "table.txt"
    bad.write_text("\n".join(lines) + "\n")
    out = run(exe, "geometry", bad, ok=(1,))
    assert out.splitlines()[0] == "table: " + lines[at] and out.splitlines()[-1] == f"rows {len(_rows())}"


# ---- request checks: each rejection beside the nearest accepted request -------------------------

# who, sets in the batch, the caller's own bound (a set above it fails the caller's condition; "-": a
# caller without one), the accepted request, the rejected one, its message; ("null", n): a null
# set_ids of n entries
REQUESTS = [
    ("pf_climb_batch", 4, "-", ("null", 0), ("null", 1), "pf_climb_batch: null set_ids"),
    ("pf_census_batch", 4, 9, [3], [4], "pf_census_batch: set 4 out of range (4 sets)"),
    ("pf_eval_batch", 1, "-", [0], [1], "pf_eval_batch: set 1 out of range (1 sets)"),
    ("pf_eval_batch_dev", 4, "-", [0, 1, 2, 3], [0, 1, 2, 4294967295],
     "pf_eval_batch_dev: set 4294967295 out of range (4 sets)"),
    ("pf_climb_batch", 4, "-", [1, 0], [1, 1], "pf_climb_batch: set 1 requested twice"),
    ("pf_census_batch", 4, 9, [3, 0, 1, 2], [3, 0, 1, 3], "pf_census_batch: set 3 requested twice"),
    ("pf_eval_batch", 0, "-", [], [0], "pf_eval_batch: set 0 out of range (0 sets)"),
    # the caller's condition is asked after the two common ones, of every set
    ("pf_census_batch", 4, 2, [2, 0], [2, 3], "pf_census_batch: set 3 is too large"),
    ("pf_census_batch", 4, 2, [2, 0], [2, 4], "pf_census_batch: set 4 out of range (4 sets)"),
    ("pf_census_batch", 4, 0, [0], [1, 1], "pf_census_batch: set 1 is too large"),     # before its repeat is seen
    ("pf_census_batch", 4, 1, [1, 0], [1, 1], "pf_census_batch: set 1 requested twice"),
]


def _request(exe, who, n_sets, bound, ids):
    args = ["none"] if ids == [] else list(ids)
    return run(exe, "request", who, n_sets, bound, *args)


@pytest.mark.parametrize("who,n_sets,bound,good,bad,message", REQUESTS, ids=[r[5] for r in REQUESTS])
def test_request_rejections(exe, who, n_sets, bound, good, bad, message):
    assert _request(exe, who, n_sets, bound, good) == "ok"
    assert _request(exe, who, n_sets, bound, bad) == message


def test_an_empty_request_is_accepted(exe):
    assert _request(exe, "pf_climb_batch", 4, "-", []) == "ok"            # n == 0, set_ids not null
    assert _request(exe, "pf_climb_batch", 4, "-", ("null", 0)) == "ok"   # n == 0, set_ids null
    assert _request(exe, "pf_climb_batch", 0, "-", []) == "ok"            # and a batch without sets


# ---- launch orders -----------------------------------------------------------------------------

def test_launch_orders(exe):
    wide = [0, 1, 0, 1, 0, 0]
    order = [4, 0, 5, 2, 3, 1]                     # narrow first, not the identity within either part
    request = [5, 1, 0, 3]
    csv = lambda v: ",".join(map(str, v))
    out = run(exe, "order", csv(wide), csv(order), csv(request)).splitlines()
    # climb, census: request order within each register file, narrow first
    assert out[0] == "request: 5,0,1,3 n_narrow 2"
    # stream: the batch's wave order, and each set's place in the request
    sets = [s for s in order if s in request]
    assert sets == [0, 5, 3, 1]
    places = [request.index(s) for s in sets]
    assert out[1] == f"batch: {csv(sets)} places {csv(places)} n_narrow 2"
    assert [request[p] for p in places] == sets    # the place table inverts the request
    # every set, in request order already: both rules agree only on n_narrow
    out = run(exe, "order", csv(wide), csv(order), csv(range(6))).splitlines()
    assert out == ["request: 0,2,4,5,1,3 n_narrow 4", "batch: 4,0,5,2,3,1 places 4,0,5,2,3,1 n_narrow 4"]
    # wide sets alone
    out = run(exe, "order", csv(wide), csv(order), "3,1").splitlines()
    assert out == ["request: 3,1 n_narrow 0", "batch: 3,1 places 0,1 n_narrow 0"]


# ---- counter sum, alignment --------------------------------------------------------------------

def test_counter_sum(exe):
    stripes = 16                                    # PF_COUNTER_STRIPES (the program asserts the line size)
    want = [sum(1000 * i + 10 * k + 1 for i in range(stripes)) for k in range(5)]
    assert run(exe, "counters") == " ".join(map(str, want))


def test_alignment(exe):
    assert run(exe, "al") == "0 256 256 256 512 4294967552"
