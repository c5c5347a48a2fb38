"""The host half of pf_batch_create (mythril_amd/csrc/pf_devprog.h: the validator, the device
program rewrites and the threaded preparation) through tests/devprog_host_check.cpp, built once
with the address and undefined-behaviour sanitizers and once with the thread sanitizer, and run
as a child process:

* every rejection of the validator, each beside the nearest well-formed batch, with the same
  message from the check program and from pf_batch_create of the built library (which validates
  before it touches a device);
* the check program's code, descriptors and pool equal pf_device_program's and
  pf_device_batch's, for PF_DEVICE_FOLD 0, 1 and 2;
* a batch large enough for host threads gets byte for byte what the single range gets, and so
  does one whose descriptors share and reorder code ranges, which takes the serial path.

CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mythril_amd import _lib, ir, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "devprog_host_check.cpp")
CLANG = "/opt/rocm/llvm/bin/clang++"
SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    assert os.path.exists(CLANG), "the host clang++ is needed to build tests/devprog_host_check.cpp"
    d = tmp_path_factory.mktemp("devprog")
    out = {}
    for name, flags in SANITIZERS.items():
        # the sanitizers' runtimes are linked into the program itself: it runs as it is
        out[name] = str(d / f"devprog_host_check_{name}")
        subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-pthread", *flags, "-o", out[name], SRC], check=True)
    return out


class Packed:
    """The arrays of one batch as pf_batch_create takes them (parents: only their count)."""

    def __init__(self, code, consts, schema, descs, n_parents):
        self.code = np.array(code, dtype=np.uint32).reshape(-1, 4)
        self.consts = np.array(consts, dtype=np.uint32).reshape(-1, 8)
        self.schema = np.array(schema, dtype=np.uint32).reshape(-1, 4)
        self.descs = np.array(descs, dtype=np.uint32).reshape(-1, 8)
        self.n_parents = n_parents

    @classmethod
    def of(cls, batch):
        return cls(batch.code, batch.consts, batch.schema, batch.descs, len(batch.parents))

    def copy(self):
        return Packed(self.code, self.consts, self.schema, self.descs, self.n_parents)

    def write(self, path):
        with open(path, "wb") as f:
            np.array([len(self.code), len(self.consts), len(self.schema), self.n_parents, len(self.descs)],
                     dtype=np.uint64).tofile(f)
            for a in (self.code, self.consts, self.schema, self.descs):
                a.tofile(f)


def run(exe, packed, tmp_path, fold=1, ranges="own", mode="batch"):
    """(message, None) of a rejected batch, else (None, (code, descs, pool, ranges used))."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    packed.write(src)
    p = subprocess.run([exe, src, dst, str(fold), ranges, mode], capture_output=True, text=True, timeout=300)
    assert p.stderr == "" and p.returncode in (0, 1), (p.returncode, p.stderr[-3000:])
    if p.returncode:
        return p.stdout.rstrip("\n"), None
    with open(dst, "rb") as f:
        n_ins, n_sets, n_pool = (int(x) for x in np.fromfile(f, dtype=np.uint64, count=3))
        code = np.fromfile(f, dtype=np.uint32, count=4 * n_ins).reshape(-1, 4)
        descs = np.fromfile(f, dtype=np.uint32, count=8 * n_sets).reshape(-1, 8)
        pool = np.fromfile(f, dtype=np.uint32, count=8 * n_pool).reshape(-1, 8)
        assert f.read() == b""
    return None, (code, descs, pool, int(p.stdout.split()[1]))


def same(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a[:3], b[:3]))


# ---- the validator ------------------------------------------------------------------------

def _prog(build, consts=(), vars=()):
    p = ir.Program(name="devprog")
    p.consts.extend(consts)
    p.vars.extend(vars)
    build(p)
    return Packed.of(ir.Batch([p.finish()]))


def _var(width=8, kind=ir.VK_GENERIC, hint0=0, hint1=0, parent=None):
    return ir.Var("v", width, kind, hint0, hint1, parent)


def _wvar(p):                                  # W_VAR r0; END
    p.emit(ir.W_VAR, 8, dst=0, aux0=0)


def _bvars(n):
    def build(p):
        for k in range(n):
            p.emit(ir.B_VAR, 1, dst=k, aux0=0)
    return build


def _then(first, *ins):
    """``first`` and then the instructions ``(op, width, fields)``."""
    def build(p):
        first(p)
        for op, w, kw in ins:
            p.emit(op, w, **kw)
    return build


def _set(array, row, col, value=None, shift=0, bits=32, add=None):
    """A mutation: the ``bits``-wide field at ``shift`` of array[row, col] set to value (or
    increased by ``add``)."""
    def mutate(b):
        a = getattr(b, array)
        mask = ((1 << bits) - 1) << shift
        old = (int(a[row, col]) & mask) >> shift
        new = value if add is None else old + add
        a[row, col] = (int(a[row, col]) & ~mask) | ((new << shift) & mask)
    return mutate


WIDTH = dict(col=0, shift=8, bits=10)
DST, RA, RB, RC = (dict(col=1, shift=s, bits=8) for s in (0, 8, 16, 24))
BOOL1 = [_var(1, ir.VK_BOOL)]
W_THEN_B = _then(_wvar, (ir.B_VAR, 1, dict(dst=0, aux0=1)), (ir.W_ITE, 8, dict(dst=1, a=0, b=0, c=0)))
B_ITE = _then(_bvars(1), (ir.B_ITE, 1, dict(dst=1, a=0, b=0, c=0)))
SPILL_FILL = _then(_wvar, (ir.W_SPILL, 8, dict(a=0, aux0=3)), (ir.W_FILL, 8, dict(dst=1, aux0=3)))
FIVE = [1, 2, 3, 4, 5]

# name, the well-formed batch, what makes it malformed, the validator's message
REJECTIONS = [
    ("code range past the end", _prog(_wvar, vars=[_var()]), _set("descs", 0, 1, add=1),
     "set 0: code range [0,+3) outside 2 instructions"),
    ("n_ins == 0", _prog(_wvar, vars=[_var()]), _set("descs", 0, 1, 0),
     "set 0: code range [0,+0) outside 2 instructions"),
    ("constant range outside the pool", _prog(_wvar, consts=[7], vars=[_var()]), _set("descs", 0, 3, add=1),
     "set 0: constant range outside pool"),
    ("schema range outside", _prog(_wvar, vars=[_var()]), _set("descs", 0, 5, add=1), "set 0: schema range outside"),
    ("no final PF_END", _prog(_then(_wvar, (ir.W_NOT, 8, dict(dst=1, a=0))), vars=[_var()]),
     _set("descs", 0, 1, add=-1), "set 0: program does not end with PF_END"),
    ("width 0", _prog(_wvar, vars=[_var()]), _set("code", 0, value=0, **WIDTH), "set 0 ins 0: width 0 out of range"),
    ("width 257", _prog(_wvar, vars=[_var()]), _set("code", 0, value=257, **WIDTH),
     "set 0 ins 0: width 257 out of range"),
    ("variable index = n_vars", _prog(_wvar, vars=[_var()]), _set("code", 0, 2, 1), "set 0 ins 0: variable 1 >= 1"),
    ("constant index = n_const", _prog(lambda p: p.emit(ir.W_CONST, 8, dst=0, aux0=0), consts=[7]),
     _set("code", 0, 2, 1), "set 0 ins 0: constant 1 >= 1"),
    ("schema width 0", _prog(_wvar, vars=[_var()]), _set("schema", 0, 0, 0, shift=8, bits=10), "set 0 var 0: width 0"),
    ("parent slot = n_parents", _prog(_wvar, vars=[_var(parent=5)]), _set("schema", 0, 3, 1),
     "set 0 var 0: parent slot"),
    ("keccak base outside the pool", _prog(_wvar, consts=[7], vars=[_var(256, ir.VK_KECCAK, 0)]),
     _set("schema", 0, 1, 1), "set 0 var 0: keccak base"),
    ("actor table of 5 entries", _prog(_wvar, consts=FIVE, vars=[_var(160, ir.VK_ACTOR, 0, 4)]),
     _set("schema", 0, 2, 5), "set 0 var 0: actor table"),
    ("actor table past the pool", _prog(_wvar, consts=FIVE, vars=[_var(160, ir.VK_ACTOR, 1, 4)]),
     _set("schema", 0, 1, 2), "set 0 var 0: actor table"),
    ("calldata byte at an unaligned bit", _prog(_wvar, consts=FIVE, vars=[_var(8, ir.VK_CDBYTE, 8, 7)]),
     _set("schema", 0, 1, 9), "set 0 var 0: calldata word constants"),
    ("calldata word constants past the pool",
     _prog(_wvar, consts=FIVE, vars=[_var(8, ir.VK_CDBYTE, 8 | 3 << 8 | 2 << 20, 7)]),
     _set("schema", 0, 1, 8 | 4 << 8 | 2 << 20), "set 0 var 0: calldata word constants"),
    ("W destination = PF_NW", _prog(_wvar, vars=[_var()]), _set("code", 0, value=ir.NW, **DST), "set 0 ins 0: W dst 15"),
    ("operand a read before written", _prog(_then(_wvar, (ir.W_NOT, 8, dict(dst=1, a=0))), vars=[_var()]),
     _set("code", 1, value=2, **RA), "set 0 ins 1: W register read before write"),
    ("operand b read before written", _prog(_then(_wvar, (ir.W_ADD, 8, dict(dst=1, a=0, b=0))), vars=[_var()]),
     _set("code", 1, value=3, **RB), "set 0 ins 1: W register read before write"),
    ("B_AND of an unwritten B register", _prog(_then(_bvars(2), (ir.B_AND, 1, dict(dst=2, a=0, b=1))), vars=BOOL1),
     _set("code", 2, value=5, **RA), "set 0 ins 2: B register read before write"),
    ("B_NOT of an unwritten B register", _prog(_then(_bvars(1), (ir.B_NOT, 1, dict(dst=1, a=0))), vars=BOOL1),
     _set("code", 1, value=5, **RA), "set 0 ins 1: B register read before write"),
    ("PF_ASSERT of an unwritten B register", _prog(_then(_bvars(1), (ir.ASSERT, 1, dict(a=0))), vars=BOOL1),
     _set("code", 1, value=5, **RA), "set 0 ins 1: B register read before write"),
    ("B_SPILL of an unwritten B register", _prog(_then(_bvars(1), (ir.B_SPILL, 1, dict(a=0, aux0=0))), vars=BOOL1),
     _set("code", 1, value=5, **RA), "set 0 ins 1: B register read before write"),
    ("W_ITE on an unwritten condition", _prog(W_THEN_B, vars=[_var(), _var(1, ir.VK_BOOL)]),
     _set("code", 2, value=7, **RC), "set 0 ins 2: B register read before write"),
    ("B_ITE with operand a unwritten", _prog(B_ITE, vars=BOOL1), _set("code", 1, value=7, **RA),
     "set 0 ins 1: B register read before write"),
    ("B_ITE with operand b unwritten", _prog(B_ITE, vars=BOOL1), _set("code", 1, value=7, **RB),
     "set 0 ins 1: B register read before write"),
    ("B_ITE with the condition unwritten", _prog(B_ITE, vars=BOOL1), _set("code", 1, value=7, **RC),
     "set 0 ins 1: B register read before write"),
    ("spill slot 64", _prog(_then(_wvar, (ir.W_SPILL, 8, dict(a=0, aux0=3))), vars=[_var()]),
     _set("code", 1, 2, ir.MAX_SPILL), "set 0 ins 1: spill slot 64 >= 64"),
    ("fill of a slot never spilled", _prog(SPILL_FILL, vars=[_var()]), _set("code", 2, 2, 4),
     "set 0 ins 2: spill slot 4 filled before it was spilled"),
]


def _batch_create_error(b):
    L = _lib.lib()
    parents = np.zeros((max(b.n_parents, 1), 8), dtype=np.uint32)
    handle = ctypes.c_uint64(0)
    rc = L.pf_batch_create(_lib.ptr_u32(b.code), len(b.code), _lib.ptr_u32(b.consts) if len(b.consts) else None,
                           len(b.consts), _lib.ptr_u32(b.schema) if len(b.schema) else None, len(b.schema),
                           _lib.ptr_u32(parents), b.n_parents, _lib.ptr_u32(b.descs), len(b.descs),
                           ctypes.byref(handle))
    assert rc != 0 and handle.value == 0
    return L.pf_last_error().decode()


@pytest.mark.parametrize("name,good,mutate,message", REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_validator_rejects(exes, tmp_path, name, good, mutate, message):
    assert 2 <= len(good.code) <= 4
    err, out = run(exes["asan"], good, tmp_path)
    assert err is None and len(out[0]) >= 1, err
    bad = good.copy()
    mutate(bad)
    assert run(exes["asan"], bad, tmp_path) == (message, None)
    assert _batch_create_error(bad) == message


# ---- the same program as the library's ---------------------------------------------------------

@pytest.mark.parametrize("fold", [0, 1, 2])
def test_check_program_equals_the_library(exes, tmp_path, monkeypatch, fold):
    import test_device_program as TDP

    batch = ir.Batch(TDP._programs(monkeypatch))
    b = Packed.of(batch)
    monkeypatch.setenv("PF_DEVICE_FOLD", str(fold))
    code, descs = TDP.device_program(batch)
    err, got = run(exes["asan"], b, tmp_path, fold, mode="program")
    assert err is None and same(got, (code, descs, b.consts))
    err, got = run(exes["asan"], b, tmp_path, fold)
    assert err is None and same(got, _lib.device_batch(batch.code, batch.consts, batch.descs))
    assert fold == 0 or len(got[2]) > len(b.consts)      # constants of the programs' own: the device pool


# ---- threaded = serial -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def large():
    b = Packed.of(ir.Batch([synth.random_dag_set(i, plant=(i % 2 == 0))[0] for i in range(1024)]))
    assert len(b.descs) >= 64 and len(b.code) >= 1 << 15
    return b


def test_threaded_ranges_equal_the_single_range(exes, tmp_path, large):
    err, single = run(exes["asan"], large, tmp_path, ranges="single")
    assert err is None and single[3] == 1 and len(single[2]) > len(large.consts)
    for name in ("asan", "tsan"):
        err, own = run(exes[name], large, tmp_path)
        assert err is None and same(own, single), name
        assert own[3] > 1 or (os.cpu_count() or 1) == 1, "the driver cut no ranges"
        err, prog = run(exes[name], large, tmp_path, mode="program")
        assert err is None and same(prog, run(exes["asan"], large, tmp_path, ranges="single", mode="program")[1])


def test_shared_and_reordered_code_ranges_take_the_serial_path(exes, tmp_path, large):
    b = large.copy()
    b.descs[10] = b.descs[900]                    # two descriptors, far enough apart for two host
    b.descs[[300, 700]] = b.descs[[700, 300]]     # threads, share one code range; two are swapped
    err, single = run(exes["asan"], b, tmp_path, ranges="single")
    assert err is None
    for name in ("asan", "tsan"):
        err, own = run(exes[name], b, tmp_path)
        assert err is None and own[3] == 1 and same(own, single), name
    s = single[1]
    n, m = int(s[10][1]), int(s[900][1])          # the shared range was rewritten once per descriptor
    assert n == m and (single[0][s[10][0]:s[10][0] + n] == single[0][s[900][0]:s[900][0] + m]).all()
