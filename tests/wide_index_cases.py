"""Case builder: array reads with 512-bit indices, in the shape the reference builds for
EIP-1153 transient storage (mythril/laser/ethereum/state/transient_storage.py:21-50) —

    select(store(... store(K(512 -> 256, 0), key_1, v_1) ..., key_n, v_n), Concat(addr, slot))

Every case is (name, constraints, "sat" | "unsat").  Shared by tests/test_wide_index.py (the C
oracle engine) and tests/test_gpu_wide_index.py (the MI355X).  ``a b i j v w`` are 256-bit
symbols, ``A1 != A2`` address constants, ``X`` a free 512-bit key.
"""

from mythril_amd.smt import terms as T

A1 = T.const(0xAFFEAFFEAFFEAFFEAFFEAFFEAFFEAFFEAFFEAFFE, 256)
A2 = T.const(0xDEADBEEFDEADBEEFDEADBEEFDEADBEEFDEADBEEF, 256)
a, b, i, j, v, w = (T.var(n, 256) for n in "abijvw")
X = T.var("X", 512)
ZERO = T.const(0, 256)
K0 = T.const_array(512, ZERO)


def key(addr, slot):
    return T.concat(addr, slot if isinstance(slot, T.Term) else T.const(slot, 256))


def ne(x, y):
    return T.not_(T.eq(x, y))


def journal(stores, base=K0):
    arr = base
    for k, val in stores:
        arr = T.store(arr, k, val)
    return arr


def _vals(n):
    return [T.var(f"v{k}", 256) for k in range(n)]


def journal3():
    v0, v1, v2 = _vals(3)
    return journal([(key(A1, 1), v0), (X, v1), (key(A1, i), v2)]), (v0, v1, v2)


def journal8():
    vs = _vals(8)
    keys = [key(A1, 0), key(A1, i), X, T.binop("bvadd", X, T.const(1 << 256, 512)), key(A2, j),
            key(A1, 2), key(a, 3), key(A1, j)]
    return journal(list(zip(keys, vs))), vs


def free_key_journal():
    """Eight stores at free 512-bit keys, read at two more: every link of either chain
    compares both chunks of two symbols, and the second read meets the first one's 16 key
    chunks again — the case built to need the 16-register kernels (over 7 registers a third
    of its program would be spill code, so the lowering takes the wide file)."""
    keys = [T.var(f"X{k}", 512) for k in range(8)]
    vs = _vals(8)
    arr = journal(list(zip(keys, vs)))
    picks = (3, 5)
    Ys = [T.var(f"Y{n}", 512) for n in range(len(picks))]
    out = [T.eq(Y, keys[p]) for Y, p in zip(Ys, picks)]
    for Y, p in zip(Ys, picks):
        out += [T.eq(T.select(arr, Y), vs[p]), ne(vs[p], ZERO)]
    return out


def cases():
    out = []

    def add(name, cs, label):
        out.append((name, list(cs), label))

    # 1. the empty journal
    r = T.select(K0, key(A1, i))
    add("empty_sat", [T.eq(r, ZERO)], "sat")
    add("empty_unsat", [ne(r, ZERO)], "unsat")
    # 2. one store, read at another slot of the same address
    r = T.select(journal([(key(A1, i), v)]), key(A1, j))
    add("one_store_hit", [T.eq(r, v), ne(v, ZERO)], "sat")         # needs i == j
    add("one_store_miss", [T.eq(r, ZERO), ne(v, ZERO)], "sat")     # needs i != j
    # 3. both chunks matter
    add("chunks_addr_const", [ne(T.select(journal([(key(A1, i), v)]), key(A2, i)), ZERO)], "unsat")
    add("chunks_slot_const", [ne(T.select(journal([(key(a, 5), v)]), key(a, 6)), ZERO)], "unsat")
    add("chunks_addr_sym", [ne(a, b), ne(T.select(journal([(key(a, i), v)]), key(b, i)), ZERO)], "unsat")
    add("chunks_slot_sym", [ne(i, j), ne(T.select(journal([(key(a, i), v)]), key(a, j)), ZERO)], "unsat")
    add("chunks_addr_sym_sat", [T.eq(a, b), ne(v, ZERO),
                                T.eq(T.select(journal([(key(a, i), v)]), key(b, i)), v)], "sat")
    # 4. the last store wins
    k1, k2 = key(A1, i), key(A1, j)
    r = T.select(journal([(k1, v), (k2, w)]), k1)
    add("last_store_unsat", [T.eq(i, j), ne(v, w), T.eq(r, v)], "unsat")
    add("last_store_sat", [T.eq(i, j), ne(v, w), T.eq(r, w)], "sat")
    # 5. journals of 3 and 8 stores
    j3, (v0, v1, v2) = journal3()
    r = T.select(j3, key(A1, 1))
    add("journal3_sat", [T.eq(r, v0), ne(v0, v1), ne(v0, v2)], "sat")
    add("journal3_unsat", [ne(i, T.const(1, 256)), ne(X, key(A1, 1)), ne(r, v0)], "unsat")
    add("journal3_free_key", [T.eq(T.select(j3, X), v1), ne(v1, v2), ne(v1, ZERO)], "sat")
    j8, vs = journal8()
    r = T.select(j8, key(A1, 2))
    add("journal8_sat", [T.eq(r, vs[5]), ne(vs[5], vs[7]), ne(vs[5], ZERO)], "sat")
    add("journal8_unsat", [ne(j, T.const(2, 256)), ne(r, vs[5])], "unsat")
    r = T.select(j8, T.binop("bvadd", X, T.const(1 << 256, 512)))
    add("journal8_offset_key", [T.eq(r, vs[3]), ne(vs[3], vs[4]), ne(vs[3], vs[6]), ne(vs[3], vs[7]),
                                ne(vs[3], ZERO)], "sat")
    # 6. a base array variable with a 512-bit domain
    ts = T.array("ts", 512, 256)
    add("base_equal_unsat", [T.eq(i, j), ne(T.select(ts, key(A1, i)), T.select(ts, key(A1, j)))], "unsat")
    add("base_high_chunk_sat", [ne(a, b), ne(T.select(ts, key(a, i)), T.select(ts, key(b, i)))], "sat")
    add("base_over_journal", [T.eq(T.select(journal([(key(A1, i), v)], ts), key(A1, 7)), T.const(9, 256)),
                              T.eq(T.select(ts, key(A1, 7)), T.const(4, 256))], "sat")   # needs i == 7, v == 9
    add("base_const_index", [T.eq(T.select(ts, T.const((5 << 256) | 7, 512)), T.const(3, 256)),
                             T.eq(T.select(ts, X), T.const(4, 256))], "sat")
    # 7. an ite between two wide-index arrays
    arr = T.ite(T.cmp("bvult", a, b), journal([(key(A1, i), v)]), journal([(key(A1, j), w)]))
    r = T.select(arr, key(A1, i))
    add("ite_sat", [T.cmp("bvult", a, b), T.eq(r, v), ne(v, ZERO)], "sat")
    add("ite_unsat", [T.cmp("bvult", a, b), ne(r, v)], "unsat")
    # 8. a 512 -> 8 array; and a byte array whose name and width look like calldata bytes
    K8 = T.const_array(512, T.const(0, 8))
    r = T.select(T.store(K8, key(A1, i), T.extract(7, 0, v)), key(A1, j))
    add("byte_range_sat", [T.eq(i, j), T.eq(r, T.const(0x5A, 8))], "sat")
    add("byte_range_unsat", [ne(i, j), ne(r, T.const(0, 8))], "unsat")
    cd = T.array("1_calldata", 512, 8)
    add("byte_base_named_calldata", [T.eq(T.select(cd, T.const((1 << 300) | 5, 512)), T.const(3, 8)),
                                     T.eq(T.select(cd, key(A1, i)), T.const(4, 8))], "sat")
    return out

