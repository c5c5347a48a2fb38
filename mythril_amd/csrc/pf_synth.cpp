// pf_synth.cpp — libpflower.so: BASELINE config 3's synthetic DAGs natively (pflt_synth of
// include/pf_lower.h): mythril_amd/synth.py:random_dag_set bit for bit, built straight into a
// Dag (pf_dag.h) and lowered by emit_program.  The benchmark's workload generator, not part
// of the term lowering (pf_terms.cpp), with which it shares pf_dag.h alone.  The planted
// values are the host evaluator's (pf_hostint.h eval_op at w = 256); synth.py:_eval is the
// Python statement tests/test_synth_native.py compares them with.  Host code, no HIP.
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "pf_dag.h"

using namespace pf_dag;
using pf_host::U;

namespace {

// numpy's Philox4x64-10 bit generator and the Generator draws random_dag_set makes: random()
// (53-bit double from next_uint64), integers(lo, hi) for int64 (Lemire on next_uint32, which
// uses both halves of a 64-bit output in turn) and integers(0, 2^32, size=8, dtype=uint64)
// (eight next_uint32).  Checked against numpy draw for draw (tests/test_synth_native.py).
struct NpPhilox {
    uint64_t ctr[4] = {0, 0, 0, 0}, key[2], buf[4] = {0, 0, 0, 0};
    int pos = 4;
    bool has32 = false;
    uint32_t u32 = 0;

    explicit NpPhilox(unsigned __int128 k) {
        key[0] = (uint64_t)k;
        key[1] = (uint64_t)(k >> 64);
    }
    static void mulhilo(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
        const unsigned __int128 p = (unsigned __int128)a * b;
        *hi = (uint64_t)(p >> 64);
        *lo = (uint64_t)p;
    }
    uint64_t next64() {
        if (pos < 4) return buf[pos++];
        if (++ctr[0] == 0 && ++ctr[1] == 0 && ++ctr[2] == 0) ++ctr[3];
        uint64_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k0 = key[0], k1 = key[1];
        for (int r = 0; r < 10; r++) {
            uint64_t hi0, lo0, hi1, lo1;
            mulhilo(0xD2E7470EE14C6C93ull, c[0], &hi0, &lo0);
            mulhilo(0xCA5A826395121157ull, c[2], &hi1, &lo1);
            const uint64_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
            c[0] = n0;
            c[1] = lo1;
            c[2] = n2;
            c[3] = lo0;
            k0 += 0x9E3779B97F4A7C15ull;
            k1 += 0xBB67AE8584CAA73Bull;
        }
        for (int i = 0; i < 4; i++) buf[i] = c[i];
        pos = 1;
        return buf[0];
    }
    uint32_t next32() {
        if (has32) {
            has32 = false;
            return u32;
        }
        const uint64_t v = next64();
        has32 = true;
        u32 = (uint32_t)(v >> 32);
        return (uint32_t)v;
    }
    double random() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
    int64_t integers(int64_t lo, int64_t hi) {  // [lo, hi), range < 2^32
        const uint64_t rng = (uint64_t)(hi - lo - 1);
        if (rng == 0) return lo;
        if (rng == 0xFFFFFFFFull) return lo + next32();
        const uint32_t rexcl = (uint32_t)rng + 1u;
        uint64_t m = (uint64_t)next32() * rexcl;
        uint32_t left = (uint32_t)m;
        if (left < rexcl) {
            const uint32_t thr = (uint32_t)((0xFFFFFFFFull - rng) % rexcl);
            while (left < thr) {
                m = (uint64_t)next32() * rexcl;
                left = (uint32_t)m;
            }
        }
        return lo + (int64_t)(m >> 32);
    }
};

constexpr uint64_t kDagGenSeed = 20260101ull;
// synth._MIX in order (the op kinds); pflt_synth's cdf is its normalised cumulative
// probabilities, the doubles numpy's cumsum / cdf[-1] produces (tests/test_synth_native.py
// checks the table)
enum SynthKind { SK_MUL, SK_DIV, SK_REM, SK_EXP, SK_ADDSUB, SK_LOGIC, SK_SHIFT, SK_ITECMP };

U synth_leaf_value(NpPhilox& g) {  // synth._leaf_value
    if (g.random() < 0.5) {  // _rand256: eight u32 draws, the first the most significant
        uint32_t l[8];
        for (int i = 7; i >= 0; i--) l[i] = g.next32();
        return U::from32(l);
    }
    const int64_t j = g.integers(0, 9);
    switch (j) {
        case 0: return U::of(0);
        case 1: return U::of(1);
        case 2: return U::of(2);
        case 3: return pf_host::mask(256);
        case 4: return pf_host::shl(U::of(1), 255);
        case 5: return pf_host::mask(160);
        default: {
            const U p = pf_host::shl(U::of(1), (unsigned)g.integers(0, 256));
            if (j == 6) return pf_host::sub(p, U::of(1));
            if (j == 8) return pf_host::add(p, U::of(1));
            return p;
        }
    }
}

// One config-3 DAG into R (synth.random_dag_set(dag_id, plant)); the witness into *wit.
void synth_dag(uint32_t dag_id, bool plant, const double* cdf, Result* R, std::vector<C8>* wit) {
    NpPhilox g(((unsigned __int128)kDagGenSeed << 32) | dag_id);
    Dag d(256);
    const int64_t n_vars = g.integers(4, 9);
    wit->clear();
    std::vector<std::pair<int32_t, U>> leaves, interior;
    for (int64_t v = 0; v < n_vars; v++) {
        leaves.push_back({-1, synth_leaf_value(g)});
        wit->push_back(c8_of(leaves.back().second));
    }
    for (int64_t v = 0; v < n_vars; v++) {
        bool created;
        leaves[v].first = d.var("x" + std::to_string(v), 256, PF_VK_GENERIC, 0, 0, plant, (*wit)[v], &created);
    }
    for (int k = 0; k < 4; k++) {
        const U c = synth_leaf_value(g);
        leaves.push_back({d.cnst(c8_of(c), 256), c});
    }
    const int depth = 32, window = 6;
    auto pick = [&](bool first) -> std::pair<int32_t, U> {
        if (first && !interior.empty() && (int)interior.size() <= depth) return interior.back();
        const size_t np = std::min<size_t>(interior.size(), (size_t)window);
        if (np && g.random() < 0.6) return interior[interior.size() - np + (size_t)g.integers(0, (int64_t)np)];
        return leaves[(size_t)g.integers(0, (int64_t)leaves.size())];
    };
    for (int it = 0; it < 48; it++) {
        const double u = g.random();
        int kind = 0;
        while (kind < 7 && !(u < cdf[kind])) kind++;   // bisect_right
        auto A = pick(true);
        auto B = pick(false);
        uint32_t op = 0;
        switch (kind) {
            case SK_DIV: op = g.random() < 0.5 ? PF_W_UDIV : PF_W_SDIV; break;
            case SK_REM: op = g.random() < 0.5 ? PF_W_UREM : PF_W_SREM; break;
            case SK_ADDSUB: op = g.random() < 0.5 ? PF_W_ADD : PF_W_SUB; break;
            case SK_LOGIC: {
                static const uint32_t ops[4] = {PF_W_AND, PF_W_OR, PF_W_XOR, PF_W_NOT};
                op = ops[g.integers(0, 4)];
                break;
            }
            case SK_SHIFT: {
                static const uint32_t ops[3] = {PF_W_SHL, PF_W_LSHR, PF_W_ASHR};
                op = ops[g.integers(0, 3)];
                if (g.random() < 0.5) {
                    (void)g.integers(0, 256);   // drawn and unused, as in synth.py
                    B.first = d.op(PF_W_AND, 256, {B.first, d.cnst(0xFF, 256)});
                    B.second = U::of(B.second.w[0] & 0xFFu);
                }
                break;
            }
            case SK_ITECMP: {
                static const uint32_t ops[3] = {PF_B_ULT, PF_B_SLT, PF_B_EQ};
                const uint32_t c_op = ops[g.integers(0, 3)];
                auto C2 = pick(false);
                const int32_t cond = d.op(c_op, 256, {A.first, C2.first});
                U cv;
                pf_host::eval_op(c_op, 256, 0, A.second, C2.second, &cv);
                const int32_t node = d.op(PF_W_ITE, 256, {cond, A.first, B.first});
                interior.push_back({node, cv.zero() ? B.second : A.second});
                continue;
            }
            case SK_MUL: op = PF_W_MUL; break;
            default: op = PF_W_EXP; break;
        }
        const int32_t node = op == PF_W_NOT ? d.op(op, 256, {A.first}) : d.op(op, 256, {A.first, B.first});
        U val;
        pf_host::eval_op(op, 256, 0, A.second, B.second, &val);
        interior.push_back({node, val});
    }
    const int64_t n_roots = g.integers(2, 5);
    const size_t nt = std::min<size_t>(interior.size(), (size_t)std::max<int64_t>(n_roots * 2, 8));
    const size_t t0 = interior.size() - nt;
    for (int64_t r = 0; r < n_roots; r++) {
        const auto& NV = interior[t0 + (size_t)g.integers(0, (int64_t)nt)];
        const int64_t cmp = g.integers(0, 3);
        const int32_t c = d.cnst(c8_of(NV.second), 256);
        int32_t root;
        if (cmp == 0) {
            root = d.op(PF_B_EQ, 256, {NV.first, c});
        } else if (cmp == 1) {
            root = d.op(PF_B_ULE, 256, {NV.first, c});
        } else {
            root = d.op(PF_B_ULE, 256, {c, NV.first});
        }
        d.roots.push_back(root);
    }
    emit_program(d, R);
    for (const DVar& v : d.vars) {
        R->names += v.name;
        R->names.push_back('\0');
    }
    R->parented = plant;
    R->dag = std::move(d);
    R->dag.memo.clear();
}

}  // namespace

extern "C" int pflt_synth(uint32_t first_id, size_t n, uint32_t plant, const double* cdf, void** results,
                          uint32_t* witness_limbs, uint32_t* n_vars_out) {
    try {
        std::vector<C8> wit;
        for (size_t i = 0; i < n; i++) {
            Result* R = new Result();
            results[i] = R;
            try {
                synth_dag(first_id + (uint32_t)i, plant != 0, cdf, R, &wit);
            } catch (const TermError& e) {
                R->rc = e.rc;
                R->err = t_err;
                return -1;
            }
            if (n_vars_out) n_vars_out[i] = (uint32_t)wit.size();
            if (witness_limbs)
                for (size_t v = 0; v < wit.size(); v++) memcpy(witness_limbs + 64 * i + 8 * v, wit[v].l, 32);
        }
    } catch (const std::exception& e) {
        t_err = std::string("pflt_synth: ") + e.what();
        return -1;
    }
    return 0;
}
