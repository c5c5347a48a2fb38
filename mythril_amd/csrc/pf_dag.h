/*
 * pf_dag.h — the bytecode DAG of libpflower.so and what comes out of it: the native form of
 * mythril_amd/lower.py:Dag (the same hash-consed node table, the same word-slicing rewrites),
 * the result a lowering hands back (Result) and the register allocation of a finished DAG
 * into it (emit_program).  Shared by the term lowering (pf_terms.cpp) and the config-3
 * generator (pf_synth.cpp), which builds its DAGs directly.  Errors are a TermError thrown
 * with the message left in t_err, which pflt_last_error reads.  Host C++ only, no HIP.
 */
#ifndef PF_DAG_H
#define PF_DAG_H

#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/pf_bytecode.h"
#include "../../include/pf_lower.h"
#include "pf_hostint.h"

namespace pf_dag {

inline thread_local std::string t_err;

struct TermError {
    int rc;
};

[[noreturn]] inline void lerr(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    t_err = buf;
    throw TermError{-2};
}

// ---- big unsigned integers (term constants: any width) ---------------------------------
typedef std::vector<uint32_t> Big;  // little-endian limbs, no trailing-zero normalisation

inline uint32_t limb(const Big& v, size_t i) { return i < v.size() ? v[i] : 0u; }

inline Big mask_big(const Big& v, uint32_t w) {
    const size_t nl = (w + 31) / 32;
    Big r(nl, 0u);
    for (size_t i = 0; i < nl; i++) r[i] = limb(v, i);
    if (w % 32 && nl) r[nl - 1] &= (1u << (w % 32)) - 1u;
    return r;
}

inline Big shr_big(const Big& v, uint32_t s) {
    const size_t q = s / 32, b = s % 32;
    Big r;
    for (size_t i = q; i < v.size(); i++) {
        uint32_t x = v[i] >> b;
        if (b && i + 1 < v.size()) x |= v[i + 1] << (32 - b);
        r.push_back(x);
    }
    return r;
}

inline bool big_zero(const Big& a) {
    for (uint32_t x : a)
        if (x) return false;
    return true;
}

inline uint32_t bitlen(const Big& a) {
    for (size_t i = a.size(); i-- > 0;)
        if (a[i]) return (uint32_t)(32 * i + 32 - __builtin_clz(a[i]));
    return 0;
}

// ---- 256-bit constants (DAG constant nodes) ------------------------------------------------
struct C8 {
    uint32_t l[8];
    bool operator==(const C8& o) const { return memcmp(l, o.l, sizeof(l)) == 0; }
};

inline C8 c8_of(const Big& v, uint32_t w) {  // v masked to w <= 256 bits
    C8 c;
    const Big m = mask_big(v, w);
    for (int i = 0; i < 8; i++) c.l[i] = limb(m, i);
    return c;
}

inline C8 c8_small(uint64_t x, uint32_t w) {
    Big b = {(uint32_t)x, (uint32_t)(x >> 32)};
    return c8_of(b, w);
}

inline Big big_of(const C8& c) { return Big(c.l, c.l + 8); }

// to and from the integers that compute (pf_hostint.h)
inline pf_host::U u_of(const C8& c) { return pf_host::U::from32(c.l); }
inline C8 c8_of(const pf_host::U& u) {
    C8 c;
    u.to32(c.l);
    return c;
}

// ---- the DAG (mythril_amd/lower.py Dag) ---------------------------------------------------
constexpr uint32_t K_VAR = PFL_K_VAR, K_CONST = PFL_K_CONST, K_BCONST = PFL_K_BCONST,
                   K_BVAR = PFL_K_BVAR;

struct DNode {
    uint32_t kind, width, nargs;
    int32_t args[3];
    uint32_t aux;
    C8 cv;  // K_CONST value
    bool is_bool;
};

struct DVar {
    std::string name;
    uint32_t width, kind, hint0, hint1;
    bool has_parent;
    C8 parent;
};

// Hash-consing table of a DAG: open addressing over node ids (the key is the node itself),
// linear probing, grown at half load.  A std::unordered_map from a node's key to its id
// allocated one 80-byte node per DAG node and, reserved for 4,096 entries per job, zeroed a
// 32 KB bucket array for buckets of a few dozen nodes — allocation churn that was a large
// share of a single query's lowering.
struct NodeTable {
    std::vector<int32_t> slot;   // -1 = empty
    size_t used = 0;
    void clear() { std::vector<int32_t>().swap(slot); used = 0; }
};

inline uint64_t node_hash(uint32_t kind, uint32_t width, uint32_t nargs, const int32_t* args, uint32_t aux,
                          bool is_bool, const C8* cv) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    auto mix = [&](uint32_t w) { h = (h ^ w) * 0x100000001B3ull; };
    mix(kind);
    mix(width);
    mix(nargs);
    mix(aux);
    for (uint32_t i = 0; i < nargs; i++) mix((uint32_t)args[i]);
    mix(is_bool ? 1u : 0u);
    if (kind == K_CONST)  // a constant without a value given is the zero constant
        for (int i = 0; i < 8; i++) mix(cv ? cv->l[i] : 0u);
    // fmix64: the table indexes with the low bits, which the FNV products alone spread poorly
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

struct Dag {
    std::vector<DNode> nodes;
    std::vector<int32_t> roots;
    std::vector<DVar> vars;
    std::vector<C8> forced;
    NodeTable memo;
    std::unordered_map<std::string, int32_t> var_index;

    explicit Dag(size_t reserve = 64) {
        size_t cap = 16;
        while (cap < 2 * reserve) cap <<= 1;
        memo.slot.assign(cap, -1);
        nodes.reserve(reserve);
    }

    bool same(const DNode& n, uint32_t kind, uint32_t width, const int32_t* args, uint32_t nargs, uint32_t aux,
              bool is_bool, const C8* cv) const {
        if (n.kind != kind || n.width != width || n.nargs != nargs || n.aux != aux || n.is_bool != is_bool) return false;
        for (uint32_t i = 0; i < nargs; i++)
            if (n.args[i] != args[i]) return false;
        if (kind == K_CONST) {
            static const C8 zero{};
            return memcmp(n.cv.l, (cv ? cv : &zero)->l, sizeof(n.cv.l)) == 0;
        }
        return true;
    }

    void grow() {
        std::vector<int32_t> old;
        old.swap(memo.slot);
        memo.slot.assign(old.size() * 2, -1);
        const size_t mask = memo.slot.size() - 1;
        for (int32_t id : old) {
            if (id < 0) continue;
            const DNode& n = nodes[(size_t)id];
            size_t h = (size_t)node_hash(n.kind, n.width, n.nargs, n.args, n.aux, n.is_bool, &n.cv) & mask;
            while (memo.slot[h] >= 0) h = (h + 1) & mask;
            memo.slot[h] = id;
        }
    }

    int32_t add_n(uint32_t kind, uint32_t width, const int32_t* args, uint32_t nargs, uint32_t aux,
                  bool is_bool, const C8* cv = nullptr) {
        if (memo.slot.empty()) memo.slot.assign(16, -1);
        const size_t mask = memo.slot.size() - 1;
        size_t h = (size_t)node_hash(kind, width, nargs, args, aux, is_bool, cv) & mask;
        for (;;) {
            const int32_t id = memo.slot[h];
            if (id < 0) break;
            if (same(nodes[(size_t)id], kind, width, args, nargs, aux, is_bool, cv)) return id;
            h = (h + 1) & mask;
        }
        DNode n;
        memset(&n, 0, sizeof(n));
        n.kind = kind;
        n.width = width;
        n.nargs = nargs;
        for (uint32_t i = 0; i < nargs; i++) n.args[i] = args[i];
        n.aux = aux;
        if (cv) n.cv = *cv;
        n.is_bool = is_bool;
        const int32_t id = (int32_t)nodes.size();
        nodes.push_back(n);
        memo.slot[h] = id;
        if (2 * ++memo.used > memo.slot.size()) grow();
        return id;
    }

    int32_t add(uint32_t kind, uint32_t width, std::initializer_list<int32_t> args, uint32_t aux,
                bool is_bool, const C8* cv = nullptr) {
        return add_n(kind, width, args.begin(), (uint32_t)args.size(), aux, is_bool, cv);
    }

    uint32_t force_consts(const std::vector<C8>& vals) {
        const uint32_t start = (uint32_t)forced.size();
        forced.insert(forced.end(), vals.begin(), vals.end());
        return start;
    }

    int32_t var(const std::string& name, uint32_t width, uint32_t kind, uint32_t h0, uint32_t h1,
                bool has_parent, const C8& parent, bool* created) {
        auto it = var_index.find(name);
        uint32_t idx;
        *created = false;
        if (it == var_index.end()) {
            idx = (uint32_t)vars.size();
            DVar v{name, width, kind, h0, h1, has_parent, parent};
            vars.push_back(v);
            var_index.emplace(name, (int32_t)idx);
            *created = true;
        } else {
            idx = (uint32_t)it->second;
        }
        if (kind == PF_VK_BOOL) return add(K_BVAR, 1, {}, idx, true);
        return add(K_VAR, width, {}, idx, false);
    }

    int32_t cnst(const C8& v, uint32_t width) {
        if (width == 256) return add(K_CONST, width, {}, 0, false, &v);
        const C8 m = c8_of(pf_host::mw(u_of(v), width));
        return add(K_CONST, width, {}, 0, false, &m);
    }
    int32_t cnst(uint64_t v, uint32_t width) { return cnst(c8_small(v, width), width); }
    int32_t bconst(bool v) { return add(K_BCONST, 1, {}, v ? 1u : 0u, true); }

    const C8* cval(int32_t i) const { return nodes[i].kind == K_CONST ? &nodes[i].cv : nullptr; }

    int32_t op(uint32_t opc, uint32_t w, std::initializer_list<int32_t> args, uint32_t aux = 0) {
        const int32_t r = simplify(opc, w, args.begin(), aux);
        if (r >= 0) return r;
        return add_n(opc, w, args.begin(), (uint32_t)args.size(), aux, opc >= PF_B_CONST);
    }

    // Dag._simplify: the word-slicing rewrites (lower.py)
    int32_t simplify(uint32_t opc, uint32_t w, const int32_t* args, uint32_t aux) {
        if (opc == PF_W_UDIV) {
            const C8* c = cval(args[1]);
            if (c) {
                const Big cb = big_of(*c);
                const uint32_t bl = bitlen(cb);
                if (bl && bitlen(mask_big(shr_big(cb, 0), bl - 1)) == 0) {  // power of two
                    const uint32_t k = bl - 1;
                    return k == 0 ? args[0] : op(PF_W_LSHR, w, {args[0], cnst(k, w)});
                }
            }
        } else if (opc == PF_W_LSHR) {
            const C8* c = cval(args[1]);
            const DNode x = nodes[args[0]];
            if (c && bitlen(big_of(*c)) <= 32 && c->l[0] < w) {
                const uint32_t k = c->l[0];
                if (k == 0) return args[0];
                if (x.kind == PF_W_MOV) {
                    const int32_t inner = x.args[0];
                    const uint32_t wi = nodes[inner].width;
                    if (k >= wi) return cnst(0, w);
                    return op(PF_W_MOV, w, {op(PF_W_EXTRACT, wi - k, {inner}, k)});
                }
                if (x.kind == PF_W_CONCAT) return op(PF_W_MOV, w, {op(PF_W_EXTRACT, w - k, {args[0]}, k)});
            }
        } else if (opc == PF_W_AND) {
            for (int xi = 0; xi < 2; xi++) {
                const int ci = 1 - xi;
                const C8* c = cval(args[ci]);
                if (!c) continue;
                const Big cb = big_of(*c);
                const uint32_t bl = bitlen(cb);
                if (bl == 0) continue;
                // c == 2^bl - 1
                bool ones = true;
                for (uint32_t i = 0; i < bl; i++)
                    if (!((cb[i / 32] >> (i % 32)) & 1u)) { ones = false; break; }
                if (ones && bl < w) return op(PF_W_MOV, w, {op(PF_W_EXTRACT, bl, {args[xi]}, 0)});
            }
        } else if (opc == PF_W_EXTRACT) {
            const DNode x = nodes[args[0]];
            if (aux == 0 && w == x.width) return args[0];
            if (x.kind == PF_W_CONCAT) {
                const int32_t hi = x.args[0], lo = x.args[1];
                const uint32_t wl = x.aux;
                if (aux >= wl) return op(PF_W_EXTRACT, w, {hi}, aux - wl);
                if (aux + w <= wl) return op(PF_W_EXTRACT, w, {lo}, aux);
                const int32_t top = op(PF_W_EXTRACT, aux + w - wl, {hi}, 0);
                const int32_t bot = op(PF_W_EXTRACT, wl - aux, {lo}, aux);
                return op(PF_W_CONCAT, w, {top, bot}, wl - aux);
            }
            if (x.kind == PF_W_MOV) {
                const int32_t inner = x.args[0];
                const uint32_t wi = nodes[inner].width;
                if (aux + w <= wi) return op(PF_W_EXTRACT, w, {inner}, aux);
                if (aux >= wi) return cnst(0, w);
            }
            if (x.kind == K_CONST) return cnst(c8_of(shr_big(big_of(x.cv), aux), w), w);
        } else if (opc == PF_W_MOV) {
            const DNode x = nodes[args[0]];
            if (x.width == w) return args[0];
            if (x.kind == PF_W_MOV) return op(PF_W_MOV, w, {x.args[0]});
            if (x.kind == K_CONST) return cnst(x.cv, w);
        } else if (opc == PF_B_EQ) {
            for (int xi = 0; xi < 2; xi++) {
                const int ci = 1 - xi;
                const C8* c = cval(args[ci]);
                const DNode x = nodes[args[xi]];
                if (c && x.kind == PF_W_MOV) {
                    const uint32_t wy = nodes[x.args[0]].width;
                    if (!big_zero(shr_big(big_of(*c), wy))) return bconst(false);
                    return op(PF_B_EQ, wy, {x.args[0], cnst(*c, wy)});
                }
            }
        }
        return -1;
    }

    // the calldata-byte arm's word constants (Dag.word_constants / finalize_word_hints)
    void finalize_word_hints() {
        bool any = false;
        for (const DVar& v : vars) any |= v.kind == PF_VK_CDBYTE;
        if (!any) return;
        std::vector<C8> words;
        for (const DNode& nd : nodes) {
            if (!(nd.kind == PF_B_EQ || nd.kind == PF_B_ULT || nd.kind == PF_B_ULE ||
                  nd.kind == PF_B_SLT || nd.kind == PF_B_SLE))
                continue;
            const DNode& a = nodes[nd.args[0]];
            const DNode& b = nodes[nd.args[1]];
            const DNode* pairs[2][2] = {{&a, &b}, {&b, &a}};
            for (auto& pr : pairs) {
                const DNode* c = pr[0];
                const DNode* other = pr[1];
                if (c->kind != K_CONST) continue;
                if (other->kind == K_VAR && vars[other->aux].kind == PF_VK_SMALL) continue;
                bool seen = false;
                for (const C8& x : words) seen |= x == c->cv;
                if (!seen) words.push_back(c->cv);
            }
        }
        if (words.size() > 0xFFF) words.resize(0xFFF);
        if (words.empty() || forced.size() >= 0xFFF) return;
        const uint32_t start = force_consts(words);
        for (DVar& v : vars)
            if (v.kind == PF_VK_CDBYTE) v.hint0 = (v.hint0 & 0xFFu) | ((uint32_t)words.size() << 8) | (start << 20);
    }
};

// ---- results ------------------------------------------------------------------------------
// var_terms descriptors handed back to the host (Lowered.var_terms)
struct VarTerm {
    uint32_t type;  // PFLT_VT_TERM / PFLT_VT_SELECT / PFLT_VT_EXTRACT
    uint32_t a, b;  // term id | (array id, index id) | (term id, lo)
    uint32_t c;     // extract hi
};

struct Result {
    Dag dag;
    std::vector<VarTerm> var_terms;
    std::vector<uint32_t> uf_apps;
    std::vector<uint32_t> reads;   // (array id, index id) pairs, arrays in insertion order
    std::vector<uint32_t> read_counts;  // entries per array, same order
    std::vector<uint32_t> code;    // n_ins x 4
    std::vector<uint32_t> consts;  // n_const x 8
    std::vector<uint32_t> packed_nodes, pool;  // pack_nodes of the DAG (tests)
    std::string names;             // variable names, '\0'-separated
    uint32_t n_wregs = 0;
    int n_sat = 0;
    int rc = 0;                    // 0, or the failure code (-2 LoweringError -> z3, -1 / -3 ...)
    std::string err;               // the failure message
    std::vector<uint32_t> in_roots;  // the bucket's conjuncts (the re-check's roots)
    bool parented = false;         // a parent model seeded some variable
};

inline void pack(const Dag& d, std::vector<uint32_t>* nodes, std::vector<uint32_t>* pool) {
    nodes->clear();
    pool->clear();
    uint32_t np = 0;
    for (const DNode& n : d.nodes) {
        uint32_t aux = n.aux;
        if (n.kind == K_CONST) {
            aux = np++;
            pool->insert(pool->end(), n.cv.l, n.cv.l + 8);
        }
        const uint32_t a0 = n.nargs > 0 ? (uint32_t)n.args[0] : 0u, a1 = n.nargs > 1 ? (uint32_t)n.args[1] : 0u,
                       a2 = n.nargs > 2 ? (uint32_t)n.args[2] : 0u;
        const uint32_t rec[8] = {n.kind, n.width, n.nargs, a0, a1, a2, aux, n.is_bool ? 1u : 0u};
        nodes->insert(nodes->end(), rec, rec + 8);
    }
    if (nodes->empty()) nodes->assign(8, 0u);
}

// Register allocation + emission of a finished DAG into R (lower.lower(dag): narrow register
// file first, wide when the narrow program is spill-heavy and the wide one at least halves
// its spill code).  Throws TermError like the lowering.
inline void emit_program(Dag& d, Result* R) {
    d.finalize_word_hints();
    pack(d, &R->packed_nodes, &R->pool);
    std::vector<uint32_t> forced;
    for (const C8& c : d.forced) forced.insert(forced.end(), c.l, c.l + 8);
    std::vector<uint32_t> roots2(d.roots.begin(), d.roots.end());
    if (roots2.empty()) roots2.push_back(0);
    const uint32_t tries[2] = {PF_NW_NARROW, PF_NW};
    int rc = -2;
    // the narrow program unless its spill code exceeds an eighth of it and the wide
    // register file at least halves that (lower.py lower(): the same policy)
    bool have_narrow = false;
    std::vector<uint32_t> n_code, n_consts;
    size_t n_spill_narrow = 0;
    // output scratch per thread, grown but never cleared (pfl_lower writes what it
    // reports); the result keeps only the words written
    thread_local std::vector<uint32_t> code_buf, const_buf;
    for (int ti = 0; ti < 2; ti++) {
        size_t cap_i = 16 * d.nodes.size() + 64 + 4 * d.roots.size();
        size_t cap_c = R->pool.size() / 8 + d.forced.size() + 1;
        size_t ni = 0, nc = 0;
        for (int attempt = 0; attempt < 4; attempt++) {
            if (code_buf.size() < 4 * cap_i) code_buf.resize(4 * cap_i);
            if (const_buf.size() < 8 * cap_c) const_buf.resize(8 * cap_c);
            rc = pfl_lower(R->packed_nodes.data(), d.nodes.size(), R->pool.data(), R->pool.size() / 8,
                           roots2.data(), d.roots.size(), forced.empty() ? nullptr : forced.data(),
                           d.forced.size(), tries[ti], code_buf.data(), cap_i, &ni, const_buf.data(),
                           cap_c, &nc);
            if (rc != -3) break;
            cap_i *= 4;
            cap_c *= 4;
        }
        if (rc == 0) {
            R->code.assign(code_buf.begin(), code_buf.begin() + 4 * ni);
            R->consts.assign(const_buf.begin(), const_buf.begin() + 8 * nc);
            size_t n_spill = 0;
            for (size_t i = 0; i < ni; i++) {
                const uint32_t op = R->code[4 * i] & 0xffu;
                n_spill += op == PF_W_SPILL || op == PF_W_FILL;
            }
            R->n_wregs = tries[ti];
            if (ti == 0 && 8 * n_spill > ni) {  // spill-heavy: try the wide register file
                have_narrow = true;
                n_code.swap(R->code);
                n_consts.swap(R->consts);
                n_spill_narrow = n_spill;
                continue;
            }
            if (ti == 1 && have_narrow && 2 * n_spill > n_spill_narrow) {
                R->code.swap(n_code);
                R->consts.swap(n_consts);
                R->n_wregs = tries[0];
            }
            break;
        }
        if (ti == 1 && have_narrow) {  // the wide lowering failed (any rc): keep the narrow one
            R->code.swap(n_code);
            R->consts.swap(n_consts);
            R->n_wregs = tries[0];
            rc = 0;
            break;
        }
        if (rc != -2) break;
    }
    if (rc != 0) {
        t_err = pfl_last_error();
        throw TermError{rc};
    }
}

}  // namespace pf_dag

#endif /* PF_DAG_H */
