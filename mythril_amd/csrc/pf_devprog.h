/*
 * pf_devprog.h — from a caller's packed batch to the program the kernels run: the validator
 * (check_set), the device-program rewrites, the threaded driver over set ranges
 * (prepare_program), the device constant pool and the wave order.  Host C++ only, no HIP:
 * pathfeas.hip uploads and launches what this header returns, and
 * tests/devprog_host_check.cpp runs it stand-alone under the sanitizers.  Errors are returned
 * as strings; nothing here keeps state between calls.  The functions are static: the header
 * has one includer per binary, and a pass with internal linkage and one call site is inlined
 * into device_program_range as it was when the passes were one function.
 */
#ifndef PF_DEVPROG_H
#define PF_DEVPROG_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pf_bytecode.h"
#include "pf_fold.h"

namespace pf_devprog {

#if defined(__GNUC__)
__attribute__((format(printf, 1, 2)))
#endif
static inline std::string errorf(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// PF_DEVICE_FOLD: the device program's fold pass (pf_fold.h).  0 = off, 1 = on (default),
// 2 = the fold pass alone, without the peepholes after it (its output is still a lowered
// program, so tests can feed it back in).  pf_batch_create takes the value read at init,
// pf_device_program reads it on every call.
// pf_batch_create folds only batches of PF_FOLD_MIN_SETS sets or more.  The walk costs ~19 ns
// per instruction on the host (corpus batch, 1,023 sets / 507,856 instructions: 2.6 -> 3.9 ms)
// and pays back over the candidates a set is swept with; a single query's batch is one or two
// buckets of ~500 instructions searched with early exit, and its upload phase grew from 0.073
// to 0.083 ms (run-to-run spread 0.001) for no search time back (profiles/r07_fold_ab.md).
// No program length makes the walk free, so the gate is the batch's set count.
constexpr size_t PF_FOLD_MIN_SETS = 16;
static inline int device_fold_env() {
    const char* e = getenv("PF_DEVICE_FOLD");
    if (!e || !*e) return 1;
    const long v = strtol(e, nullptr, 10);
    return v >= 0 && v <= 2 ? (int)v : 1;
}

// `code` with the traffic / unit bits of every instruction recomputed (the host-only exports,
// which rewrite without validating)
static inline std::vector<uint32_t> stamped(const uint32_t* code, size_t n_ins) {
    std::vector<uint32_t> fixed(code, code + 4 * n_ins);
    for (size_t i = 0; i < n_ins; i++) fixed[4 * i] = pf_ins_stamp(fixed[4 * i]);
    return fixed;
}

// Set s: its ranges, operands and schema checked against the batch, and its instructions
// copied into fixed[] (the set's own range) with the traffic / unit bits recomputed and
// register def-before-use checked; wide[s] set.  Every kernel index is derived from what
// passes here, so nothing the caller packed is trusted.  Returns the error, empty if none.
static inline std::string check_set(size_t s, const uint32_t* code, size_t n_ins, size_t n_const, const uint32_t* schema,
                             size_t n_vars, size_t n_parents, const pf_set_desc* descs, uint32_t* fixed,
                             uint8_t* wide) {
    const pf_set_desc& d = descs[s];
    if ((uint64_t)d.code_off + d.n_ins > n_ins || d.n_ins == 0)
        return errorf("set %zu: code range [%u,+%u) outside %zu instructions", s, d.code_off, d.n_ins, n_ins);
    if ((uint64_t)d.const_off + d.n_const > n_const) return errorf("set %zu: constant range outside pool", s);
    if ((uint64_t)d.var_off + d.n_vars > n_vars) return errorf("set %zu: schema range outside", s);
    if (pf_ins_op(code[4 * ((size_t)d.code_off + d.n_ins - 1)]) != PF_END)
        return errorf("set %zu: program does not end with PF_END", s);
    for (uint32_t i = 0; i < d.n_ins; i++) {
        const uint32_t* I = code + 4 * ((size_t)d.code_off + i);
        const uint32_t op = pf_ins_op(I[0]), w = pf_ins_width(I[0]);
        if (op != PF_END && (w == 0 || w > PF_MAX_WIDTH))
            return errorf("set %zu ins %u: width %u out of range", s, i, w);
        if ((op == PF_W_VAR || op == PF_B_VAR) && I[2] >= d.n_vars)
            return errorf("set %zu ins %u: variable %u >= %u", s, i, I[2], d.n_vars);
        if (op == PF_W_CONST && I[2] >= d.n_const)
            return errorf("set %zu ins %u: constant %u >= %u", s, i, I[2], d.n_const);
    }
    for (uint32_t v = 0; v < d.n_vars; v++) {
        const uint32_t* sc = schema + 4 * ((size_t)d.var_off + v);
        const uint32_t kind = sc[0] & 0xffu, w = (sc[0] >> 8) & 0x3ffu;
        if (w == 0 || w > PF_MAX_WIDTH) return errorf("set %zu var %u: width %u", s, v, w);
        if (sc[3] != PF_NO_PARENT && sc[3] >= n_parents) return errorf("set %zu var %u: parent slot", s, v);
        if (kind == PF_VK_KECCAK && sc[1] >= d.n_const) return errorf("set %zu var %u: keccak base", s, v);
        if (kind == PF_VK_ACTOR && (sc[2] > 4 || sc[1] + sc[2] > d.n_const))
            return errorf("set %zu var %u: actor table", s, v);
        if (kind == PF_VK_CDBYTE && ((sc[1] & 0xffu) > 248u || (sc[1] & 7u) ||
                                     (sc[1] >> 20) + ((sc[1] >> 8) & 0xfffu) > d.n_const))
            return errorf("set %zu var %u: calldata word constants", s, v);
    }
    // traffic bits and register def-before-use, recomputed here so the kernel can trust
    // them whatever the caller packed (w0 bits 18..23)
    memcpy(fixed + 4 * (size_t)d.code_off, code + 4 * (size_t)d.code_off, 16 * (size_t)d.n_ins);
    uint32_t wdef = 0u, bdef = 0u, max_wreg = 0u;
    uint64_t sdef = 0ull;
    for (uint32_t i = 0; i < d.n_ins; i++) {
        uint32_t* I = fixed + 4 * ((size_t)d.code_off + i);
        const uint32_t op = pf_ins_op(I[0]), tr = pf_op_traffic(op);
        I[0] = pf_ins_stamp(I[0]);
        const uint32_t rd = pf_ins_dst(I[1]), ra = pf_ins_a(I[1]), rb = pf_ins_b(I[1]), rc = pf_ins_c(I[1]);
        if ((tr & PF_TR_WW) && rd >= PF_NW) return errorf("set %zu ins %u: W dst %u", s, i, rd);
        if (((tr & PF_TR_RA) && (ra >= PF_NW || !(wdef >> ra & 1u))) ||
            ((tr & PF_TR_RB) && (rb >= PF_NW || !(wdef >> rb & 1u))))
            return errorf("set %zu ins %u: W register read before write", s, i);
        const bool bres = PF_OP_WRITES_B(op);
        const bool breads_ab = op >= PF_B_AND && op <= PF_B_XOR;
        if ((breads_ab && (!(bdef >> (ra & 31u) & 1u) || !(bdef >> (rb & 31u) & 1u))) ||
            ((op == PF_B_NOT || op == PF_ASSERT || op == PF_B_SPILL) && !(bdef >> (ra & 31u) & 1u)) ||
            ((op == PF_W_ITE || op == PF_B_ITE) && !(bdef >> (rc & 31u) & 1u)) ||
            (op == PF_B_ITE && (!(bdef >> (ra & 31u) & 1u) || !(bdef >> (rb & 31u) & 1u))))
            return errorf("set %zu ins %u: B register read before write", s, i);
        if ((op == PF_W_SPILL || op == PF_W_FILL || op == PF_B_SPILL || op == PF_B_FILL) && I[2] >= PF_MAX_SPILL)
            return errorf("set %zu ins %u: spill slot %u >= %d", s, i, I[2], PF_MAX_SPILL);
        if (op == PF_W_SPILL || op == PF_B_SPILL) sdef |= 1ull << I[2];
        if ((op == PF_W_FILL || op == PF_B_FILL) && !(sdef >> I[2] & 1ull))
            return errorf("set %zu ins %u: spill slot %u filled before it was spilled", s, i, I[2]);
        if (tr & PF_TR_WW) {
            wdef |= 1u << rd;
            max_wreg = std::max(max_wreg, rd);
        }
        if (i + 1 == d.n_ins) wide[s] = max_wreg >= PF_NW_NARROW;
        if (bres) bdef |= 1u << (rd & 31u);
    }
    return {};
}

// The device form of a validated batch (traffic / unit bits already set): a fold pass and
// semantics-preserving peepholes rewrite the program the kernel runs, never the caller's
// arrays (the oracles evaluate the program as lowered).  Each set is rewritten in a working
// copy (descriptors may share or reorder code ranges) and appended to code_out; every pass is
// one forward walk with per-register state.  The passes, in the order device_program_range
// runs them (PF_DEVICE_FOLD = 2 stops after the first):
//  0. fold_constants   1. fuse_asserts   2. drop_zext_movs   3. constant_operands
//  4. lds_spill_slots  5. forward_results, then append_kept compacts.
// aux1 of every dropped instruction, in whatever pass, moves to the next kept one: a wave
// leaves a program only at an assert, so `ops` counts what it counted for the lowered
// program (the counter contract).

// One set's working copy and the passes' scratch, one per host thread and reused from set to
// set (a per-set allocation shows in a single query's upload phase).
struct Work {
    std::vector<uint32_t> P;    // the set being rewritten, 4 u32 per instruction
    std::vector<uint8_t> drop;  // 1: the device program leaves the instruction out
    uint32_t n = 0;
    pf_fold::Scratch fold;
    struct Pending {  // pass 3: the W_CONST a register holds, and its readers
        int64_t at = -1;
        bool ok = true;
        std::vector<uint32_t> readers;
    };
    Pending pend[PF_NW + 1];
    // site bookkeeping (SiteMap below), filled only while one is collected: origin[k] = the
    // PF_ASSERT that fuse_asserts moved onto instruction k
    std::vector<int64_t> origin;
};

// Which PF_ASSERT of the lowered program every assert site of the device program stands for
// (pf_device_sites): asserts holds, per site and in set and site order, the assert's ordinal
// among the set's PF_ASSERTs; cnt[s] = the sites of set s.  The working copy keeps every
// instruction at its lowered index until append_kept, so an assert is followed by its index:
// the fold pass drops the ones it proves true, fuse_asserts moves one onto the last writer of
// its B register (at most one per writer).
struct SiteMap {
    std::vector<uint32_t> asserts, cnt;
};
static inline void collect_sites(const Work& T, SiteMap& M) {
    std::vector<uint32_t> ord(T.n, 0);
    uint32_t k = 0;
    for (uint32_t i = 0; i < T.n; i++)
        if (pf_ins_op(T.P[4 * (size_t)i]) == PF_ASSERT) ord[i] = k++;
    uint32_t sites = 0;
    for (uint32_t i = 0; i < T.n; i++) {
        if (T.drop[i]) continue;
        const uint32_t w0 = T.P[4 * (size_t)i];
        if (pf_ins_op(w0) == PF_ASSERT) {
            M.asserts.push_back(ord[i]);
            sites++;
        } else if ((w0 & PF_I_ASSERT) && T.origin[i] >= 0) {
            M.asserts.push_back(ord[(size_t)T.origin[i]]);
            sites++;
        }
    }
    M.cnt.push_back(sites);
}

// Constants of the device programs' own (pf_fold.h: a constant result that is neither 0 nor in
// the set's pool): vals holds 8 u32 each in set order, cnt[s] how many set s has.  Their indices
// follow the set's own n_const constants (device_program lays the pool out that way).
struct OwnConsts {
    std::vector<uint32_t> vals;
    std::vector<uint32_t> cnt;
};

// 0. fold (pf_fold.h, PF_DEVICE_FOLD): results that are the same for every candidate —
// constant operands, x-op-x identities, absorbing and neutral constants, compares and
// divisions a value's range decides — become a W_MOV, W_CONST (of the set's pool, or of a
// constant of the program's own: OwnConsts), B_CONST or W_XOR r, r, and what only they needed
// is dropped (liveness from the ASSERTs).  The passes below clean up after it (its W_MOVs and
// W_CONSTs mostly vanish).  consts (n_const x 8 u32, set-relative indices resolved through
// const_off) may be null: then no constant is known.
static inline void fold_constants(Work& T, size_t s, const pf_set_desc& d, const uint32_t* consts, size_t n_const,
                           OwnConsts* own) {
    const bool pool = consts && (uint64_t)d.const_off + d.n_const <= n_const;
    // a set without constants has a pool all the same: the empty one
    const bool own_ok = own && (pool || (d.n_const == 0 && d.const_off <= n_const));
    const size_t before = own ? own->vals.size() : 0;
    pf_fold::fold_program(T.P.data(), T.n, T.drop.data(), pool ? consts + 8 * (size_t)d.const_off : nullptr,
                          pool ? d.n_const : 0u, T.fold, own_ok ? &own->vals : nullptr);
    if (own) own->cnt[s] = (uint32_t)((own->vals.size() - before) / 8);
}

// 1. ASSERT: folded into the last writer of its B register when that is a compare or bool op
// (PF_I_ASSERT) — the conjunction's value does not depend on where the and happens, and
// with PF_FLAG_SHORTCIRCUIT an earlier check only exits sooner (round 2 folded it only
// into the instruction right before it).
static inline void fuse_asserts(Work& T) {
    uint32_t* P = T.P.data();
    int64_t last_b[PF_NB];
    for (int r = 0; r < PF_NB; r++) last_b[r] = -1;
    for (uint32_t i = 0; i < T.n; i++) {
        if (T.drop[i]) continue;
        const uint32_t op = pf_ins_op(P[4 * i]);
        if (op == PF_ASSERT) {
            const int64_t k = last_b[pf_ins_a(P[4 * i + 1]) & 31u];
            if (k >= 0) {
                const uint32_t unit = pf_op_unit(pf_ins_op(P[4 * (size_t)k]));
                if ((unit == PF_U_CMP || unit == PF_U_BOOL) && !(P[4 * (size_t)k] & PF_I_ASSERT)) {
                    P[4 * (size_t)k] |= PF_I_ASSERT;
                    T.drop[i] = 1;
                    if (!T.origin.empty()) T.origin[(size_t)k] = i;
                }
            }
        } else if (PF_OP_WRITES_B(op)) {
            last_b[pf_ins_dst(P[4 * i + 1]) & 31u] = i;
        }
    }
}

// does instruction (w0, w1) read W register r as operand a / b, or write it, by its traffic bits
static inline bool reads_a(uint32_t w0, uint32_t w1, uint32_t r) {
    return (pf_ins_traffic(w0) & PF_TR_RA) && pf_ins_a(w1) == r;
}
static inline bool reads_b(uint32_t w0, uint32_t w1, uint32_t r) {
    return (pf_ins_traffic(w0) & PF_TR_RB) && pf_ins_b(w1) == r;
}
static inline bool writes_w(uint32_t w0, uint32_t w1, uint32_t r) {
    return (pf_ins_traffic(w0) & PF_TR_WW) && pf_ins_dst(w1) == r;
}

// 2. W_MOV: a zero-extending move (its source holds a value no wider than the move — values
// are kept zero-extended, so the move copies it unchanged) is deleted and the readers of
// its destination, up to that register's next write, read the source — provided the
// source is not rewritten before the last of them.
static inline void drop_zext_movs(Work& T) {
    uint32_t* P = T.P.data();
    const uint8_t* drop = T.drop.data();
    const uint32_t n = T.n;
    uint32_t wwidth[PF_NW + 1];  // width of the value each W register holds now
    for (int r = 0; r <= PF_NW; r++) wwidth[r] = 0xffffffffu;
    for (uint32_t i = 0; i < n; i++) {
        if (drop[i]) continue;
        const uint32_t w0 = P[4 * i], dst = pf_ins_dst(P[4 * i + 1]), w = pf_ins_width(w0);
        if (pf_ins_op(w0) != PF_W_MOV) {
            if ((pf_ins_traffic(w0) & PF_TR_WW) && dst <= PF_NW) wwidth[dst] = w;
            continue;
        }
        const uint32_t src = pf_ins_a(P[4 * i + 1]);
        bool ok = src <= PF_NW && dst <= PF_NW && wwidth[src] <= w;
        uint32_t last = i;
        if (ok) {
            bool src_dead = false;
            for (uint32_t j = i + 1; j < n; j++) {
                if (drop[j]) continue;
                const uint32_t jw0 = P[4 * j], jw1 = P[4 * j + 1];
                if (reads_a(jw0, jw1, dst) || reads_b(jw0, jw1, dst)) {
                    if (src_dead) { ok = false; break; }
                    last = j;
                }
                if (writes_w(jw0, jw1, dst)) break;
                if (writes_w(jw0, jw1, src)) src_dead = true;
                if (pf_ins_op(jw0) == PF_END) break;
            }
        }
        if (!ok) {
            if (dst <= PF_NW) wwidth[dst] = w;
            continue;
        }
        for (uint32_t t = i + 1; t <= last; t++) {
            const uint32_t tw0 = P[4 * t];
            uint32_t& w1 = P[4 * t + 1];
            if (reads_a(tw0, w1, dst)) w1 = pf_ins_with_a(w1, src);
            if (reads_b(tw0, w1, dst)) w1 = pf_ins_with_b(w1, src);
        }
        T.drop[i] = 1;  // dst keeps its old value, which nothing reads before its next write
    }
}

// A constant is folded into an operand only when it fits the W_CONST's width: the W_CONST
// masks its value at write-back, a folded operand is read raw (ADVICE r4 — the lowering never
// packs a wider one, but pf_batch_create trusts nothing the caller packed).  consts may be
// null: then every constant is taken to fit (pf_device_program's callers that pass none).
static inline bool const_fits(const uint32_t* consts, size_t n_const, uint32_t idx, uint32_t w) {
    if (!consts) return true;
    if (idx >= n_const) return false;
    const uint32_t* c = consts + 8 * (size_t)idx;
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t lo = 32u * j;
        const uint32_t keep = w >= lo + 32u ? 0xffffffffu : (w > lo ? (1u << (w - lo)) - 1u : 0u);
        if (c[j] & ~keep) return false;
    }
    return true;
}

// 3. W_CONST: deleted when its register is read, until its next write, only as the a / b
// operand of W-reading instructions (not SPILL or MOV); those take the constant directly
// (PF_I_KA / PF_I_KB, the constant index in the register field, traffic bit cleared) and
// the kernel reads it with one scalar load.  own: the program may hold constants of its own,
// whose indices follow the set's n_const.
static inline void constant_operands(Work& T, const pf_set_desc& d, const uint32_t* consts, size_t n_const, bool own) {
    uint32_t* P = T.P.data();
    auto settle = [&](uint32_t r) {
        Work::Pending& q = T.pend[r];
        if (q.at >= 0 && q.ok && !q.readers.empty()) {
            const uint32_t k = P[4 * (size_t)q.at + 2];
            for (uint32_t t : q.readers) {
                uint32_t& w0 = P[4 * t];
                uint32_t& w1 = P[4 * t + 1];
                const bool ka = reads_a(w0, w1, r), kb = reads_b(w0, w1, r);
                if (ka) {
                    w0 = (w0 & ~(PF_TR_RA << 18)) | PF_I_KA;
                    w1 = pf_ins_with_a(w1, k);
                }
                if (kb) {
                    w0 = (w0 & ~(PF_TR_RB << 18)) | PF_I_KB;
                    w1 = pf_ins_with_b(w1, k);
                }
            }
            T.drop[q.at] = 1;
        }
        q.at = -1;
        q.ok = true;
        q.readers.clear();
    };
    for (uint32_t i = 0; i < T.n; i++) {
        if (T.drop[i]) continue;
        const uint32_t w0 = P[4 * i], w1 = P[4 * i + 1], op = pf_ins_op(w0), tr = pf_ins_traffic(w0);
        const uint32_t ra = pf_ins_a(w1), rb = pf_ins_b(w1), rd = pf_ins_dst(w1);
        if (op == PF_END) break;
        // reads first (an instruction may read and rewrite the same register)
        for (int side = 0; side < 2; side++) {
            const uint32_t r = side ? rb : ra;
            if (!(tr & (side ? PF_TR_RB : PF_TR_RA)) || r > PF_NW || T.pend[r].at < 0) continue;
            if (side && (tr & PF_TR_RA) && ra == r) continue;  // the same register twice
            if (op == PF_W_SPILL || op == PF_W_MOV) T.pend[r].ok = false;
            else T.pend[r].readers.push_back(i);
        }
        if ((tr & PF_TR_WW) && rd <= PF_NW) {
            settle(rd);
            // (a constant of the program's own is below 2^w of the instruction it replaced)
            if (op == PF_W_CONST && P[4 * i + 2] <= 0xffu &&
                ((own && P[4 * i + 2] >= d.n_const) ||
                 const_fits(consts, n_const, d.const_off + P[4 * i + 2], pf_ins_width(w0))))
                T.pend[rd].at = i;
        }
    }
    for (uint32_t r = 0; r <= PF_NW; r++) settle(r);
}

// 4. spill slots -> LDS entries 1..3 of EXP's window table (PF_SPILL_LDS)
// A segment is a SPILL of slot k and the FILLs of k before its next SPILL.  One whose
// range holds no W_EXP takes entry 2 or 3 when free (entry 1 too if no B_UMUL_NOOVF
// runs in it): the value never touches scratch.  Entries are handed out in program
// order; a segment without a FILL stays (a dead store costs nothing more).
static inline void lds_spill_slots(Work& T) {
    uint32_t* P = T.P.data();
    struct Seg {
        uint32_t spill, last;
        std::vector<uint32_t> fills;
    };
    std::vector<Seg> segs;
    int64_t open[PF_MAX_SPILL];
    for (int k = 0; k < PF_MAX_SPILL; k++) open[k] = -1;
    std::vector<uint32_t> exp_at, umul_at;
    for (uint32_t i = 0; i < T.n; i++) {
        if (T.drop[i]) continue;
        const uint32_t op = pf_ins_op(P[4 * i]), k = P[4 * i + 2] & (PF_MAX_SPILL - 1u);
        if (op == PF_END) break;
        if (op == PF_W_EXP) exp_at.push_back(i);
        if (op == PF_B_UMUL_NOOVF) umul_at.push_back(i);
        if (op == PF_W_SPILL || op == PF_B_SPILL) {
            open[k] = (int64_t)segs.size();
            segs.push_back(Seg{i, i, {}});
        } else if ((op == PF_W_FILL || op == PF_B_FILL) && open[k] >= 0) {
            Seg& g = segs[(size_t)open[k]];
            g.fills.push_back(i);
            g.last = i;
        }
    }
    auto any_in = [](const std::vector<uint32_t>& at, uint32_t lo, uint32_t hi) {
        const auto it = std::upper_bound(at.begin(), at.end(), lo);
        return it != at.end() && *it < hi;
    };
    int64_t busy_until[4] = {-1, -1, -1, -1};
    static const uint32_t order[3] = {2u, 3u, 1u};
    for (const Seg& g : segs) {
        if (g.fills.empty() || any_in(exp_at, g.spill, g.last)) continue;
        const bool umul = any_in(umul_at, g.spill, g.last);
        for (uint32_t e : order) {
            if ((e == 1u && umul) || busy_until[e] >= (int64_t)g.spill) continue;
            busy_until[e] = g.last;
            P[4 * (size_t)g.spill + 2] = PF_SPILL_LDS | e;
            for (uint32_t f : g.fills) P[4 * (size_t)f + 2] = PF_SPILL_LDS | e;
            break;
        }
    }
}

// 5. back-to-back forwarding: an instruction reading the W register the kept
// instruction right before it wrote takes that result directly (PF_I_FA / PF_I_FB,
// traffic bit cleared), and the writer skips its write-back (PF_TR_WW cleared) when
// no later instruction reads the register before its next write
static inline void forward_results(Work& T) {
    uint32_t* P = T.P.data();
    const uint8_t* drop = T.drop.data();
    const uint32_t n = T.n;
    int64_t prev = -1;
    for (uint32_t q = 0; q < n; q++) {
        if (drop[q]) continue;
        const int64_t p = prev;
        prev = q;
        uint32_t& qw0 = P[4 * q];
        if (pf_ins_op(qw0) == PF_END) break;
        if (p < 0) continue;
        uint32_t& pw0 = P[4 * (size_t)p];
        const uint32_t pd = pf_ins_dst(P[4 * (size_t)p + 1]);
        if (!(pf_ins_traffic(pw0) & PF_TR_WW) || PF_OP_WRITES_B(pf_ins_op(pw0)) || pd > PF_NW) continue;
        const uint32_t qw1 = P[4 * q + 1];
        const bool fa = reads_a(qw0, qw1, pd), fb = reads_b(qw0, qw1, pd);
        if (!fa && !fb) continue;
        bool live = false;
        if (!writes_w(qw0, qw1, pd)) {
            for (uint32_t r = q + 1; r < n && !live; r++) {
                if (drop[r]) continue;
                const uint32_t rw0 = P[4 * r], rw1 = P[4 * r + 1];
                if (pf_ins_op(rw0) == PF_END) break;
                live = reads_a(rw0, rw1, pd) || reads_b(rw0, rw1, pd);
                if (writes_w(rw0, rw1, pd)) break;
            }
        }
        qw0 &= ~(((fa ? PF_TR_RA : 0u) | (fb ? PF_TR_RB : 0u)) << 18);
        qw0 |= (fa ? PF_I_FA : 0u) | (fb ? PF_I_FB : 0u);
        if (!live) pw0 &= ~(PF_TR_WW << 18);
    }
}

// The kept instructions appended to code_out, aux1 of the dropped ones since the last kept one
// carried onto the next (the counter contract above); d's code range becomes the appended one.
static inline void append_kept(const Work& T, std::vector<uint32_t>& code_out, pf_set_desc& d) {
    const size_t first = code_out.size() / 4;
    size_t kept = 0;
    for (uint32_t i = 0; i < T.n; i++) kept += !T.drop[i];
    code_out.resize(4 * (first + kept));
    uint32_t* o = code_out.data() + 4 * first;
    uint32_t carry = 0;
    for (uint32_t i = 0; i < T.n; i++) {
        if (T.drop[i]) {
            carry += T.P[4 * (size_t)i + 3];
            continue;
        }
        memcpy(o, T.P.data() + 4 * (size_t)i, 16);
        o[3] += carry;
        carry = 0;
        o += 4;
    }
    d.code_off = (uint32_t)first;
    d.n_ins = (uint32_t)kept;
}

// Sets [s0, s1) of the batch: their device programs appended to code_out, each set's
// code_off rewritten to its offset in code_out.  own (may be null: pf_device_program, whose
// result is read against the caller's pool) collects the sets' own constants.
static inline void device_program_range(const uint32_t* code_fixed, std::vector<pf_set_desc>& descs_out, size_t s0,
                                 size_t s1, std::vector<uint32_t>& code_out, const uint32_t* consts,
                                 size_t n_const, int fold, OwnConsts* own = nullptr, SiteMap* sites = nullptr) {
    Work T;
    for (size_t s = s0; s < s1; s++) {
        pf_set_desc& d = descs_out[s];
        T.n = d.n_ins;
        T.P.assign(code_fixed + 4 * (size_t)d.code_off, code_fixed + 4 * ((size_t)d.code_off + T.n));
        T.drop.assign(T.n, 0);
        if (sites) T.origin.assign(T.n, -1);
        if (fold) fold_constants(T, s, d, consts, n_const, own);
        if (fold != 2) {
            fuse_asserts(T);
            drop_zext_movs(T);
            constant_operands(T, d, consts, n_const, own != nullptr);
            lds_spill_slots(T);
            forward_results(T);
        }
        if (sites) collect_sites(T, *sites);
        append_kept(T, code_out, d);
    }
}

// Host threads for a batch's preparation and the set ranges they take (about equal
// instruction counts): one for small batches (a single query's), up to 8 for large ones —
// and one whenever the sets' code ranges are not disjoint and ascending: check_set copies
// each set's range into one shared buffer, so threads may only get ranges that cannot meet
// (the serial pass takes shared and reordered ranges as it always did).
static inline std::vector<size_t> prep_ranges(const pf_set_desc* descs, size_t n_sets, size_t n_ins) {
    size_t nt = 1;
    if (n_sets >= 64 && n_ins >= (1u << 15)) {
        // hardware_concurrency reads sysfs: once per process, and not on a small batch's path
        static const size_t hw = std::max<size_t>(1, std::thread::hardware_concurrency());
        nt = std::min<size_t>({8, hw, n_sets / 32});
        for (size_t s = 1; s < n_sets && nt > 1; s++)
            if (descs[s].code_off < (uint64_t)descs[s - 1].code_off + descs[s - 1].n_ins) nt = 1;
    }
    std::vector<size_t> cut(nt + 1, n_sets);
    cut[0] = 0;
    uint64_t total = 0, acc = 0;
    for (size_t s = 0; s < n_sets; s++) total += descs[s].n_ins;
    size_t t = 1;
    for (size_t s = 0; s < n_sets && t < nt; s++) {
        acc += descs[s].n_ins;
        if (acc * nt >= total * t) cut[t++] = s + 1;
    }
    return cut;
}

// fn(t) for t in [0, n) on the caller and n - 1 spawned threads
template <typename F>
static void run_ranges(size_t n, F&& fn) {
    std::vector<std::thread> th;
    for (size_t t = 1; t < n; t++) th.emplace_back(fn, t);
    fn(0);
    for (auto& x : th) x.join();
}

// The device program of every set: each range of `cut` rewritten into its own buffer (on its
// own thread), then concatenated in set order — the program one pass over all sets gives.
// pool_out (may be null: no constants of the programs' own) receives the device constant pool
// when it differs from the caller's (else it is left empty): the caller's n_const constants
// verbatim, then, for every set that gained constants of its own, that set's constants again
// followed by the new ones, with the set's const_off pointing there.  n_const of the
// descriptors stays the caller's count — the candidate generator draws from [const_off,
// const_off + n_const) and sees the constants it saw before — and a set without new constants
// keeps its range.
static inline void device_program(const uint32_t* code_fixed, size_t n_fixed, std::vector<pf_set_desc>& descs_out,
                           const std::vector<size_t>& cut, std::vector<uint32_t>& code_out, const uint32_t* consts,
                           size_t n_const, int fold, std::vector<uint32_t>* pool_out = nullptr,
                           SiteMap* sites = nullptr) {
    // (a site map is collected by the serial pass only: its caller passes the one range {0, n_sets})
    const size_t nt = cut.size() - 1, n_sets = descs_out.size();
    code_out.clear();
    const bool owning = pool_out && fold;
    std::vector<OwnConsts> own(owning ? nt : 0);
    for (OwnConsts& o : own) o.cnt.assign(n_sets, 0);
    if (nt == 1) {
        code_out.reserve(n_fixed);
        device_program_range(code_fixed, descs_out, 0, n_sets, code_out, consts, n_const, fold,
                             owning ? &own[0] : nullptr, sites);
    } else {
        std::vector<std::vector<uint32_t>> outs(nt);
        run_ranges(nt, [&](size_t t) {
            device_program_range(code_fixed, descs_out, cut[t], cut[t + 1], outs[t], consts, n_const, fold,
                                 owning ? &own[t] : nullptr);
        });
        size_t total = 0;
        for (const auto& o : outs) total += o.size();
        code_out.reserve(total);
        for (size_t t = 0; t < nt; t++) {
            const uint32_t base = (uint32_t)(code_out.size() / 4);
            for (size_t s = cut[t]; s < cut[t + 1]; s++) descs_out[s].code_off += base;
            code_out.insert(code_out.end(), outs[t].begin(), outs[t].end());
        }
    }
    if (!pool_out) return;
    pool_out->clear();
    size_t n_own = 0;
    for (const OwnConsts& o : own) n_own += o.vals.size();
    if (!n_own) return;  // left empty: the device pool is the caller's, no copy
    if (consts) pool_out->assign(consts, consts + 8 * n_const);
    for (size_t t = 0; t < own.size(); t++) {
        const uint32_t* v = own[t].vals.data();
        for (size_t s = cut[t]; s < cut[t + 1]; s++) {
            const uint32_t k = own[t].cnt[s];
            if (!k) continue;
            pf_set_desc& d = descs_out[s];
            const uint32_t at = (uint32_t)(pool_out->size() / 8);
            if (d.n_const) pool_out->insert(pool_out->end(), consts + 8 * (size_t)d.const_off,
                                            consts + 8 * ((size_t)d.const_off + d.n_const));
            pool_out->insert(pool_out->end(), v, v + 8 * (size_t)k);
            v += 8 * (size_t)k;
            d.const_off = at;
        }
    }
}

// The site map of the batch pf_batch_create would upload (pf_device_sites): the same passes under
// the same gate — fold (the PF_DEVICE_FOLD value) only for batches of PF_FOLD_MIN_SETS sets or
// more, the sets' own constants collected as the upload collects them — on one thread.
static inline SiteMap device_sites(const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                                   const pf_set_desc* descs, size_t n_sets, int fold) {
    const std::vector<uint32_t> fixed = stamped(code, n_ins);
    std::vector<pf_set_desc> d(descs, descs + n_sets);
    std::vector<uint32_t> out, pool;
    SiteMap M;
    device_program(fixed.data(), fixed.size(), d, std::vector<size_t>{0, n_sets}, out, consts, n_const,
                   n_sets >= PF_FOLD_MIN_SETS ? fold : 0, &pool, &M);
    return M;
}

// What prepare_program hands the upload: the device programs, their descriptors, the device
// constant pool (empty: the caller's, see device_program), the per-set wide flags (a W register
// >= PF_NW_NARROW is written: the 16-register kernels) and the largest variable count — or err.
struct Prepared {
    std::vector<uint32_t> code;
    std::vector<pf_set_desc> descs;
    std::vector<uint32_t> pool;
    std::vector<uint8_t> wide;
    uint32_t max_vars = 0;
    std::string err;
};

// Host-side checks of packed programs and their device form (pf_batch_create and
// pf_eval_program).  fold: the PF_DEVICE_FOLD value, applied to batches of PF_FOLD_MIN_SETS
// sets or more.  A large batch (the corpus pass: 1,023 sets, 376k instructions, ~10 ms on one
// host thread) is checked and rewritten in set ranges on host threads, each range's device
// program appended to its own buffer, then concatenated in set order — the same program as the
// serial pass; a range that fails sends the whole batch through the serial pass, so the error
// reported is the first set's, as before.
static inline Prepared prepare_program(const uint32_t* code, size_t n_ins, const uint32_t* consts, size_t n_const,
                                const uint32_t* schema, size_t n_vars, size_t n_parents, const pf_set_desc* descs,
                                size_t n_sets, int fold) {
    Prepared R;
    for (size_t s = 0; s < n_sets; s++) R.max_vars = std::max(R.max_vars, descs[s].n_vars);
    std::vector<uint32_t> code_fixed(4 * n_ins);
    R.wide.assign(n_sets, 0);
    R.descs.assign(descs, descs + n_sets);
    const std::vector<size_t> cut = prep_ranges(descs, n_sets, n_ins);
    const size_t nt = cut.size() - 1;
    bool bad = false;
    if (nt > 1) {
        std::vector<uint8_t> bad_t(nt, 0);
        run_ranges(nt, [&](size_t t) {  // a failing range's message is dropped: the serial pass reports
            for (size_t s = cut[t]; s < cut[t + 1] && !bad_t[t]; s++)
                bad_t[t] = !check_set(s, code, n_ins, n_const, schema, n_vars, n_parents, descs, code_fixed.data(),
                                      R.wide.data()).empty();
        });
        bad = std::find(bad_t.begin(), bad_t.end(), (uint8_t)1) != bad_t.end();
    }
    if (nt == 1 || bad) {
        for (size_t s = 0; s < n_sets && R.err.empty(); s++)
            R.err = check_set(s, code, n_ins, n_const, schema, n_vars, n_parents, descs, code_fixed.data(),
                              R.wide.data());
        if (!R.err.empty()) return R;
    }
    device_program(code_fixed.data(), code_fixed.size(), R.descs, cut, R.code, consts, n_const,
                   n_sets >= PF_FOLD_MIN_SETS ? fold : 0, &R.pool);
    return R;
}

// Longest-first wave order: waves are dispatched in index order, so mapping the first
// waves to the most expensive sets leaves the cheap ones for the last, partly filled
// round.  Weights are measured SIMD cycles per instruction relative to a cheap op
// (EXP ~7.1k, a division ~2.6k, MUL ~750, cheap ~650).  8-register sets
// come first (their launch precedes the 16-register one's).  sites: each set's assert sites
// (the climb contract's witness score).  Both read the device program.
struct WaveOrder {
    std::vector<uint32_t> order, sites;
};
static inline WaveOrder wave_order(const uint32_t* code, const pf_set_desc* descs, size_t n_sets,
                            const std::vector<uint8_t>& wide) {
    WaveOrder R;
    std::vector<uint64_t> cost(n_sets, 0);
    R.sites.assign(n_sets, 0);
    for (size_t s = 0; s < n_sets; ++s) {
        const uint32_t* I = code + 4 * (size_t)descs[s].code_off;
        uint64_t c = 0;
        uint32_t ns = 0;
        for (uint32_t i = 0; i < descs[s].n_ins; ++i) {
            const uint32_t w0 = I[4 * (size_t)i], op = pf_ins_op(w0);
            c += op == PF_W_EXP ? 110u : op == PF_W_MUL ? 12u : pf_op_unit(op) == PF_U_DIV ? 40u : 10u;
            ns += (uint32_t)(op == PF_ASSERT) | (uint32_t)((w0 & PF_I_ASSERT) != 0u);
        }
        cost[s] = c;
        R.sites[s] = ns;
    }
    R.order.resize(n_sets);
    for (size_t s = 0; s < n_sets; ++s) R.order[s] = (uint32_t)s;
    std::stable_sort(R.order.begin(), R.order.end(), [&](uint32_t a, uint32_t b) {
        return wide[a] != wide[b] ? wide[a] < wide[b] : cost[a] > cost[b];
    });
    return R;
}

// ---- link groups (include/pf_bytecode.h, link contract) ---------------------------------
// The host copies pf_batch_create keeps of what a link group's members must share: the device
// descriptors (const_off into the device pool, whose ranges begin with the caller's n_const
// constants), the device constant pool, the schema and the parent values.
struct LinkTables {
    std::vector<uint32_t> consts, schema, parents;
};
// What pf_check_linked checks before it launches anything: ids in range, no empty group, no
// group above PF_LINK_MAX_PARTS, every member equal to its group's first in all the contract
// names.  parts_out[g] = the members of group g.  Returns the error, empty when there is none.
static inline std::string link_validate(const std::vector<pf_set_desc>& descs, const LinkTables& T,
                                        const uint32_t* group_of, uint32_t n_groups,
                                        std::vector<uint32_t>& parts_out) {
    const size_t n_sets = descs.size();
    if (n_groups == 0) return errorf("pf_check_linked: no groups");
    if (!group_of) return errorf("pf_check_linked: null group_of");
    std::vector<uint32_t> parts(n_groups, 0), first(n_groups, 0);
    for (size_t s = 0; s < n_sets; s++) {
        const uint32_t g = group_of[s];
        if (g >= n_groups) return errorf("pf_check_linked: set %zu names group %u of %u", s, g, n_groups);
        if (parts[g]++ == 0) first[g] = (uint32_t)s;
    }
    for (uint32_t g = 0; g < n_groups; g++) {
        if (parts[g] == 0) return errorf("pf_check_linked: group %u is empty", g);
        if (parts[g] > PF_LINK_MAX_PARTS)
            return errorf("pf_check_linked: group %u has %u members (at most %u)", g, parts[g], PF_LINK_MAX_PARTS);
    }
    for (size_t s = 0; s < n_sets; s++) {
        const pf_set_desc &a = descs[first[group_of[s]]], &b = descs[s];
        if (&a == &b) continue;
        const uint32_t g = group_of[s];
        if (a.n_vars != b.n_vars) return errorf("pf_check_linked: group %u: set %zu has %u variables, not %u", g, s, b.n_vars, a.n_vars);
        if (a.n_const != b.n_const) return errorf("pf_check_linked: group %u: set %zu has %u constants, not %u", g, s, b.n_const, a.n_const);
        if (a.seed != b.seed) return errorf("pf_check_linked: group %u: set %zu has another seed", g, s);
        if (a.n_const && memcmp(T.consts.data() + 8 * (size_t)a.const_off, T.consts.data() + 8 * (size_t)b.const_off,
                                32 * (size_t)a.n_const))
            return errorf("pf_check_linked: group %u: set %zu has other constants", g, s);
        for (uint32_t v = 0; v < a.n_vars; v++) {
            const uint32_t* sa = T.schema.data() + 4 * ((size_t)a.var_off + v);
            const uint32_t* sb = T.schema.data() + 4 * ((size_t)b.var_off + v);
            if (sa[0] != sb[0] || sa[1] != sb[1] || sa[2] != sb[2])
                return errorf("pf_check_linked: group %u: set %zu variable %u has another schema entry", g, s, v);
            if ((sa[3] == PF_NO_PARENT) != (sb[3] == PF_NO_PARENT) ||
                (sa[3] != PF_NO_PARENT &&
                 memcmp(T.parents.data() + 8 * (size_t)sa[3], T.parents.data() + 8 * (size_t)sb[3], 32)))
                return errorf("pf_check_linked: group %u: set %zu variable %u has another parent value", g, s, v);
        }
    }
    parts_out = std::move(parts);
    return std::string();
}

}  // namespace pf_devprog

#endif /* PF_DEVPROG_H */
