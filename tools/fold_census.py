#!/usr/bin/env python3
"""Static census of config-3 device programs (host only, no GPU): instructions, weighted cost
(the wave-order weights of pf_batch_create: EXP 110, division 40, MUL 12, other 10) and the
heavy opcodes, for PF_DEVICE_FOLD=0, for pf_device_program (readable against the caller's
pool) and for pf_device_batch (what pf_batch_create uploads, with the device pool).

    python tools/fold_census.py [--sets 1024] [--first 0]
"""

import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mythril_amd import _lib, ir, synth  # noqa: E402

DIV_OPS = (ir.W_UDIV, ir.W_UREM, ir.W_SDIV, ir.W_SREM, ir.W_SMOD, ir.B_UMUL_NOOVF)


def census(code):
    ops = code[:, 0] & 0xFF
    cost = np.full(len(ops), 10, dtype=np.int64)
    cost[ops == ir.W_MUL] = 12
    cost[np.isin(ops, DIV_OPS)] = 40
    cost[ops == ir.W_EXP] = 110
    return {"instructions": len(ops), "cost": int(cost.sum()), "EXP": int((ops == ir.W_EXP).sum()),
            "div": int(np.isin(ops, DIV_OPS).sum()), "MUL": int((ops == ir.W_MUL).sum()),
            "W_VAR": int((ops == ir.W_VAR).sum()), "W_CONST": int((ops == ir.W_CONST).sum())}


def device_program(batch):
    code = np.ascontiguousarray(batch.code, dtype=np.uint32)
    descs = np.ascontiguousarray(batch.descs, dtype=np.uint32)
    consts = np.ascontiguousarray(batch.consts, dtype=np.uint32)
    out, dout, n = np.zeros_like(code), np.zeros_like(descs), ctypes.c_size_t()
    _lib.check(_lib.lib().pf_device_program(
        _lib.ptr_u32(code), len(code), _lib.ptr_u32(consts.reshape(-1)) if consts.size else None, len(consts),
        _lib.ptr_u32(descs), len(descs), _lib.ptr_u32(out), ctypes.byref(n), _lib.ptr_u32(dout)),
        "pf_device_program")
    return out[:n.value], dout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--first", type=int, default=0)
    args = ap.parse_args()

    batch = ir.Batch([synth.random_dag_set(args.first + i, plant=False)[0] for i in range(args.sets)])
    rows = []
    os.environ["PF_DEVICE_FOLD"] = "0"
    rows.append(("PF_DEVICE_FOLD=0", census(device_program(batch)[0])))
    del os.environ["PF_DEVICE_FOLD"]
    rows.append(("pf_device_program", census(device_program(batch)[0])))
    code, descs, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    rows.append(("pf_device_batch", census(code)))
    base, fold = rows[0][1]["cost"], rows[1][1]["cost"]
    for name, c in rows:
        print(f"{name:18s} " + " ".join(f"{k}={v}" for k, v in c.items()) +
              f" cost/unfolded={c['cost'] / base:.4f} cost/device_program={c['cost'] / fold:.4f}")
    own = len(pool) - len(batch.consts)
    moved = int((np.asarray(descs)[:, 2] != np.asarray(batch.descs)[:, 2]).sum())
    print(f"device pool: {len(pool)} constants ({len(batch.consts)} the caller's, {own} added for {moved} sets)")


if __name__ == "__main__":
    main()
