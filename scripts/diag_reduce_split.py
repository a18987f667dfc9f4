#!/usr/bin/env python3
"""Where the time of reduce_rows_kernel goes: the clock stamps of the diagnostics build (make stamps; SGA_LIB_PATH names it) at the row
counts of the headline's passes.  Every sum runs through sga_debug_reduce_rows on freshly uploaded rows (they miss the L2s, as the rows a
search kernel wrote on other XCDs do).  Usage: diag_reduce_split.py [reps] [rows ...]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import small_gicp_amd as sga

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
counts = [int(a) for a in sys.argv[2:]] or [977, 3907, 15625]
lib, ctx = sga.load(), sga.default_context()
rng = np.random.default_rng(0)
names = ["stage 1 (loads + fold)", "stage row, ticket", "stage 2 (loads + folds)", "result stores", "system fence + barrier"]
print("lib", sga.LIB_PATH, " reps", reps, " (us, median [min .. max]; 100 MHz clock: 0.01 us steps)")
for n in counts:
    rows = np.ascontiguousarray(rng.standard_normal((n, 96)))
    out, st = np.zeros(96), (C.c_ulonglong * 24)()
    rec = []
    for _ in range(reps + 10):
        sga._lib.check(lib.sga_debug_reduce_rows(ctx.h, rows.ctypes.data_as(C.c_void_p), n, 1, out.ctypes.data_as(C.c_void_p)))
        sga._lib.check(lib.sga_debug_reduce_stamps(st))
        rec.append(np.array(st[:], dtype=np.int64))
    rec = np.array(rec[10:]) * 0.01
    G = int(round(rec[0, 23] / 0.01))
    w = rec[:, 16:22]
    start = np.minimum(np.minimum(rec[:, 0], rec[:, 8]), w[:, 0])

    def line(label, v):
        print("  %-44s %6.2f  [%5.2f .. %5.2f]" % (label, np.median(v), v.min(), v.max()))

    print("rows %d, workgroups %d" % (n, G))
    line("entry of the finishing workgroup after the first seen", w[:, 0] - start)
    for k, name in enumerate(names):
        if G == 1 and k in (1, 2):
            continue
        line("finishing workgroup: " + name, w[:, k + 1] - w[:, k])
    line("first workgroup: stage 1", rec[:, 1] - rec[:, 0])
    line("last workgroup: stage 1", rec[:, 9] - rec[:, 8])
    if G > 1:
        line("first workgroup: stage row, ticket", rec[:, 2] - rec[:, 1])
        line("last workgroup: stage row, ticket", rec[:, 10] - rec[:, 9])
    line("first entry seen -> after the fence", w[:, 5] - start)
