#!/usr/bin/env python3
"""
Median duration of k_spmm<P> (and k_spmv, and the P-column PCG's vector kernels k_mp_*) per instantiation from a rocprofv3 --kernel-trace CSV, with algorithmic bytes
(12 B per stored entry + 16 P B per row + 2 B per row: row length and fixed mask) against 8 TB/s for k_spmm.

    python tools/spmm_medians.py <kernel_trace.csv> <nnz> <rows>
"""
import csv
import json
import re
import sys

import numpy as np


def main():
    path, nnz, rows = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    durs = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            m = re.search(r"k_spmm<(\d+)", name)
            key = "k_spmm<%s>" % m.group(1) if m else ("k_spmv" if re.search(r"\bk_spmv<", name) else None)
            mp = re.search(r"(k_mp_\w+)<(\d+)>", name)
            if mp:
                key = "%s<%s>" % (mp.group(1), mp.group(2))
            if key:
                durs.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    for key in sorted(durs):
        us = float(np.median(durs[key]))
        out = dict(kernel=key, launches=len(durs[key]), median_us=round(us, 2))
        m = re.match(r"k_spmm<(\d+)>", key)
        if m:
            P = int(m.group(1))
            b = 12 * nnz + (16 * P + 2) * rows
            out.update(algorithmic_bytes=b, GBps=round(b / us * 1e-3, 1), frac_of_8TBps=round(b / us * 1e-3 / 8000, 3))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
