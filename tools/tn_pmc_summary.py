"""Per-kernel counter table of rocprofv3 --pmc passes over tools/tn_ab.py --once
(one pass per run, directories p1, p2, ... under the given root): the TN GEMM
instantiations in launch order with the shape each ran at, and the slab reduce.
HBM-side bytes = 2 * FETCH_SIZE + WRITE_SIZE (KiB; the gfx950 correction of
DESIGN.md §8).   python tools/tn_pmc_summary.py <root>"""
import collections
import csv
import glob
import os
import re
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    m = re.search(r"(gemm_lds_kernel<[^>]*>|slab_reduce\w*)", name)
    return m.group(1) if m else None


def main():
    root = sys.argv[1]
    rows = collections.OrderedDict()
    for path in sorted(glob.glob(os.path.join(root, "p*", "**", "*counter_collection.csv"), recursive=True)):
        per, order = collections.defaultdict(dict), []
        for r in csv.DictReader(open(path)):
            k = short(r["Kernel_Name"])
            if not k:
                continue
            d = int(r["Dispatch_Id"])
            if d not in per:
                order.append((d, k))
            per[d][r["Counter_Name"]] = per[d].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
        for n, (d, k) in enumerate(sorted(order)):
            rows.setdefault((n, k), {}).update(per[d])
    for (n, k), c in rows.items():
        hbm = (2 * c.get("FETCH_SIZE", 0) + c.get("WRITE_SIZE", 0)) * 1024 / 1e6
        hit, miss = c.get("TCC_HIT_sum", 0), c.get("TCC_MISS_sum", 0)
        cyc = c.get("GRBM_GUI_ACTIVE", 0) / 8
        print(f"{n:2d} {k:36s} fetch*2 {2 * c.get('FETCH_SIZE', 0) * 1024 / 1e6:7.1f} MB  write "
              f"{c.get('WRITE_SIZE', 0) * 1024 / 1e6:6.1f} MB  hbm {hbm:7.1f} MB  L2 hit {hit / max(hit + miss, 1):.3f}  "
              f"mfma busy "
              f"{c.get('SQ_VALU_MFMA_BUSY_CYCLES', 0) / max(cyc * 1024, 1):.3f}  lds conflict/active "
              f"{c.get('SQ_LDS_BANK_CONFLICT', 0) / max(c.get('SQ_LDS_IDX_ACTIVE', 0), 1):.3f}")


if __name__ == "__main__":
    main()
