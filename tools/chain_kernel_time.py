#!/usr/bin/env python
"""Development tool: what the greedy launch chain's kernels cost per decoded batch, from a kernel trace of a benchmark run.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o NAME -- python bench.py
    python tools/chain_kernel_time.py DIR/.../NAME_kernel_trace.csv [--rows 64] [--max-length 20]

Sums the durations of the chain's kernels (csrc/decoder.hip: dec_gemm_kernel<*>, dec_row_kernel / dec_row2_kernel,
attn_step_kernel, the picks, greedy_init_kernel and search_finalize_kernel) over the run and divides by the number of batches
decoded: the workgroups of all greedy_pick_kernel dispatches (one per row per step) / rows / max_length.  A launch whose
workgroups all return at once (the rows of batches that have ended) still appears with its launch-floor duration, so the
table shows both what the skipped steps no longer cost and what an empty launch still does: where most launches of a kernel
are empty (a benchmark whose clips end after 3 of 20 steps) the MEDIAN duration is an empty launch's.  The rows per chain
are read from the picks' grids (64: lone batches; 256: four batches grouped - under the profiler the host is slower and
forward_async's "auto" pairing finds the decode stream idle, AUDIOCAPTION_PAIR_DECODE=1 makes it wait for full groups).
max_wgs: the largest grid of the kernel, in workgroups.  The convolution kernels' total is printed for scale."""
import argparse
import collections
import csv
import re

CHAIN = ("dec_gemm_kernel", "dec_row2_kernel", "dec_row_kernel", "attn_step_kernel", "greedy_pick_kernel", "sample_kernel",
         "greedy_init_kernel", "search_finalize_kernel")


def short(name):
    m = re.search(r"(\w+_kernel)(<[^>]*>)?", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:60]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--rows", type=int, default=64, help="rows of one batch")
    ap.add_argument("--max-length", type=int, default=20)
    args = ap.parse_args()
    tot, calls, conv = collections.Counter(), collections.Counter(), 0.0
    durs, grid = collections.defaultdict(list), collections.Counter()
    pick_wgs, chain_rows = 0, collections.Counter()
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            name = short(r["Kernel_Name"])
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if name.startswith("conv3x3"):
                conv += us
            if not name.startswith(CHAIN):
                continue
            tot[name] += us
            calls[name] += 1
            durs[name].append(us)
            wgs = 1
            for ax in "XYZ":
                wgs *= max(int(r["Grid_Size_" + ax]) // max(int(r["Workgroup_Size_" + ax]), 1), 1)
            grid[name] = max(grid[name], wgs)
            if name.startswith("greedy_pick_kernel"):
                pick_wgs += wgs
                chain_rows[wgs] += 1
    batches = pick_wgs / args.rows / args.max_length
    print(f"# {args.trace.split('/')[-1]}: {batches:.1f} batches of {args.rows} rows decoded ({args.max_length} steps each)")
    print("# rows per chain (workgroups of a pick launch: chains of that size): "
          + ", ".join(f"{k}: {v / args.max_length:g}" for k, v in sorted(chain_rows.items())))
    print(f"{'calls':>7} {'total_us':>11} {'avg_us':>8} {'median_us':>9} {'max_wgs':>8} {'us/batch':>9}  kernel")
    for name in sorted(tot, key=tot.get, reverse=True):
        med = sorted(durs[name])[len(durs[name]) // 2]
        print(f"{calls[name]:7d} {tot[name]:11.1f} {tot[name] / calls[name]:8.2f} {med:9.2f} {grid[name]:8d} "
              f"{tot[name] / max(batches, 1e-9):9.1f}  {name}")
    s = sum(tot.values())
    print(f"{sum(calls.values()):7d} {s:11.1f} {'':27} {s / max(batches, 1e-9):9.1f}  all chain kernels")
    print(f"{'':7} {conv:11.1f} {'':27} {conv / max(batches, 1e-9):9.1f}  conv3x3* kernels (for scale)")


if __name__ == "__main__":
    main()
