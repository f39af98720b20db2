"""Per-kernel statistics of a rocprofv3 kernel trace, as the kernel_stats_*.csv files under profiles/ hold them.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_streams.py --raw-depth --depth-format u16 --ks 256 --ticks 20
    python tools/rocprof_kernel_stats.py DIR/NAME_results.db > profiles/depth_register/kernel_stats_direct.csv

Reads the `kernels` view of the results database (one row per dispatch: name, grid_x, start, end in nanoseconds), groups the dispatches
by (kernel name without its argument list, grid_x) and prints, longest total first: calls, total milliseconds, and the median, minimum
and maximum duration of one dispatch in microseconds.  Every dispatch of the traced process counts, warm-ups included."""
import collections
import sqlite3
import statistics
import sys


def main(path):
    rows = sqlite3.connect(path).execute("select name, grid_x, (end - start) from kernels").fetchall()
    groups = collections.defaultdict(list)
    for name, grid_x, ns in rows:
        groups[(name.split("(")[0], grid_x)].append(ns)
    print("kernel,grid_x,calls,total_ms,median_us,min_us,max_us")
    for (name, grid_x), v in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
        print('"%s",%d,%d,%.3f,%.1f,%.1f,%.1f' % (name, grid_x, len(v), sum(v) / 1e6, statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: rocprof_kernel_stats.py RESULTS.db")
    main(sys.argv[1])
