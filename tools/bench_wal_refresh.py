#!/usr/bin/env python3
"""Following a growing search WAL file: Engine.refresh_wal_block of an open WAL block against
closing it and opening the grown file again (tools/bench_wal.py's file: the full open is the
baseline), for a file grown by 1 % and by 10 %.

The two ways alternate, `--rounds` times each per growth; medians and the min..max spread are
reported, with the refresh's upload_bytes and kernel_ns and the merge kernel's achieved bytes/s
against its algorithmic bytes (the old block's columns read once, the new block's written
once). Every refreshed handle is checked against the fresh open (info, one search).
Prints one JSON line per growth; --out writes the numbers as a markdown file.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_wal import gen  # noqa: E402


def page_ends(data):
    off, out = 0, []
    while off < len(data):
        off += int.from_bytes(data[off:off + 4], "little")
        out.append(off)
    return out


def column_bytes(info_keys_widths, n):
    """Bytes per entry the merge touches on one side: ds | dur32 | start_s | end_s (16), dur64 (8),
    id (16), start_ns, end_ns (16), root-name ids (8), id length (1), and each term column."""
    return n * (16 + 8 + 16 + 16 + 8 + 1 + sum(info_keys_widths))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=200_000)
    ap.add_argument("--dup", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import tempo_amd as T

    d = tempfile.mkdtemp(prefix="tsg_walr_", dir="/tmp")
    rows = []
    try:
        full = os.path.join(d, "full")
        gen(full, args.entries, 7, args.dup)
        data = open(full, "rb").read()
        ends = page_ends(data)
        path = os.path.join(d, T.wal_filename(T.ENC_SNAPPY))
        eng = T.Engine(devices=[0])
        pipe = T.Pipeline(T.SearchRequest(tags={"service.name": "svc-07", "http.method": "get"}, min_duration_ms=10,
                                          max_duration_ms=1000))
        for pct in (1, 10):
            cut = ends[len(ends) * 100 // (100 + pct) - 1]
            t_ref, t_open, stats = [], [], None
            for _ in range(args.rounds):
                with open(path, "wb") as f:
                    f.write(data[:cut])
                old = eng.open_wal_block(path)
                with open(path, "wb") as f:
                    f.write(data)
                # the refresh (old stays open, closed after the swap: outside the timed part, as in use)
                t = time.perf_counter()
                blk, st = eng.refresh_wal_block(old, path)
                t_ref.append(time.perf_counter() - t)
                # the baseline: close + open of the grown file
                t = time.perf_counter()
                old.close()
                fresh = eng.open_wal_block(path)
                t_open.append(time.perf_counter() - t)
                bi, fi = blk.info(), fresh.info()
                same = all(bi[k] == fi[k] for k in ("entries", "pages", "keys", "fb_bytes", "min_dur_ns", "max_dur_ns", "partial"))
                g0, m0 = eng.search([blk], pipe)
                g1, m1 = eng.search([fresh], pipe)
                same = same and [(m.entry_idx, m.trace_id) for m in g0] == [(m.entry_idx, m.trace_id) for m in g1] \
                    and m0.inspected_bytes == m1.inspected_bytes
                assert st["mode"] == 1 and st["bytes_replayed"] == len(data) - cut and same, (st, same)
                stats, n_new, dev_bytes = st, bi["entries"], bi["device_bytes"]
                n_old = n_new - st["entries_added"]
                blk.close()
                fresh.close()
            # term columns: one byte per key here (narrow keys) unless the block says otherwise; the
            # device_bytes of the block bound it from above, so quote the fixed columns plus one byte per key
            algo = column_bytes([1] * bi["keys"], n_old) + column_bytes([1] * bi["keys"], n_new)
            row = {
                "metric": "WAL refresh vs close + open, file grown by %d %%" % pct, "entries": n_new,
                "appended_bytes": len(data) - cut, "pages_replayed": stats["pages_replayed"],
                "entries_added": stats["entries_added"], "entries_combined": stats["entries_combined"],
                "refresh_ms_median": statistics.median(t_ref) * 1e3, "refresh_ms_min": min(t_ref) * 1e3, "refresh_ms_max": max(t_ref) * 1e3,
                "open_ms_median": statistics.median(t_open) * 1e3, "open_ms_min": min(t_open) * 1e3, "open_ms_max": max(t_open) * 1e3,
                "upload_bytes": stats["upload_bytes"], "kernel_ns": stats["kernel_ns"], "device_bytes": dev_bytes,
                "merge_algorithmic_bytes": algo,
                "merge_GBps": algo / stats["kernel_ns"] if stats["kernel_ns"] else None,
                "rounds": args.rounds,
            }
            rows.append(row)
            print(json.dumps(row), flush=True)
        eng.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("command: python tools/bench_wal_refresh.py --entries %d --dup %g --rounds %d\n\n" % (args.entries, args.dup, args.rounds))
            f.write("| growth | entries | appended bytes | refresh ms (median, min..max) | close + open ms (median, min..max) | upload bytes | kernel us | merge GB/s of algorithmic bytes |\n")
            f.write("|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %d | %.2f (%.2f..%.2f) | %.2f (%.2f..%.2f) | %d | %.1f | %s |\n" % (
                    r["metric"].split("by ")[1], r["entries"], r["appended_bytes"], r["refresh_ms_median"], r["refresh_ms_min"],
                    r["refresh_ms_max"], r["open_ms_median"], r["open_ms_min"], r["open_ms_max"], r["upload_bytes"],
                    r["kernel_ns"] / 1e3, "%.1f" % r["merge_GBps"] if r["merge_GBps"] else "-"))


if __name__ == "__main__":
    main()
