#!/usr/bin/env python3
"""Crossover of the narrow kernels' terms-first mode (profiles/terms_first): the
bench's block set (10 x 1 M synthetic entries, four resident copies searched in turn) under five
conjunctions of falling selectivity, each with the bench's duration and range filters, with the
mode forced off, forced on and left to the planner. Prints one line per (conjunction, mode): the
device span's p10 / p50 / p90 in us over the timed steps (every fourth step carries
SEARCH_TIME_DEFER, as in bench.py), the step's p50, the matches, and how many of the queries a
terms-first instance served.

  terms_first_sweep.py [--steps 200] [--entries 1000000] [--blocks 10] [--sets 4] [--out FILE.tsv]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T0 = 1_700_000_000
CONJ = [("svc-07", {"service.name": "svc-07"}),
        ("get,error", {"http.method": "get", "status.code": "error"}),
        ("svc-07,get", {"service.name": "svc-07", "http.method": "get"}),
        ("svc-07,error", {"service.name": "svc-07", "status.code": "error"}),
        ("svc-07,get,error", {"service.name": "svc-07", "http.method": "get", "status.code": "error"})]
MODES = (("off", 0), ("on", 1), ("auto", 2))


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))] if v else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--entries", type=int, default=1_000_000)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import tempo_amd as T

    lines = ["conjunction\tmode\tspan_p10_us\tspan_p50_us\tspan_p90_us\tstep_p50_us\tmatches\tterms_first_queries"]
    with tempfile.TemporaryDirectory() as d:
        eng = T.Engine(devices=[0])
        base = []
        for i in range(args.blocks):
            p = os.path.join(d, "b%d" % i)
            T.synth_search_block(p, args.entries, seed=i, profile=0, encoding=T.ENC_SNAPPY, page_size=1024 * 1024)
            base.append(eng.open_block(p))
        sets = [tuple(base)] + [tuple(b.clone(eng) for b in base) for _ in range(args.sets - 1)]
        try:
            for name, tags in CONJ:
                pipe = T.Pipeline(T.SearchRequest(tags=tags, min_duration_ms=10, max_duration_ms=1000, start=T0 + 900,
                                                  end=T0 + 2700))
                for mname, mode in MODES:
                    T.debug_set("terms_first", mode)
                    got, _ = eng.search(list(sets[0]), pipe)
                    for i in range(8):
                        eng.search_raw(sets[i % len(sets)], pipe, flags=0)
                    eng.kernel_times()
                    c0 = eng.resident_counters()["terms_first_queries"]
                    steps = []
                    for i in range(args.steps):
                        t = time.perf_counter()
                        eng.search_raw(sets[i % len(sets)], pipe, flags=T.SEARCH_TIME_DEFER if i % 4 == 2 else 0, metrics=False)
                        steps.append((time.perf_counter() - t) * 1e6)
                    span = [x / 1e3 for x in eng.kernel_times()]
                    tf = eng.resident_counters()["terms_first_queries"] - c0
                    lines.append("%s\t%s\t%.2f\t%.2f\t%.2f\t%.2f\t%d\t%d" % (name, mname, pct(span, 0.1), pct(span, 0.5),
                                                                             pct(span, 0.9), pct(steps, 0.5), len(got), tf))
                    print(lines[-1], flush=True)
        finally:
            T.debug_set("terms_first", 2)
            for s in sets:
                for b in s:
                    b.close()
            eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
