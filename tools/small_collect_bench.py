#!/usr/bin/env python3
"""Latency of shmem_collectmem on one GPU: the one-kernel small path against the executor
route (SHMEMX_SMALL_COLLECT=0: a lengths fcollect, then PLAN_COLLECT), with
shmem_fcollectmem at the same per-PE bytes beside them (the nearest call the tree had
before collect; its code path is not touched by collect).

  python tools/small_collect_bench.py --out profiles/small_collect.json

starts tools/oshrun at P = 2 and 4 PEs on one GPU (p2p transport), once per route, and
writes one row per (P, residency, per-PE bytes): median microseconds per call over REPS
repeats of CALLS back-to-back calls, and the spread (max - min of the repeats' means).
Every PE contributes the same length, so that fcollect is comparable.  One-GPU figures:
PEs share the device and its queues; nothing here says how 8 GPUs behave.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [8, 64, 512, 4096, 16384, 65536]
REPS, CALLS, WARM = 7, 200, 50


def pe_main():
    from sos_amd import _lib as L
    from sos_amd import shmem as S
    S.shmem_init()
    me, P = S.shmem_my_pe(), S.shmem_n_pes()
    world = S.team_world()
    cap = max(SIZES)
    bufs = {"host": (S.shmem_malloc(cap), S.shmem_malloc(cap * P)),
            "device": (S.shmemx_malloc_device(cap), S.shmemx_malloc_device(cap * P))}
    ctypes.memset(bufs["host"][0], me + 1, cap)
    rows = []
    for res, (src, dst) in bufs.items():
        for n in SIZES:
            for name, fn in (("collect", S.shmem_collectmem), ("fcollect", S.shmem_fcollectmem)):
                before = L.lib().sosx_small_collect_calls()
                for _ in range(WARM):
                    fn(world, dst, src, n)
                means = []
                for _ in range(REPS):
                    S.shmem_barrier_all()
                    t0 = time.perf_counter()
                    for _ in range(CALLS):
                        fn(world, dst, src, n)
                    means.append((time.perf_counter() - t0) / CALLS * 1e6)
                means.sort()
                rows.append({"P": P, "residency": res, "bytes_per_pe": n, "call": name,
                             "us_median": round(means[len(means) // 2], 2),
                             "us_spread": round(means[-1] - means[0], 2),
                             "small_path": L.lib().sosx_small_collect_calls() > before})
    S.shmem_barrier_all()
    if me == 0:
        print("ROWS " + json.dumps(rows), flush=True)
    S.shmem_finalize()


def launch(P, small):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update({"SHMEMX_TRANSPORT": "p2p", "SHMEMX_DEVICE_HEAP_SIZE": "256M", "SHMEMX_STAGE_BYTES": "64M",
                "SHMEMX_DEVICE": "0", "PYTHONPATH": ROOT, "SHMEMX_SMALL_COLLECT": "1" if small else "0"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "oshrun"), "-np", str(P), "--timeout",
                        "150", sys.executable, os.path.abspath(__file__), "--pe"], capture_output=True,
                       text=True, timeout=180, env=env)
    if r.returncode != 0:
        raise SystemExit(f"P={P} small={small} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][-1]
    return json.loads(line[5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pe", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.pe:
        return pe_main()
    table = []
    for P in (2, 4):
        on, off = launch(P, True), launch(P, False)
        key = lambda r: (r["residency"], r["bytes_per_pe"], r["call"])
        off_by = {key(r): r for r in off}
        for r in on:
            if r["call"] != "collect":
                continue
            ex = off_by[key(r)]
            fc = off_by[(r["residency"], r["bytes_per_pe"], "fcollect")]
            spread = max(r["us_spread"], ex["us_spread"], fc["us_spread"])
            wins = r["small_path"] and r["us_median"] + spread < min(ex["us_median"], fc["us_median"])
            table.append({"P": P, "residency": r["residency"], "bytes_per_pe": r["bytes_per_pe"],
                          "small_path_taken": r["small_path"],
                          "small_us": r["us_median"], "small_spread_us": r["us_spread"],
                          "executor_us": ex["us_median"], "executor_spread_us": ex["us_spread"],
                          "fcollect_us": fc["us_median"], "fcollect_spread_us": fc["us_spread"],
                          "small_wins_both_by_more_than_spread": bool(wins)})
    doc = {"what": "us per shmem_collectmem call, every PE contributing bytes_per_pe: small path (one "
                   "kernel over the node shared slots) vs executor route (SHMEMX_SMALL_COLLECT=0) vs "
                   "shmem_fcollectmem at the same bytes (fcollect's path is the one the tree had before "
                   "collect)",
           "how": f"median of {REPS} repeats of {CALLS} back-to-back calls after {WARM} warm-up calls, host "
                  "wall clock on PE 0; spread = max - min of the repeats' means",
           "scope": "P PEs on ONE MI355X, p2p transport; 8-GPU behaviour is unmeasured",
           "rows": table}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
