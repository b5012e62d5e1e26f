"""sosx_strided_copy (strided.hip) on ONE GPU against the HIP runtime's own strided copy
and against the contiguous ceiling.

For 64Mi elements of 4 B and of 8 B at (dst_stride, src_stride) = (1,2), (2,1), (1,8),
(2,3), three ways:
  1. sosx_strided_copy;
  2. hipMemcpy2DAsync with width = elem_size and the pitches set to the strides (the
     runtime's way to do the same copy, as striped_host_ring uses it for its slices);
  3. sosx_gather of the same payload, contiguous: the ceiling.
Every operand is at least 256 MiB (the payload itself), and source plus target exceed the
256 MB last-level cache in every row, so the reads come from HBM.  Each figure is the
median of --reps timings, each a batch of launches between two HIP events after a
warm-up; the spread is (max - min) / median of those timings.  Payload GiB/s counts the
payload once (count * elem_size / time).

If one hipMemcpy2DAsync of a row would take longer than --memcpy2d-limit seconds
(extrapolated from a 64Ki-element call), the runtime copy is timed on fewer elements and
the row says so (`memcpy2d.elems`).

Writes profiles/strided_copy.json (or --out) and prints it.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = [(1, 2), (2, 1), (1, 8), (2, 3)]
D2D = 3  # hipMemcpyDeviceToDevice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elems", type=int, default=64 << 20)
    ap.add_argument("--iters", type=int, default=10, help="launches per timed batch")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--memcpy2d-limit", type=float, default=2.0,
                    help="seconds one runtime 2-D copy may take before it is timed on fewer rows")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "strided_copy.json"))
    a = ap.parse_args()
    import torch
    from sos_amd import _lib as L
    torch.cuda.set_device(0)
    lib = L.lib()
    m2d = lib.hipMemcpy2DAsync
    m2d.restype = ctypes.c_int
    m2d.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                    ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, iters):
        """Median ms per launch and the spread over --reps batches (after a warm-up)."""
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
        med = statistics.median(ms)
        return med, (max(ms) - min(ms)) / med

    def figure(ms, spread, elems, es):
        return {"ms": round(ms, 4), "spread": round(spread, 4), "elems": elems,
                "payload_GiBs": round(elems * es / (ms / 1e3) / 2 ** 30, 1)}

    rows = []
    n = a.elems
    for es in (4, 8):
        for dstr, sst in ROWS:
            sb, db = es * ((n - 1) * sst + 1), es * ((n - 1) * dstr + 1)
            src = torch.empty(sb, dtype=torch.uint8, device="cuda")
            dst = torch.empty(db, dtype=torch.uint8, device="cuda")
            src.random_(0, 256)
            sp, dp = src.data_ptr(), dst.data_ptr()
            row = {"elem_size": es, "dst_stride": dstr, "src_stride": sst, "elems": n}

            def kernel():
                L.strided_copy(dp, dstr, sp, sst, es, n, stream)

            row["strided_copy"] = figure(*timed(kernel, a.iters), n, es)
            # correctness of what was timed: a sample of elements, compared on the device
            dv = dst.view(torch.int32 if es == 4 else torch.int64)[::dstr][:n]
            sv = src.view(torch.int32 if es == 4 else torch.int64)[::sst][:n]
            row["equal"] = bool(torch.equal(dv[:: 4099], sv[:: 4099]))
            print(f"# es={es} d={dstr} s={sst} strided_copy {row['strided_copy']}", file=sys.stderr, flush=True)

            def copy2d(rows_):
                rc = m2d(dp, dstr * es, sp, sst * es, es, rows_, D2D, stream)
                if rc:
                    raise RuntimeError(f"hipMemcpy2DAsync failed ({rc})")

            try:
                probe = min(n, 1 << 16)
                t_probe, _ = timed(lambda: copy2d(probe), 1)
                rows2d = n
                while rows2d > probe and t_probe / 1e3 * (rows2d / probe) > a.memcpy2d_limit:
                    rows2d //= 2
                iters2d = max(1, min(a.iters, int(a.memcpy2d_limit / max(t_probe / 1e3 * rows2d / probe, 1e-6))))
                row["memcpy2d"] = figure(*timed(lambda: copy2d(rows2d), iters2d), rows2d, es)
            except RuntimeError as e:
                row["memcpy2d"] = {"error": str(e)}
            print(f"# es={es} d={dstr} s={sst} memcpy2d {row['memcpy2d']}", file=sys.stderr, flush=True)
            # the ceiling: the same payload, contiguous, through the gather kernel
            csrc = src[:n * es]
            cdst = torch.empty(n * es, dtype=torch.uint8, device="cuda")
            S = (ctypes.c_void_p * 1)(csrc.data_ptr())
            D = (ctypes.c_void_p * 1)(cdst.data_ptr())
            B = (ctypes.c_size_t * 1)(n * es)
            row["gather_contiguous"] = figure(
                *timed(lambda: L.check(lib.sosx_gather(1, S, D, B, stream), "sosx_gather"), a.iters), n, es)
            k, r = row["strided_copy"], row["memcpy2d"]
            if "error" not in r:
                # the kernel wins the row if it is faster by more than both spreads
                row["kernel_over_memcpy2d"] = round(k["payload_GiBs"] / r["payload_GiBs"], 2)
                row["kernel_beats_memcpy2d"] = bool(
                    k["payload_GiBs"] * (1 - k["spread"]) > r["payload_GiBs"] * (1 + r["spread"]))
            row["fraction_of_ceiling"] = round(k["payload_GiBs"] / row["gather_contiguous"]["payload_GiBs"], 3)
            rows.append(row)
            del src, dst, cdst, csrc, dv, sv
            torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "reps": a.reps, "rows": rows,
           "kernel_beats_memcpy2d_every_row": all(r.get("kernel_beats_memcpy2d", False) for r in rows),
           "all_equal": all(r["equal"] for r in rows)}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return 0 if out["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
