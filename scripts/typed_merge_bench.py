#!/usr/bin/env python3
"""Typed merge region timing on the gfx950 kernels: a 64 MiB f32 Sum region
with 1 %, 25 % and 100 % of its elements changed (scattered at random).

Times DeviceSnapshot.typed_diff and DeviceSnapshot.apply_typed_diff as the
fork-join uses them: whole calls on a host clock, each ending in a stream
synchronise. typed_diff includes the copy of the packed diff to the host,
apply_typed_diff the host validation of every index and the upload.
Kernel times come from a kernel trace of this script, one run per fraction
(rocprofv3 --kernel-trace --stats -- python scripts/typed_merge_bench.py
OUT MiB ITERS PCT).
A fraction with a trailing "c" (such as 1c) puts the same number of changes
into one contiguous run, so only few 4 KiB chunks hold one; 0 changes none.
Usage: python scripts/typed_merge_bench.py [out.json] [MiB] [iters] [pcts]"""

import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from faabric_amd import _core

WARMUP = 2


def timed_ms(fn, iters):
    out = None
    times = []
    for i in range(WARMUP + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if i >= WARMUP:
            times.append((t1 - t0) * 1e3)
    return out, times


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/typed_merge.json"
    mib = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    pcts = sys.argv[4].split(",") if len(sys.argv) > 4 else ["1", "25", "100"]
    if not torch.cuda.is_available():
        raise SystemExit("typed_merge_bench needs a GPU")

    nbytes = mib << 20
    n = nbytes // 4
    gen = torch.Generator(device="cuda").manual_seed(7)
    base = torch.rand(n, dtype=torch.float32, device="cuda", generator=gen)
    snap = _core.DeviceSnapshot(nbytes)
    target = _core.DeviceSnapshot(nbytes)
    snap.capture_from_ptr(base.data_ptr())
    dtype = _core.SnapshotDataType.Float
    op = _core.SnapshotMergeOperation.Sum

    rows = []
    for spec in pcts:
        clustered = spec.endswith("c")
        pct = float(spec.rstrip("c"))
        k = int(n * pct / 100.0)
        cur = base.clone()
        if clustered:
            which = torch.arange(k, device="cuda")
        else:
            which = torch.randperm(n, device="cuda", generator=gen)[:k]
        cur[which] += 1.0
        torch.cuda.synchronize()

        diff, diff_ms = timed_ms(
            lambda: snap.typed_diff(cur.data_ptr(), 0, nbytes, dtype, op),
            iters)
        count = 0 if diff is None else (len(diff.data) - 8) // 8
        assert count == k, (count, k)

        def apply_once():
            target.capture_from_ptr(base.data_ptr())
            t0 = time.perf_counter()
            target.apply_typed_diff(diff)
            return (time.perf_counter() - t0) * 1e3

        apply_ms = [0.0]
        if diff is not None:
            apply_ms = [apply_once()
                        for _ in range(WARMUP + iters)][WARMUP:]
            merged = torch.empty_like(base)
            _core.fam_copy_buffer(target.data_ptr, merged.data_ptr(), nbytes)
            want = base.clone()
            want[which] = base[which] + (cur[which] - base[which])
            assert torch.equal(merged, want)

        d_ms = statistics.median(diff_ms)
        a_ms = statistics.median(apply_ms)
        # the diff reads both buffers once; the apply reads an index, a
        # value and the target element per entry
        rows.append({
            "region_mib": mib,
            "changed_pct": pct,
            "placement": "contiguous" if clustered else "scattered",
            "chunks_with_a_change": (k * 4 + 4095) // 4096 if clustered
            else None,
            "entries": count,
            "typed_diff_ms": round(d_ms, 4),
            "typed_diff_read_gbps": round(2 * nbytes / (d_ms / 1e3) / 1e9, 1),
            "apply_typed_diff_ms": round(a_ms, 4),
            "apply_typed_diff_read_gbps":
                round(12 * count / (a_ms / 1e3) / 1e9, 2) if count else None,
            "typed_diff_ms_all": [round(t, 4) for t in diff_ms],
            "apply_typed_diff_ms_all": [round(t, 4) for t in apply_ms],
        })
        print(json.dumps(rows[-1]))

    result = {
        "what": "f32 Sum typed merge region",
        "timing": "host clock around whole synchronous calls, median of "
                  "%d after %d warm-up" % (iters, WARMUP),
        "compared_against": None,
        "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
