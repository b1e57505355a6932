#!/usr/bin/env python3
"""Times one conntrack GC round over N per-endpoint map pairs (cilium_ct4_<id> and
cilium_ct6_<id> of MapNumEntriesLocal entries, device-owned, at about half load, about
half of the lifetimes below the cutoff) two ways on equal maps: a loop of gf_ct_gc, one
call per map, against one gf_ct_gc_maps over all of them.  Both calls are synchronous, so
the time is the wall clock around them.  Between repetitions the deleted half is put back
into both sets (not timed); the first --warmup repetitions are dropped; the order of the
two alternates.  One JSON line per N with the median, minimum and maximum of each and the
ratio of the medians; the per-map counts of the two must agree.  --prof adds one more
round each under the library's launch profiler (gf_prof_read: device time per phase).

    python tools/gc_round_time.py [--pairs 32,128,256] [--reps 7] [--warmup 2] [--prof]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUT = 100


def entries(v6, n, seed):
    """n distinct CT keys and their entries: the first half expired, the rest alive."""
    from cilium_amd.maps import ctmap
    rng = np.random.default_rng(seed)
    ksz = 40 if v6 else 14
    keys = rng.integers(0, 256, (n, ksz), dtype=np.uint8)
    keys[:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)     # distinct
    if v6:
        keys[:, 38:] = 0
    vals = np.zeros((n, 48), np.uint8)
    vals[: n // 2] = np.frombuffer(ctmap.ct_entry(lifetime=CUT - 50, flags=16), np.uint8)
    vals[n // 2:] = np.frombuffer(ctmap.ct_entry(lifetime=43300, flags=16), np.uint8)
    return np.ascontiguousarray(keys), np.ascontiguousarray(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="32,128,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--entries", type=int, default=0, help="entries per map (default: half of MapNumEntriesLocal)")
    ap.add_argument("--prof", action="store_true")
    a = ap.parse_args()
    import torch
    from cilium_amd import bpf
    from cilium_amd._lib import lib, gf_prof_rec
    from cilium_amd.maps import ctmap
    assert torch.cuda.is_available(), "gc_round_time needs a GPU"
    torch.cuda.set_device(0)
    ne = a.entries or ctmap.MapNumEntriesLocal // 2
    assert ne >= 8192, "a refill of ne / 2 entries must take the device bulk insert (>= 4096)"
    data = {v6: entries(v6, ne, 3 + v6) for v6 in (False, True)}

    def fill(fd, v6, n):                                 # the first n entries (all of them, or the expired half)
        k, v = data[v6]
        bpf.UpdateBatch(fd, k.ctypes.data, v.ctypes.data, n, bpf.BPF_ANY)

    def build(npairs):
        fds = []
        for _ in range(npairs):
            for v6 in (True, False):
                fd = bpf.CreateMap(bpf.BPF_MAP_TYPE_LRU_HASH, 40 if v6 else 14, 48, ctmap.MapNumEntriesLocal)
                fill(fd, v6, ne)
                fds.append((fd, v6))
        return fds

    def loop(fds):
        t0 = time.perf_counter()
        got = [lib.gf_ct_gc(fd, CUT, None) for fd, _ in fds]
        return time.perf_counter() - t0, got

    def single(fds):
        arr = (C.c_int * len(fds))(*[fd for fd, _ in fds])
        out = (C.c_uint32 * len(fds))()
        t0 = time.perf_counter()
        rc = lib.gf_ct_gc_maps(arr, len(fds), CUT, out, None)
        dt = time.perf_counter() - t0
        assert rc == sum(out), rc
        return dt, list(out)

    def prof(fn, fds):
        recs = (gf_prof_rec * 64)()
        lib.gf_prof_enable(1)
        fn(fds)
        k = lib.gf_prof_read(recs, 64)
        lib.gf_prof_enable(0)
        return {recs[j].name.decode(): [recs[j].count, round(recs[j].total_ms, 4)] for j in range(k)}

    for npairs in [int(x) for x in a.pairs.split(",")]:
        A, B = build(npairs), build(npairs)
        tl, ts = [], []
        for rep in range(a.warmup + a.reps):
            if rep:
                for fds in (A, B):
                    for fd, v6 in fds:
                        fill(fd, v6, ne // 2)
            torch.cuda.synchronize()
            if rep % 2:
                (dl, gl), (ds, gs) = loop(A), single(B)
            else:
                (ds, gs), (dl, gl) = single(B), loop(A)
            assert gl == gs == [ne // 2] * len(A), (gl[:4], gs[:4])
            if rep >= a.warmup:
                tl.append(dl * 1e3)
                ts.append(ds * 1e3)
        res = {"pairs": npairs, "maps": len(A), "entries_per_map": ne, "deleted_per_map": ne // 2, "reps": a.reps,
               "loop_ms": {"median": round(float(np.median(tl)), 3), "min": round(min(tl), 3), "max": round(max(tl), 3)},
               "single_ms": {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}}
        res["loop_over_single"] = round(res["loop_ms"]["median"] / res["single_ms"]["median"], 2)
        if a.prof:
            for name, fn, fds in (("loop", loop, A), ("single", single, B)):
                for fd, v6 in fds:
                    fill(fd, v6, ne // 2)
                torch.cuda.synchronize()
                res["prof_" + name] = prof(fn, fds)
        print(json.dumps(res), flush=True)
        for fd, _ in A + B:
            bpf.ObjClose(fd)


if __name__ == "__main__":
    main()
