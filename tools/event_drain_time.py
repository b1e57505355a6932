#!/usr/bin/env python3
"""Times gf_event_drain (k_evd_count, k_evd_scan, k_evd_scatter, by the library's launch
profiler) over a ring of --n trace records (160 B slots, len_cap 128: a packed record is a whole
slot too, so both modes move the same bytes) of which 0 %, 1 %, 50 % or 100 % pass `--from`, in
slot mode and in packed mode, and beside them two device-to-device hipMemcpyAsync copies: the
whole ring (what a listener needs today before it can look at anything) and just the matched
bytes (the floor of the scatter).  Median of --launches launches after --warmup, one JSON line.

    python tools/event_drain_time.py [--n 1000000] [--launches 25] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = (b"k_evd_count", b"k_evd_scan", b"k_evd_scatter")


def ring_of(n, share, seed=1):
    """n trace records from endpoint 7, a `share` of them (spread at random) from endpoint 5."""
    rng = np.random.default_rng(seed)
    ring = rng.integers(0, 256, (n, 160), dtype=np.uint8)
    ring[:, 0] = 4
    src = np.where(rng.random(n) < share, 5, 7).astype("<u2")
    if share >= 1.0:
        src[:] = 5
    ring[:, 2:4] = src.view(np.uint8).reshape(n, 2)
    ring[:, 12:16] = np.array([128], "<u4").view(np.uint8)
    return ring, int((src == 5).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from cilium_amd import monitor, synth
    from cilium_amd._lib import lib, gf_prof_rec
    from cilium_amd.datapath import Datapath

    n = a.n
    dp = Datapath(synth.Scenario("event_drain_time"), pin_prefix=None)
    recs, cnt, _ = dp.set_event_ring(n)
    out = torch.empty((n, 160), dtype=torch.uint8, device="cuda")
    filt = monitor.EventFilter(frm=(5,))
    prof = (gf_prof_rec * 16)()
    res = {"n": n, "ring_bytes": n * 160, "launches": a.launches}

    def timed(packed):
        def one():
            lib.gf_prof_enable(1)
            _, _, r = dp.event_drain(filt, packed=packed, out_records=out)
            torch.cuda.synchronize()
            k = lib.gf_prof_read(prof, 16)
            return [sum(prof[j].total_ms for j in range(k) if prof[j].name == name) for name in KERNELS], r
        for _ in range(a.warmup):
            one()
        runs = [one() for _ in range(a.launches)]
        ms = np.median(np.array([t for t, _ in runs]), axis=0)
        return [round(float(x), 5) for x in ms], runs[-1][1]

    def copy_ms(nbytes):
        if nbytes == 0:
            return 0.0
        src, dst = recs.view(-1)[:nbytes], out.view(-1)[:nbytes]
        ts = []
        for k in range(a.warmup + a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)                              # hipMemcpyAsync, device to device
            e1.record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 5)

    for share in (0.0, 0.01, 0.5, 1.0):
        ring, want = ring_of(n, share)
        recs.copy_(torch.from_numpy(ring))
        cnt.fill_(n)
        case = {"matched": want, "matched_bytes": want * 160}
        for mode, packed in (("slot", False), ("packed", True)):
            ms, r = timed(packed)
            assert r["matched"] == want and r["written"] == want and r["bytes"] == want * 160, r
            case[mode] = dict(zip(("count_ms", "scan_ms", "scatter_ms"), ms), total_ms=round(sum(ms), 5))
        lib.gf_prof_enable(0)
        case["copy_matched_ms"] = copy_ms(want * 160)
        res[f"match_{int(share * 100)}"] = case
    res["copy_ring_ms"] = copy_ms(n * 160)
    for k, case in res.items():
        if k.startswith("match_"):
            for mode in ("slot", "packed"):
                case[mode]["vs_ring_copy"] = round(case[mode]["total_ms"] / res["copy_ring_ms"], 3)
                if case["copy_matched_ms"]:
                    case[mode]["vs_matched_copy"] = round(case[mode]["total_ms"] / case["copy_matched_ms"], 3)
    print(json.dumps(res))
    filt.close()
    dp.close()


if __name__ == "__main__":
    main()
