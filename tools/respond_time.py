#!/usr/bin/env python3
"""Times gf_respond (k_respond) with the library's launch profiler over one batch at stride 128:
(a) no calls, (b) 1 % calls evenly mixed, (c) every frame a call evenly mixed, and beside (a) a
plain device-to-device copy of the call column's size.  Median of --launches launches after
--warmup, one JSON line.

    python tools/respond_time.py [--n 1000000] [--launches 25] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from cilium_amd import synth
    from cilium_amd._lib import lib, gf_prof_rec
    from cilium_amd.datapath import Datapath
    from tests import respond_model as M

    sc = synth.Scenario("respond_time", host_ifindex=3)
    sc.node = {"ipv4_gateway": int.from_bytes(M.GATEWAY, "little"), "router_ip6": M.ROUTER, "node_mac": M.NODE_MAC}
    dp = Datapath(sc, pin_prefix=None)
    S, n = 128, a.n
    # one well-formed frame per call kind, tiled
    mac, pod = bytes.fromhex("aa1111111111"), bytes.fromhex("f00d000000000000000000000a0b0007")
    kinds = [M.arp_frame(b"\xff" * 6, mac, 1, bytes([10, 11, 0, 7]), M.GATEWAY),
             M.ns_frame(bytes.fromhex("3333ff010000"), mac, pod, b"\xff\x02" + bytes(9) + b"\x01\xff\x01\x00\x00", M.ROUTER),
             M.echo_frame(M.NODE_MAC, mac, pod, M.ROUTER, 1, 1, b"0123456789abcdef"),
             M.ip6_frame(M.NODE_MAC, mac, pod, bytes.fromhex("f00d00000000000000000000c0a80163"), 17, bytes(28), hop=1)]
    rows = np.zeros((4, S), np.uint8)
    for k, f in enumerate(kinds):
        rows[k, :len(f)] = np.frombuffer(f, np.uint8)
    idx = np.arange(n) % 4
    frames = torch.from_numpy(rows[idx]).cuda()
    lens = torch.from_numpy(np.array([len(f) for f in kinds], np.int32)[idx]).cuda()
    snap = torch.empty_like(frames)
    rng = np.random.default_rng(1)
    cols = {"a_no_calls": np.zeros(n, np.uint8),
            "b_1pct_calls": np.where(rng.random(n) < 0.01, idx + 1, 0).astype(np.uint8),
            "c_all_calls": (idx + 1).astype(np.uint8)}
    recs = (gf_prof_rec * 16)()

    def one(call):
        lib.gf_prof_enable(1)
        dp.respond(frames, lens, call, snap_out=snap)
        torch.cuda.synchronize()
        k = lib.gf_prof_read(recs, 16)
        return sum(recs[j].total_ms for j in range(k) if recs[j].name == b"k_respond")

    res = {"n": n, "stride": S, "launches": a.launches}
    for name, col in cols.items():
        call = torch.from_numpy(col).cuda()
        for _ in range(a.warmup):
            one(call)
        res[name + "_ms"] = round(float(np.median([one(call) for _ in range(a.launches)])), 5)
    lib.gf_prof_enable(0)
    src = torch.from_numpy(cols["a_no_calls"]).cuda()
    dst = torch.empty_like(src)
    ts = []
    for k in range(a.warmup + a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            ts.append(e0.elapsed_time(e1))
    res["d2d_copy_bytes"] = n
    res["d2d_copy_ms"] = round(float(np.median(ts)), 5)
    print(json.dumps(res))
    dp.close()


if __name__ == "__main__":
    main()
