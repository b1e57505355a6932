#!/usr/bin/env python3
"""Times gf_lb_classify_frames (k_lb_frames) with the library's launch profiler over one batch at
stride 128: 0 %, 1 % and 100 % of the frames translated, in place and out of place, and beside
them a device-to-device hipMemcpyAsync of the same frame buffer (the floor of the out-of-place
form).  Median of --launches launches after --warmup, one JSON line.

    python tools/lb_frames_time.py [--n 1000000] [--launches 25] [--warmup 5]
"""
import argparse
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
    from cilium_amd.datapath import Datapath, DeviceBatch

    S, n = 128, a.n
    rng = np.random.default_rng(1)
    # 1024 TCP services with 4 backends each (another port: the dport is rewritten too), LB_REDIRECT + LB_DSTMAC
    nsvc, nbe = 1024, 4
    vip = (synth.ip4("10.96.0.1") + np.arange(nsvc)).astype(np.uint32)
    keys = [synth.lb4_keys(vip, np.full(nsvc, 80), np.zeros(nsvc))]
    vals = [synth.lb4_vals(np.zeros(nsvc), np.zeros(nsvc), np.full(nsvc, nbe), np.zeros(nsvc))]
    for s in range(1, nbe + 1):
        keys.append(synth.lb4_keys(vip, np.full(nsvc, 80), np.full(nsvc, s)))
        vals.append(synth.lb4_vals((synth.ip4("10.1.0.0") + np.arange(nsvc) * nbe + s).astype(np.uint32), np.full(nsvc, 8080),
                                   np.zeros(nsvc), 1 + np.arange(nsvc) % 1000))
    sc = synth.Scenario("lb_frames_time")
    sc.add_map(synth.MapSpec("lb4_svc", synth.HASH, 8, 12, 65536, 0, np.concatenate(keys), np.concatenate(vals)))
    sc.lb = {"lb4": "lb4_svc", "lb6": None, "flags": synth.LB_L3 | synth.LB_L4 | synth.LB_REDIRECT, "redirect_ifindex": 2,
             "dstmac": bytes.fromhex("aabbccddeeff")}
    dp = Datapath(sc, pin_prefix=None)
    src = (synth.ip4("100.64.0.0") + rng.integers(0, 1 << 16, n)).astype(np.uint32)
    other = (synth.ip4("192.168.0.0") + rng.integers(0, 1 << 16, n)).astype(np.uint32)
    to_vip = vip[rng.integers(0, nsvc, n)]
    sport = rng.integers(1024, 65536, n)
    recs = (gf_prof_rec * 16)()
    res = {"n": n, "stride": S, "launches": a.launches}

    def one(b, mode):
        lib.gf_prof_enable(1)
        dp.lb_frames(b, snap_out=mode)
        torch.cuda.synchronize()
        k = lib.gf_prof_read(recs, 16)
        return sum(recs[j].total_ms for j in range(k) if recs[j].name == b"k_lb_frames")

    for name, share in (("0pct", 0.0), ("1pct", 0.01), ("100pct", 1.0)):
        pick = rng.random(n) < share
        f, lens = synth.frames_v4(n, S, src, np.where(pick, to_vip, other), synth.TCP, sport, 80, synth.F_ACK, payload=32)
        pk = synth.Packets(f, lens, flow_hash=synth.flow_hash(src, to_vip, sport, 80, synth.TCP))
        b = DeviceBatch(pk, parse=False)
        pristine = b.frames.clone()
        out = torch.empty_like(b.frames)
        o, _, _ = dp.lb_frames(b, snap_out=out)
        torch.cuda.synchronize()
        res[f"translated_{name}"] = int((o[:, 2:4] != 0).any(dim=1).sum().item())
        for _ in range(a.warmup):
            one(b, out)
        res[f"out_of_place_{name}_ms"] = round(float(np.median([one(b, out) for _ in range(a.launches)])), 5)
        ts = []
        for k in range(a.warmup + a.launches):          # in place: every launch starts from the frames as received
            b.frames.copy_(pristine)
            t = one(b, "inplace")
            if k >= a.warmup:
                ts.append(t)
        res[f"in_place_{name}_ms"] = round(float(np.median(ts)), 5)
    lib.gf_prof_enable(0)
    dst = torch.empty_like(pristine)
    ts = []
    for k in range(a.warmup + a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(pristine)                             # hipMemcpyAsync, device to device
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            ts.append(e0.elapsed_time(e1))
    res["d2d_copy_bytes"] = n * S
    res["d2d_copy_ms"] = round(float(np.median(ts)), 5)
    for name in ("0pct", "1pct", "100pct"):
        res[f"out_of_place_{name}_vs_copy"] = round(res[f"out_of_place_{name}_ms"] / res["d2d_copy_ms"], 3)
        res[f"in_place_{name}_vs_copy"] = round(res[f"in_place_{name}_ms"] / res["d2d_copy_ms"], 3)
    print(json.dumps(res))
    dp.close()


if __name__ == "__main__":
    main()
