#!/usr/bin/env python3
"""Times gf_tunnel_encap (k_tun_encap, with and without the UDP checksum) and gf_tunnel_decap
(k_tun_decap) with the library's launch profiler over one batch at inner stride 128 and outer
stride 192, VXLAN, every frame selected and every frame as long as its snap (len 128, 178 bytes on
the wire: both kernels move whole rows, so the copy beside them is like for like), and beside each
a device-to-device hipMemcpyAsync of the same output buffer (the copy floor).  The bytes each
kernel reads and writes are printed next to the ratios.  Median of --launches launches after
--warmup, one JSON line.

    python tools/tunnel_time.py [--n 1000000] [--launches 25] [--warmup 5]
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
    from cilium_amd.datapath import Datapath

    S, OS, n = 128, 192, a.n
    z = synth.tunnel_fuzz(n, 0, seed=1, stride=S, negatives=0)
    z.lens[:] = S                                       # whole rows: 50 + 128 of the 192 output bytes written
    dp = Datapath(synth.Scenario("tunnel_time"), pin_prefix=None)
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).cuda()
    frames, lens = dev(z.frames, np.uint8), dev(z.lens, np.int32)
    rip, tid, fh = dev(z.remote_ip, np.int32), dev(z.tunnel_id, np.int32), dev(z.flow_hash, np.int32)
    recs = (gf_prof_rec * 16)()
    res = {"n": n, "inner_stride": S, "outer_stride": OS, "launches": a.launches}

    def timed(kernel, call):
        def one():
            lib.gf_prof_enable(1)
            call()
            torch.cuda.synchronize()
            k = lib.gf_prof_read(recs, 16)
            return sum(recs[j].total_ms for j in range(k) if recs[j].name == kernel)
        for _ in range(a.warmup):
            one()
        return round(float(np.median([one() for _ in range(a.launches)])), 5)

    def copy_ms(t):
        dst = torch.empty_like(t)
        ts = []
        for k in range(a.warmup + a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(t)                                # hipMemcpyAsync, device to device
            e1.record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 5)

    out = torch.empty((n, OS), dtype=torch.uint8, device="cuda")
    for name, flags in (("encap", 0), ("encap_csum", 1)):
        tun = dp.tunnel_load(0, 8472, synth.ip4("192.168.10.1"), flags)
        res[f"{name}_ms"] = timed(b"k_tun_encap", lambda: dp.tunnel_encap(tun, frames, lens, rip, tid, OS, flow_hash=fh, out=out))
    rx = dp.tunnel_load(0, 8472, 0)
    _, olen, _ = dp.tunnel_encap(tun, frames, lens, rip, tid, OS, flow_hash=fh, out=out)
    res["decap_ms"] = timed(b"k_tun_decap", lambda: dp.tunnel_decap(rx, out, olen, inner_stride=S))
    lib.gf_prof_enable(0)
    res["encap_copy_bytes"], res["encap_copy_ms"] = n * OS, copy_ms(out)
    res["decap_copy_bytes"], res["decap_copy_ms"] = n * S, copy_ms(frames)
    # frames, len, remote_ip, tunnel_id, flow_hash in; the row's 178 bytes, out_len, status out
    res["encap_bytes_read"], res["encap_bytes_written"] = n * (S + 16), n * (S + 50 + 5)
    # outer rows and len in; inner row, inner_len, tunnel_id, outer_saddr, opt_len, status out
    res["decap_bytes_read"], res["decap_bytes_written"] = n * (OS + 4), n * (S + 14)
    for name, c in (("encap", "encap"), ("encap_csum", "encap"), ("decap", "decap")):
        res[f"{name}_vs_copy"] = round(res[f"{name}_ms"] / res[f"{c}_copy_ms"], 3)
    print(json.dumps(res))
    dp.close()


if __name__ == "__main__":
    main()
