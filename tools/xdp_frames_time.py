#!/usr/bin/env python3
"""Times gf_xdp_filter_frames over one batch of config-1 frames at strides 64 and 128, against
  (a) a device-to-device hipMemcpyAsync of the bytes the call writes (n verdict bytes, the
      surviving rows, their len and index words, counts): the floor of its output side;
  (b) what the library offered for the same job before: gf_parse_frames + gf_xdp_classify + a
      torch boolean-mask gather of the frames and of len.
Each figure is the median of --launches runs after --warmup, taken with device events around the
whole call (all its launches; for (b) also the host round trip the gather's size needs).  The
library's launch profiler adds the mean time of each of the call's three kernels.  One JSON line.

    python tools/xdp_frames_time.py [--n 1000000] [--launches 25] [--warmup 5]
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
    from cilium_amd._lib import lib, gf_frames, gf_prof_rec, gf_xdp_frames_out
    from cilium_amd.datapath import Datapath, DeviceBatch

    assert torch.cuda.is_available(), "needs a GPU"
    n = a.n
    res = {"n": n, "launches": a.launches}

    def timed(fn):
        ts = []
        for k in range(a.warmup + a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return round(float(np.median(ts)), 5)

    for S in (64, 128):
        sc = synth.config1(n_packets=n, stride=S)
        dp = Datapath(sc, pin_prefix=None)
        b = DeviceBatch(sc.batches[0])
        e = lambda dt, *shape: torch.empty(shape, dtype=dt, device="cuda")
        v, snap, ln, ix, counts = e(torch.uint8, n), e(torch.uint8, n, S), e(torch.int32, n), e(torch.int32, n), e(torch.int32, 4)
        fr = gf_frames(n, S, b.frames.data_ptr(), b.len.data_ptr())
        o = gf_xdp_frames_out(v.data_ptr(), snap.data_ptr(), ln.data_ptr(), ix.data_ptr(), n, counts.data_ptr())
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def new():
            rc = lib.gf_xdp_filter_frames(dp.xdp_prog, C.byref(fr), C.byref(o), stream())
            assert rc == 0, rc

        def old():
            b.parse()
            vv = dp.xdp(b)
            keep = vv == 2
            return b.frames[keep], b.len[keep]

        new()
        f_old, l_old = old()
        torch.cuda.synchronize()
        k = int(counts[2].item())
        assert k == f_old.shape[0] and torch.equal(snap[:k], f_old) and torch.equal(ln[:k], l_old)
        written = n + k * (S + 8) + 16
        src, dst = e(torch.uint8, written), e(torch.uint8, written)
        t = {"passed": k, "written_bytes": written}
        t["filter_frames_ms"] = timed(new)
        t["parse_classify_gather_ms"] = timed(old)
        t["d2d_copy_ms"] = timed(lambda: dst.copy_(src))
        t["vs_copy"] = round(t["filter_frames_ms"] / t["d2d_copy_ms"], 3)
        t["vs_parse_classify_gather"] = round(t["filter_frames_ms"] / t["parse_classify_gather_ms"], 3)
        recs = (gf_prof_rec * 32)()
        lib.gf_prof_enable(1)
        for _ in range(a.launches):
            new()
        torch.cuda.synchronize()
        for j in range(lib.gf_prof_read(recs, 32)):
            name = recs[j].name.decode()
            if name.startswith("k_xdpf_"):
                t[name + "_ms"] = round(recs[j].total_ms / max(recs[j].count, 1), 5)
        lib.gf_prof_enable(0)
        res[f"stride_{S}"] = t
        dp.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
