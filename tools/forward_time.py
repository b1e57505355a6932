#!/usr/bin/env python3
"""Times gf_forward_frames over one batch of frames at strides 64 and 128, with 4 and 64 queues and
0 / 50 / 100 % of the rows forwarded (the queue column is random over the queues, the rest
GF_FWD_DROP), against
  (a) a device-to-device hipMemcpyAsync of the bytes the call writes (the forwarded rows, their
      len and index words, qoff, counts): the floor of its output side;
  (b) the torch composition a caller would write without it: a stable argsort of the queue
      column, the forwarded count read back on the host, index_select of the rows and of len, and
      a bincount + cumsum for the queue offsets.
Each figure is the median of --launches runs after --warmup, taken with device events around the
whole call (all its launches; for (b) also the host round trip the selection's size needs).  The
library's launch profiler adds the mean time of each of the call's three kernels, and the tool
times gf_forward_queues over pipeline-shaped records once per stride.  One JSON line.

    python tools/forward_time.py [--n 1000000] [--launches 25] [--warmup 5]
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
    from cilium_amd._lib import lib, gf_frames, gf_prof_rec, gf_forward_cfg, gf_forward_out, GF_FWD_DROP, GF_REC_PIPELINE

    assert torch.cuda.is_available(), "needs a GPU"
    n = a.n
    res = {"n": n, "launches": a.launches}
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e = lambda dt, *shape: torch.empty(shape, dtype=dt, device="cuda")

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

    rng = np.random.default_rng(1)
    for S in (64, 128):
        frames = torch.from_numpy(rng.integers(0, 256, (n, S), dtype=np.uint8)).cuda()
        lens = torch.from_numpy(rng.integers(60, 1515, n).astype(np.int32)).cuda()
        snap, ln, ix, counts = e(torch.uint8, n, S), e(torch.int32, n), e(torch.int32, n), e(torch.int32, 4)
        fr = gf_frames(n, S, frames.data_ptr(), lens.data_ptr())
        # the queue column from records: stage POLICY, a third each SHOT / OK / REDIRECT to ifindex 3
        recs = np.zeros((n, 24), np.uint8)
        recs[:, 0], recs[:, 1], recs[:, 8] = 4, rng.choice([2, 0, 7], n), 3
        d_recs, col = torch.from_numpy(recs).cuda(), e(torch.uint8, n)
        cfg = gf_forward_cfg(4, 0, 1, 2, 0, 0, None)
        h = lib.gf_forward_load(C.byref(cfg))
        assert h > 0, h

        def queues():
            rc = lib.gf_forward_queues(h, d_recs.data_ptr(), GF_REC_PIPELINE, n, col.data_ptr(), stream())
            assert rc == 0, rc

        queues()
        res[f"stride_{S}"] = {"forward_queues_ms": timed(queues)}
        lib.gf_obj_close(h)
        for nq in (4, 64):
            for pct in (0, 50, 100):
                q_np = rng.integers(0, nq, n).astype(np.uint8)
                q_np[rng.random(n) >= pct / 100.0] = GF_FWD_DROP
                q = torch.from_numpy(q_np).cuda()
                qoff = e(torch.int32, nq + 1)
                o = gf_forward_out(snap.data_ptr(), ln.data_ptr(), ix.data_ptr(), n, qoff.data_ptr(), counts.data_ptr())

                def new():
                    rc = lib.gf_forward_frames(C.byref(fr), q.data_ptr(), nq, C.byref(o), stream())
                    assert rc == 0, rc

                def old():
                    order = torch.argsort(q, stable=True)
                    k = int((q < nq).sum())
                    sel = order[:k]
                    off = torch.bincount(q.int(), minlength=256)[:nq].cumsum(0)
                    return frames.index_select(0, sel), lens.index_select(0, sel), sel, off

                new()
                f_old, l_old, sel, off = old()
                torch.cuda.synchronize()
                k = int(counts[0].item())
                assert k == f_old.shape[0] and torch.equal(snap[:k], f_old) and torch.equal(ln[:k], l_old)
                assert torch.equal(ix[:k].long(), sel) and torch.equal(qoff[1:].long(), off)
                written = k * (S + 8) + 4 * (nq + 1) + 16
                src, dst = e(torch.uint8, written), e(torch.uint8, written)
                t = {"forwarded": k, "written_bytes": written}
                t["forward_frames_ms"] = timed(new)
                t["argsort_index_select_ms"] = timed(old)
                t["d2d_copy_ms"] = timed(lambda: dst.copy_(src))
                t["vs_copy"] = round(t["forward_frames_ms"] / t["d2d_copy_ms"], 3)
                t["vs_argsort_index_select"] = round(t["forward_frames_ms"] / t["argsort_index_select_ms"], 3)
                prof = (gf_prof_rec * 32)()
                lib.gf_prof_enable(1)
                for _ in range(a.launches):
                    new()
                torch.cuda.synchronize()
                for j in range(lib.gf_prof_read(prof, 32)):
                    name = prof[j].name.decode()
                    if name.startswith("k_fwd_"):
                        t[name + "_ms"] = round(prof[j].total_ms / max(prof[j].count, 1), 5)
                lib.gf_prof_enable(0)
                res[f"stride_{S}"][f"queues_{nq}_fwd_{pct}"] = t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
